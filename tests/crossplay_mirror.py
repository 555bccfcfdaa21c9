"""float64 numpy restatement of cross-play (thrl_crossplay, include/thrl.h) on top of deviation_mirror: match m is the
game whose agent-i table is agent i's block of q[seats[i][m]], so the mirror assembles those tables and hands them to
deviation_mirror.Game -- its first-repeat cycle search (not the kernel's Brent search) and its transition."""
import numpy as np

import deviation_mirror as M


def cross_tables(config, q, seats):
    """q_cross [M, stride]: agent i's block of q[seats[i][m]] for every i."""
    ag, _, _ = M.params(config)
    q, seats = np.asarray(q), np.asarray(seats, np.int64)
    out = np.empty((seats.shape[1], q.shape[1]), q.dtype)
    off = 0
    for i, p in enumerate(ag):
        n = (p["states"] + 1) * p["actions"]
        out[:, off:off + n] = q[seats[i], off:off + n]
        off += n
    return out


def analyse(config, q, seats, state0, steps=0, horizon=None):
    """Every output of thrl_crossplay for seats inside the batch: mu, lam, cycle_reward, cycle_action, the rows
    [steps, N, M] of the path from x_0, and s_key [M] (the row tuple s* as one integer)."""
    from th_rl_amd.deviation import default_horizon
    g = M.Game(config, cross_tables(config, q, seats))
    N, G, K = g.N, g.G, int(steps)
    H = default_horizon([p["actions"] for p in g.ag]) if horizon is None else int(horizon)
    state0 = np.asarray(state0, np.float64)
    x0 = [M.encode(state0, g.ag[i]) for i in range(N)]
    mu, lam, s, _ = g.cycle(x0, H)
    cr = [np.zeros(G) for _ in range(N)]
    ca = [np.zeros(G) for _ in range(N)]
    x = [r.copy() for r in s]
    for j in range(int(lam.max()) if lam.size else 0):
        sc, rew, nx = g.transition(g.greedy(x))
        on = j < lam
        for i in range(N):
            cr[i] = np.where(on, cr[i] + rew[i], cr[i])
            ca[i] = np.where(on, ca[i] + sc[i], ca[i])
        x = nx
    with np.errstate(invalid="ignore", divide="ignore"):
        cr = [np.where(lam > 0, c / lam, 0.0) for c in cr]
        ca = [np.where(lam > 0, c / lam, 0.0) for c in ca]
    rrows, arows = np.zeros((K, N, G)), np.zeros((K, N, G))
    x = [r.copy() for r in x0]
    for t in range(K):
        sc, rew, x = g.transition(g.greedy(x))
        for i in range(N):
            rrows[t, i], arows[t, i] = rew[i], sc[i]
    return {"mu": mu.astype(np.int32), "lam": lam.astype(np.int32), "cycle_reward": np.stack(cr),
            "cycle_action": np.stack(ca), "reward_rows": rrows, "action_rows": arows, "s_key": g.key(s), "horizon": H}


def differs_from_self_play(config, q, seats, state0, ref, horizon=None):
    """bool [M]: the match's (mu, lam, s*) differs from the self-play of seat 0's game from the same start price."""
    seats = np.asarray(seats, np.int64)
    own = analyse(config, q, np.tile(seats[0], (seats.shape[0], 1)), state0, horizon=horizon)
    return (own["mu"] != ref["mu"]) | (own["lam"] != ref["lam"]) | (own["s_key"] != ref["s_key"])


def policies(config, q):
    """uint16 [G, P]: every row's first maximum, agent 0's rows first (the layout of thrl_policy_track)."""
    return np.concatenate([np.argmax(t, axis=2) for t in M.split_tables(config, q)], axis=1).astype(np.uint16)
