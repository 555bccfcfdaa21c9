"""numpy restatement of the tuple walk (thrl_tuple_walk, include/thrl.h) from a given tuple_policy array and
tuple_play.tables(): a plain first-repeat cycle search (not the kernel's Brent search), the same sums in the same order."""
import numpy as np


def next_tuple(tabs, policy, seats_m, t):
    """The tuple the agents seated in one match play at t: entries clamped to the last action, agent 0 slowest."""
    nact = [int(a) for a in tabs["n_actions"]]
    n = 0
    for i, A in enumerate(nact):
        n = n * A + min(int(policy[seats_m[i], i, t]), A - 1)
    return n


def analyse(tabs, policy, seats, start, steps=0, horizon=None):
    """Every output of thrl_tuple_walk: mu, lam, cycle_start [M], cycle_reward, cycle_action [N, M] and the rows
    [steps, N, M] of the path from the start tuple."""
    from th_rl_amd.deviation import default_horizon
    policy = np.asarray(policy).view(np.uint16) if np.asarray(policy).dtype == np.int16 else np.asarray(policy)
    seats, start = np.asarray(seats, np.int64), np.asarray(start, np.int64).reshape(-1)
    G, N, T = policy.shape
    M, K = seats.shape[1], int(steps)
    H = default_horizon([int(a) for a in tabs["n_actions"]]) if horizon is None else int(horizon)
    rew, sca = np.asarray(tabs["reward"], np.float64), np.asarray(tabs["scaled"], np.float64)
    mu, lam, cs = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros(M, np.int32)
    cr, ca = np.zeros((N, M)), np.zeros((N, M))
    rrows, arows = np.zeros((K, N, M)), np.zeros((K, N, M))
    for m in range(M):
        sm = seats[:, m]
        if sm.min() < 0 or sm.max() >= G or not 0 <= start[m] < T:
            mu[m], lam[m], cs[m] = -1, 0, -1
            continue
        path, seen = [int(start[m])], {int(start[m]): 0}
        found = False
        for k in range(1, H + 1):                       # the first repeat closes the cycle at position mu + lam = k
            t = next_tuple(tabs, policy, sm, path[-1])
            if t in seen:
                mu[m], lam[m], cs[m], found = seen[t], k - seen[t], t, True
                break
            seen[t] = k
            path.append(t)
        if not found:
            mu[m], lam[m], cs[m] = H, 0, -1
        else:
            x = int(cs[m])
            r, a = np.zeros(N), np.zeros(N)
            for _ in range(int(lam[m])):
                x = next_tuple(tabs, policy, sm, x)
                r, a = r + rew[:, x], a + sca[:, x]
            cr[:, m], ca[:, m] = r / float(lam[m]), a / float(lam[m])
        x = int(start[m])
        for tau in range(K):
            x = next_tuple(tabs, policy, sm, x)
            rrows[tau, :, m], arows[tau, :, m] = rew[:, x], sca[:, x]
    return {"mu": mu, "lam": lam, "cycle_start": cs, "cycle_reward": cr, "cycle_action": ca, "reward_rows": rrows,
            "action_rows": arows, "horizon": H}


def differs_from_self_play(tabs, policy, seats, start, ref, horizon=None):
    """bool [M]: the match's (mu, lam, cycle_start) differs from the self-play of seat 0's game from the same start."""
    seats = np.asarray(seats, np.int64)
    own = analyse(tabs, policy, np.tile(seats[0], (seats.shape[0], 1)), start, horizon=horizon)
    return (own["mu"] != ref["mu"]) | (own["lam"] != ref["lam"]) | (own["cycle_start"] != ref["cycle_start"])
