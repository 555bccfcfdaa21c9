"""float64 numpy restatement of the equilibrium check (thrl_equilibrium, include/thrl.h), written from its
definitions on top of deviation_mirror's encode / scale / env_step.  One game at a time, all states at once; the
cycle is found from the definition (the first row tuple of the trajectory that repeats an earlier one).  Also an
independent solver (plain value iteration) to hold the scheme itself against, and the hand-built strategies of the
known answers.
"""
import numpy as np

import deviation_mirror as M

MAX_ITERS = 64
MAX_D = 64


def plan(config):
    """The per-config tables: T, S, rew [N, T], sid [T], srow [N, S], tstride [N], n_actions [N]."""
    ag, a, b = M.params(config)
    N = len(ag)
    nact = [p["actions"] for p in ag]
    T = int(np.prod(nact))
    idx = np.unravel_index(np.arange(T), nact)                  # agent 0 slowest
    sc = [M.scale(idx[i], ag[i]) for i in range(N)]
    p, rew = M.env_step(sc, a, b)
    rows = np.stack([M.encode(p, ag[i]) for i in range(N)], axis=1)     # [T, N]
    ids, srow, sid = {}, [], np.zeros(T, np.int64)
    for t in range(T):
        key = tuple(int(v) for v in rows[t])
        if key not in ids:
            ids[key] = len(srow)
            srow.append(key)
        sid[t] = ids[key]
    tstride = [int(np.prod(nact[i + 1:])) for i in range(N)]
    return dict(ag=ag, N=N, T=T, S=len(srow), rew=np.stack(rew), sid=sid, srow=np.array(srow, np.int64).T.copy(),
                tstride=tstride, n_actions=nact, ids=ids)


def doublings(gamma):
    w, d = float(gamma), 0
    while w >= 2.0 ** -64 and d < MAX_D:
        w = w * w
        d += 1
    return d


def problem(pl, pol, i):
    """R [S, A] and nxt [S, A] of agent i against the others' strategies pol [N][S]."""
    base = np.zeros(pl["S"], np.int64)
    for j in range(pl["N"]):
        if j != i:
            base = base + pol[j] * pl["tstride"][j]
    tt = base[:, None] + np.arange(pl["n_actions"][i])[None, :] * pl["tstride"][i]
    return pl["rew"][i][tt], pl["sid"][tt]


def evaluate(R, nxt, sigma, gamma):
    ar = np.arange(R.shape[0])
    V, n, w = R[ar, sigma].copy(), nxt[ar, sigma].copy(), float(gamma)
    for _ in range(doublings(gamma)):
        V = V + w * V[n]
        n = n[n]
        w = w * w
    return V


def solve(pl, pol, i, gamma):
    """(iters, sigma*, V*, V_pi) of agent i: policy iteration from its own strategy, the incumbent kept on ties."""
    R, nxt = problem(pl, pol, i)
    ar = np.arange(pl["S"])
    sigma = np.asarray(pol[i], np.int64).copy()
    k = 0
    while True:
        V = evaluate(R, nxt, sigma, gamma)
        if k == 0:
            v_pi = V
        if k == MAX_ITERS:
            return -1, sigma, V, v_pi
        Q = R + float(gamma) * V[nxt]
        best = np.argmax(Q, axis=1)                 # first maximum
        better = Q[ar, best] > Q[ar, sigma]
        if not better.any():
            return k, sigma, V, v_pi
        sigma = np.where(better, best, sigma)
        k += 1


def value_iteration(R, nxt, gamma):
    """Independent solver: W <- max_a (R + gamma W[nxt]) from 0, n sweeps with gamma^n < 2^-64."""
    W = np.zeros(R.shape[0])
    g, w, n = float(gamma), 1.0, 0
    while w >= 2.0 ** -64:
        w *= g
        n += 1
    for _ in range(n):
        W = (R + g * W[nxt]).max(axis=1)
    return W


def losses(v_opt, v_pi):
    same = (v_opt == v_pi) | (v_opt == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(same, 0.0, (v_opt - v_pi) / np.where(v_opt == 0.0, 1.0, v_opt))


def ordered_sum(x):
    s = 0.0
    for v in x:
        s = s + float(v)
    return s


def analyse(config, q, state0, agents=None, gamma=None):
    """Every output of thrl_equilibrium, with the per-state arrays.  gamma: [N, G] per-game (a sweep) or None."""
    pl = plan(config)
    N, S = pl["N"], pl["S"]
    tab = M.split_tables(config, q)
    G = tab[0].shape[0]
    agents = list(range(N)) if agents is None else sorted(agents)
    state0 = np.asarray(state0, np.float64)
    out = {"mu": np.zeros(G, np.int32), "lam": np.zeros(G, np.int32)}
    for f in ("iters", "n_diff_all", "n_diff_on"):
        out[f] = np.zeros((N, G), np.int32)
    for f in ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on"):
        out[f] = np.zeros((N, G))
    out["br_policy"] = np.zeros((N, G, S), np.uint16)
    out["v_opt"], out["v_pi"] = np.zeros((N, G, S)), np.zeros((N, G, S))
    for g in range(G):
        pol = [np.argmax(tab[i][g][pl["srow"][i]], axis=1) for i in range(N)]
        # the path of row tuples from x_0
        x = tuple(int(M.encode(state0[g], pl["ag"][i])) for i in range(N))
        seen, traj = {}, []
        while x not in seen:
            seen[x] = len(traj)
            traj.append(x)
            acts = [int(np.argmax(tab[i][g][x[i]])) for i in range(N)]
            t = sum(acts[i] * pl["tstride"][i] for i in range(N))
            x = tuple(int(v) for v in pl["srow"][:, pl["sid"][t]])
        mu = seen[x]
        lam = len(traj) - mu
        cyc = [pl["ids"][r] for r in traj[mu:]]
        out["mu"][g], out["lam"][g] = mu, lam
        for i in agents:
            gam = float(gamma[i][g]) if gamma is not None else pl["ag"][i]["gamma"]
            it, sig, v_opt, v_pi = solve(pl, pol, i, gam)
            ls = losses(v_opt, v_pi)
            diff = sig != pol[i]
            out["iters"][i, g] = it
            out["n_diff_all"][i, g], out["n_diff_on"][i, g] = diff.sum(), diff[cyc].sum()
            out["loss_all"][i, g], out["loss_on"][i, g] = ls.max(), ls[cyc].max()
            out["loss_all_mean"][i, g] = ordered_sum(ls) / float(S)
            out["loss_on_mean"][i, g] = ordered_sum(ls[cyc]) / float(lam)
            out["v_on"][i, g] = ordered_sum(v_pi[cyc]) / float(lam)
            out["br_policy"][i, g], out["v_opt"][i, g], out["v_pi"][i, g] = sig, v_opt, v_pi
    out["n_states"] = S
    return out


# ---------------------------------------------------------------------------------------------- known answers
def strategy_tables(config, strategies, n_games=1):
    """[n_games, stride] float64 tables in which agent i plays strategies[i][row] at every row (one-hot rows);
    strategies[i]: an action index for every row, or an array [states + 1]."""
    ag, _, _ = M.params(config)
    flat = []
    for p, s in zip(ag, strategies):
        rows = p["states"] + 1
        t = np.zeros((rows, p["actions"]))
        t[np.arange(rows), np.broadcast_to(np.asarray(s, np.int64), (rows,))] = 1.0
        flat.append(t.ravel())
    return np.tile(np.concatenate(flat)[None, :], (n_games, 1))


def static_best_responses(pl):
    """All action pairs (a0, a1) of a two-agent plan that are mutual one-period best responses (first maximum)."""
    A0, A1 = pl["n_actions"]
    r0 = pl["rew"][0].reshape(A0, A1)
    r1 = pl["rew"][1].reshape(A0, A1)
    return [(a0, a1) for a0 in range(A0) for a1 in range(A1)
            if int(np.argmax(r0[:, a1])) == a0 and int(np.argmax(r1[a0, :])) == a1]
