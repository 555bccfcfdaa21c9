"""numpy restatement of thrl_tuple_equilibrium (include/thrl.h) from a given tuple_policy array and
tuple_play.tables(): evaluation by doubling and policy iteration on whole arrays, the ordered sums one add at a time."""
import numpy as np

MAX_ITERS = 64


def doublings(gamma):
    """D: the squarings w = w * w from w = gamma until w < 2^-64, stopping at 64."""
    w, D = np.float64(gamma), 0
    while w >= 2.0 ** -64 and D < 64:
        w, D = w * w, D + 1
    return D


def evaluate(R, base, sigma, ts, gamma, D):
    n = base + sigma * ts
    V = R[n]
    w = np.float64(gamma)
    for _ in range(D):
        V, n, w = V + w * V[n], n[n], w * w
    return V


def solve(R, base, pi, nact, ts, gamma):
    """(iters, sigma*, V*, V_pi) of one agent in one game: R [T] its reward per tuple, base [T] the tuple of the others'
    actions with 0 in its place, pi [T] its own (clamped) strategy."""
    D = doublings(gamma)
    sigma = pi.copy()
    acts = np.arange(nact, dtype=np.int64)
    tt = base[:, None] + acts[None, :] * ts
    s_all = np.arange(base.size)
    V_pi = None
    for k in range(MAX_ITERS + 1):
        V = evaluate(R, base, sigma, ts, gamma, D)
        if k == 0:
            V_pi = V
        if k == MAX_ITERS:
            return -1, sigma, V, V_pi
        Q = R[tt] + np.float64(gamma) * V[tt]
        best = np.argmax(Q, axis=1)                                     # the first maximum
        change = Q[s_all, best] > Q[s_all, sigma]
        if not change.any():
            return k, sigma, V, V_pi
        sigma = np.where(change, best, sigma)


def _osum(x):
    s = np.float64(0.0)
    for v in x:
        s = s + v
    return s


def analyse(tabs, policy, start, agents=None, gamma=0.95, policies=False):
    """Every output of thrl_tuple_equilibrium.  gamma: a number, [N] or [N, G]."""
    policy = np.asarray(policy)
    policy = policy.view(np.uint16) if policy.dtype == np.int16 else policy
    start = np.asarray(start, np.int64).reshape(-1)
    G, N, T = policy.shape
    nact = [int(a) for a in tabs["n_actions"]]
    stride = [int(np.prod(nact[i + 1:])) for i in range(N)]
    agents = list(range(N)) if agents is None else sorted(set(int(i) for i in agents))
    gam = np.asarray(gamma, np.float64)
    gam = np.broadcast_to(gam[:, None] if gam.ndim == 1 else gam, (N, G))
    rew = np.asarray(tabs["reward"], np.float64)
    out = {"mu": np.zeros(G, np.int32), "lam": np.zeros(G, np.int32)}
    out.update({f: np.zeros((N, G), np.int32) for f in ("iters", "n_diff_all", "n_diff_on")})
    out.update({f: np.zeros((N, G)) for f in ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on")})
    if policies:
        out.update(br_policy=np.zeros((N, G, T), np.uint16), v_opt=np.zeros((N, G, T)), v_pi=np.zeros((N, G, T)))
    for g in range(G):
        pi = np.stack([np.minimum(policy[g, i].astype(np.int64), nact[i] - 1) for i in range(N)])
        F = (pi * np.asarray(stride)[:, None]).sum(axis=0)
        on = []
        if 0 <= start[g] < T:
            seen, path, t = {}, [], int(start[g])
            while t not in seen:
                seen[t] = len(path)
                path.append(t)
                t = int(F[t])
            out["mu"][g], out["lam"][g] = seen[t], len(path) - seen[t]
            on = path[seen[t]:]
        else:
            out["mu"][g] = -1
        for i in agents:
            if not 0.0 <= gam[i, g] < 1.0:
                out["iters"][i, g] = -1
                for f in ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on"):
                    out[f][i, g] = np.nan
                continue
            base = F - pi[i] * stride[i]
            iters, sig, V, V_pi = solve(rew[i], base, pi[i], nact[i], stride[i], gam[i, g])
            with np.errstate(divide="ignore", invalid="ignore"):
                loss = np.where((V == V_pi) | (V == 0.0), 0.0, (V - V_pi) / V)
            diff = sig != pi[i]
            out["iters"][i, g], out["n_diff_all"][i, g] = iters, diff.sum()
            out["loss_all"][i, g], out["loss_all_mean"][i, g] = loss.max(), _osum(loss) / float(T)
            if on:
                out["n_diff_on"][i, g] = diff[on].sum()
                out["loss_on"][i, g] = loss[on].max()
                out["loss_on_mean"][i, g] = _osum(loss[on]) / float(len(on))
                out["v_on"][i, g] = _osum(V_pi[on]) / float(len(on))
            else:
                out["loss_on"][i, g] = out["loss_on_mean"][i, g] = out["v_on"][i, g] = np.nan
            if policies:
                out["br_policy"][i, g], out["v_opt"][i, g], out["v_pi"][i, g] = sig, V, V_pi
    return out
