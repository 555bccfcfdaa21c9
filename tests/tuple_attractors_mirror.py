"""numpy restatement of thrl_tuple_attractors (include/thrl.h) from a given tuple_policy array and the per-config
tables: every tuple's path is walked step by step, the ordered sums are added one term at a time."""
import numpy as np

KEEP = 8


def greedy_map(n_actions, pol):
    """F [T] of one game: pol [N, T] with entries clamped to the agent's last action, agent 0 slowest."""
    n_actions = [int(x) for x in n_actions]
    F = np.zeros(pol.shape[1], np.int64)
    stride = 1
    for i in range(len(n_actions) - 1, -1, -1):
        F += np.minimum(pol[i].astype(np.int64), n_actions[i] - 1) * stride
        stride *= n_actions[i]
    return F


def structure(F):
    """(rep [T], mu [T], lam {rep: length}) of the map F, by walking."""
    T = F.size
    F = [int(x) for x in F]
    rep, mu = [-1] * T, [-1] * T
    lam = {}
    for t0 in range(T):
        if rep[t0] >= 0:
            continue
        path, at = [], {}
        t = t0
        while rep[t] < 0 and t not in at:
            at[t] = len(path)
            path.append(t)
            t = F[t]
        if rep[t] < 0:                                  # closed on itself: path[at[t]:] is a new cycle
            cyc = path[at[t]:]
            r = min(cyc)
            lam[r] = len(cyc)
            for c in cyc:
                rep[c], mu[c] = r, 0
            path = path[:at[t]]
        for k, s in enumerate(reversed(path)):          # the tail, from the tuple next to what is known
            rep[s], mu[s] = rep[t], mu[t] + k + 1
    return np.array(rep, np.int64), np.array(mu, np.int64), lam


def cycle_mean(F, tab, r, lam):
    """(sum over F(r), F^2(r), .., F^lam(r) in that order from 0.0) / lam."""
    s, c = 0.0, int(r)
    for _ in range(lam):
        c = int(F[c])
        s = s + float(tab[c])
    return s / float(lam)


def analyse(tabs, policy, start, start_w=None, policies=False):
    """tabs: T, n_actions, reward [N, T], scaled [N, T]; policy uint16 [G, N, T]; start int [G]; start_w [T] or None."""
    T = int(tabs["T"])
    reward, scaled = np.asarray(tabs["reward"], np.float64), np.asarray(tabs["scaled"], np.float64)
    policy = np.asarray(policy)
    G, N = policy.shape[0], policy.shape[1]
    start = np.asarray(start).reshape(G)
    out = {f: np.zeros(G, np.int32) for f in ("n_attr", "mu_max", "n_cycle_states", "rep_x0", "mu_x0", "slot_x0")}
    out.update(rep=np.full((KEEP, G), -1, np.int32), lam=np.zeros((KEEP, G), np.int32), basin=np.zeros((KEEP, G), np.int32),
               cycle_reward=np.zeros((KEEP, N, G)), cycle_action=np.zeros((KEEP, N, G)))
    if start_w is not None:
        w = np.asarray(start_w, np.float64).reshape(T)
        out.update(start_mass=np.zeros((KEEP, G)), start_mass_other=np.zeros(G), start_reward=np.zeros((N, G)))
    if policies:
        out.update(tuple_rep=np.zeros((G, T), np.uint16), tuple_mu=np.zeros((G, T), np.uint16))
    for g in range(G):
        F = greedy_map(tabs["n_actions"], policy[g])
        rep, mu, lam = structure(F)
        basin = np.bincount(rep, minlength=T)
        order = sorted(lam, key=lambda r: (-int(basin[r]), r))
        slot = {r: k for k, r in enumerate(order[:KEEP])}
        out["n_attr"][g], out["mu_max"][g], out["n_cycle_states"][g] = len(order), mu.max(), sum(lam.values())
        for r, k in slot.items():
            out["rep"][k, g], out["lam"][k, g], out["basin"][k, g] = r, lam[r], basin[r]
            for i in range(N):
                out["cycle_reward"][k, i, g] = cycle_mean(F, reward[i], r, lam[r])
                out["cycle_action"][k, i, g] = cycle_mean(F, scaled[i], r, lam[r])
        t0 = int(start[g])
        if 0 <= t0 < T:
            out["rep_x0"][g], out["mu_x0"][g], out["slot_x0"][g] = rep[t0], mu[t0], slot.get(int(rep[t0]), -1)
        else:
            out["rep_x0"][g] = out["mu_x0"][g] = out["slot_x0"][g] = -1
        if start_w is not None:
            cr = {r: [cycle_mean(F, reward[i], r, lam[r]) for i in range(N)] for r in order}
            mass, other, rew = [0.0] * KEEP, 0.0, [0.0] * N
            for t in range(T):
                r, wt = int(rep[t]), float(w[t])
                if r in slot:
                    mass[slot[r]] = mass[slot[r]] + wt
                else:
                    other = other + wt
                for i in range(N):
                    rew[i] = rew[i] + wt * cr[r][i]
            out["start_mass"][:, g], out["start_mass_other"][g], out["start_reward"][:, g] = mass, other, rew
        if policies:
            out["tuple_rep"][g], out["tuple_mu"][g] = rep, mu
    return out
