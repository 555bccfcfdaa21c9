"""numpy restatement of the attractor analysis (thrl_attractors, include/thrl.h), written from its definitions on top
of equilibrium_mirror's plan and deviation_mirror's encode / scale.  One game at a time; every state is WALKED step by
step to the first state its path repeats (the kernel never walks: it doubles pointers), and the sums are taken in the
stated order.  brute_structure() restates mu / rep / lam once more from the powers of the map, to hold the walk
against on small maps.
"""
import numpy as np

import deviation_mirror as M
import equilibrium_mirror as E

KEEP = 8


def map_structure(f):
    """(mu, rep, lam) of every state of the map f [S] by walking each state to its first repeat."""
    f = [int(v) for v in f]
    S = len(f)
    mu, rep, lam = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    for s in range(S):
        seen, path, c = {}, [], s
        while c not in seen:
            seen[c] = len(path)
            path.append(c)
            c = f[c]
        mu[s] = seen[c]
        cyc = path[seen[c]:]
        rep[s], lam[s] = min(cyc), len(cyc)
    return mu, rep, lam


def brute_structure(f):
    """The same from the definitions on the powers of f: c is on a cycle iff f^k(c) = c for some 1 <= k <= S."""
    f = np.asarray(f, np.int64)
    S = f.size
    powers = [np.arange(S)]
    for _ in range(2 * S):
        powers.append(f[powers[-1]])
    P = np.stack(powers)                                        # P[k][s] = f^k(s)
    on = np.array([any(P[k][s] == s for k in range(1, S + 1)) for s in range(S)])
    mu = np.array([min(k for k in range(S + 1) if on[P[k][s]]) for s in range(S)])
    rep = np.array([min(P[mu[s] + k][s] for k in range(S)) for s in range(S)])
    lam = np.array([min(k for k in range(1, S + 1) if P[mu[s] + k][s] == P[mu[s]][s]) for s in range(S)])
    return mu, rep, lam


def ordered(f, rep, mu):
    """The attractors [(rep, basin)] in the reported order: basin descending, ties by rep ascending."""
    reps, counts = np.unique(rep, return_counts=True)
    return sorted(zip(reps.tolist(), counts.tolist()), key=lambda rb: (-rb[1], rb[0]))


def policies(config, q):
    """policy [G, P] uint16 of the tables q [G, stride]: argmax of every row, agent 0's rows first."""
    tab = M.split_tables(config, q)
    return np.concatenate([np.argmax(t, axis=2) for t in tab], axis=1).astype(np.uint16)


def ordered_sum(x):
    s = 0.0
    for v in x:
        s = s + float(v)
    return s


def analyse(config, q, state0, policy=None, reset=None, n_games=None):
    """Every output of thrl_attractors.  policy [G, P]: played in place of q's greedy policies (entries clamped).
    reset: (rows [N, J], w [J]) or None."""
    pl = E.plan(config)
    N, S = pl["N"], pl["S"]
    if policy is None:
        policy = policies(config, q)
    policy = np.asarray(policy).astype(np.int64)
    G = policy.shape[0] if n_games is None else int(n_games)
    roff = np.concatenate([[0], np.cumsum([p["states"] + 1 for p in pl["ag"]])])
    state0 = np.asarray(state0, np.float64)
    sc_lut = [M.scale(np.arange(pl["n_actions"][i]), pl["ag"][i]) for i in range(N)]

    def act(g, i, row):
        return min(int(policy[g, roff[i] + row]), pl["n_actions"][i] - 1)

    out = {f: np.zeros(G, np.int32) for f in ("n_attr", "mu_max", "n_cycle_states", "rep_x0", "mu_x0", "slot_x0")}
    out["rep"] = np.full((KEEP, G), -1, np.int32)
    out["lam"], out["basin"] = np.zeros((KEEP, G), np.int32), np.zeros((KEEP, G), np.int32)
    out["cycle_reward"], out["cycle_action"] = np.zeros((KEEP, N, G)), np.zeros((KEEP, N, G))
    out["state_rep"], out["state_mu"] = np.zeros((G, S), np.uint16), np.zeros((G, S), np.uint16)
    if reset is not None:
        rows, w = np.asarray(reset[0], np.int64), np.asarray(reset[1], np.float64)
        out["reset_mass"], out["reset_mass_other"] = np.zeros((KEEP, G)), np.zeros(G)
        out["reset_reward"] = np.zeros((N, G))
    for g in range(G):
        a = [[act(g, i, int(pl["srow"][i][s])) for s in range(S)] for i in range(N)]
        tup = [sum(a[i][s] * pl["tstride"][i] for i in range(N)) for s in range(S)]
        f = [int(pl["sid"][t]) for t in tup]
        mu, rep, lam = map_structure(f)
        attr = ordered(f, rep, mu)
        slot = {r: k for k, (r, _) in enumerate(attr)}
        lam_of = {int(rep[s]): int(lam[s]) for s in range(S)}

        def means(r):
            cr, ca, c = [0.0] * N, [0.0] * N, r
            for _ in range(lam_of[r]):
                for i in range(N):
                    cr[i] = cr[i] + float(pl["rew"][i][tup[c]])
                    ca[i] = ca[i] + float(sc_lut[i][a[i][c]])
                c = f[c]
            return [x / float(lam_of[r]) for x in cr], [x / float(lam_of[r]) for x in ca]

        out["n_attr"][g], out["mu_max"][g] = len(attr), mu.max()
        out["n_cycle_states"][g] = sum(lam_of[r] for r, _ in attr)
        out["state_rep"][g], out["state_mu"][g] = rep, mu
        for k, (r, b) in enumerate(attr[:KEEP]):
            out["rep"][k, g], out["lam"][k, g], out["basin"][k, g] = r, lam_of[r], b
            cr, ca = means(r)
            out["cycle_reward"][k, :, g], out["cycle_action"][k, :, g] = cr, ca
        # the training state: the path of row tuples from x_0, walked to its first repeat
        x = tuple(int(M.encode(state0[g], pl["ag"][i])) for i in range(N))
        seen, traj = {}, []
        while x not in seen:
            seen[x] = len(traj)
            traj.append(x)
            t = sum(act(g, i, x[i]) * pl["tstride"][i] for i in range(N))
            x = tuple(int(r) for r in pl["srow"][:, pl["sid"][t]])
        r0 = min(pl["ids"][r] for r in traj[seen[x]:])
        out["rep_x0"][g], out["mu_x0"][g] = r0, seen[x]
        out["slot_x0"][g] = slot[r0] if slot[r0] < KEEP else -1
        if reset is not None:
            mass, other, rr = [0.0] * KEEP, 0.0, [0.0] * N
            cache = {}
            for j in range(w.size):
                t = sum(act(g, i, int(np.clip(rows[i, j], 0, pl["ag"][i]["states"]))) * pl["tstride"][i] for i in range(N))
                r = int(rep[pl["sid"][t]])
                if slot[r] < KEEP:
                    mass[slot[r]] = mass[slot[r]] + float(w[j])
                else:
                    other = other + float(w[j])
                if r not in cache:
                    cache[r] = means(r)[0]
                for i in range(N):
                    rr[i] = rr[i] + float(w[j]) * cache[r][i]
            out["reset_mass"][:, g], out["reset_mass_other"][g], out["reset_reward"][:, g] = mass, other, rr
    out["n_states"] = S
    return out


def fixed_point_tables(config, n_games=1):
    """Tables [n_games, stride] under which EVERY state is a fixed point: in state s each agent plays its action of
    the first tuple that produces s."""
    pl = E.plan(config)
    strat = []
    for i in range(pl["N"]):
        s_i = np.zeros(pl["ag"][i]["states"] + 1, np.int64)
        for s in range(pl["S"]):
            t = int(np.flatnonzero(pl["sid"] == s)[0])
            s_i[pl["srow"][i][s]] = (t // pl["tstride"][i]) % pl["n_actions"][i]
        strat.append(s_i)
    return E.strategy_tables(config, strat, n_games)
