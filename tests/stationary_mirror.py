"""numpy restatement of the stationary analysis (thrl_stationary, include/thrl.h), written from its definitions on top
of th_rl_amd.stationary.tables (the tables the device reads too), equilibrium_mirror's plan (the noise-free rewards) and
deviation_mirror's encode / scale / env_step.  iterate() is the recurrence itself, vectorised over games, with an
explicit ascending loop over the source cells j so that every sum has the stated order and every operation is rounded
once; solve() finds the same limit without iterating: the closed classes of the transition graph, the absorption
probabilities from mu_0 and the per-class stationary vectors with numpy.linalg.solve.
"""
import numpy as np

import attractors_mirror as A
import deviation_mirror as M
import equilibrium_mirror as E


def cell_tuples(config, policy, tabs, G):
    """t_g(k) [G, J]: the tuple of the (clamped) policy entries at the cells' rows."""
    pl = E.plan(config)
    roff = np.concatenate([[0], np.cumsum([p["states"] + 1 for p in pl["ag"]])])
    policy = np.asarray(policy).astype(np.int64)[:G]
    t = np.zeros((G, tabs["n_cells"]), np.int64)
    for i in range(pl["N"]):
        rows = np.clip(np.asarray(tabs["cell_rows"][i], np.int64), 0, pl["ag"][i]["states"])
        t += np.minimum(policy[:, roff[i] + rows], pl["n_actions"][i] - 1) * pl["tstride"][i]
    return t


def full_band(tabs):
    """n [T, J] from band_lo / band."""
    T, J, W = tabs["n_tuples"], tabs["n_cells"], tabs["band_w"]
    n = np.zeros((T, J))
    for t in range(T):
        for d in range(W):
            k = int(tabs["band_lo"][t]) + d
            if 0 <= k < J:
                n[t, k] = tabs["band"][t, d]
    return n


def chain(tabs, tup, p):
    """P [J, J] of one game: tup [J], p its noise probability."""
    n = full_band(tabs)
    J = tabs["n_cells"]
    q = 1.0 - p
    P = p * n[tup]
    det = np.asarray(tabs["det_cell"])[tup]
    for j in range(J):
        if 0 <= det[j] < J:
            P[j, det[j]] = q + P[j, det[j]]
    return P


def start_cells(config, tabs, state0):
    """The cell whose row tuple is (encode64_i(state0))_i per game, -1 where there is none."""
    ag, _, _ = M.params(config)
    rows = np.stack([M.encode(np.asarray(state0, np.float64), p) for p in ag])         # [N, G]
    cell_of = {tuple(int(v) for v in tabs["cell_rows"][:, k]): k for k in range(tabs["n_cells"])}
    return np.array([cell_of.get(tuple(int(v) for v in rows[:, g]), -1) for g in range(rows.shape[1])], np.int64)


def values(config, tabs, tup, p):
    """Per game and cell the terms of the outputs: reward [N, G, J], action [N, G, J], price [G, J]."""
    pl = E.plan(config)
    _, a, b = M.params(config)
    idx = np.unravel_index(np.arange(pl["T"]), pl["n_actions"])
    sc = [M.scale(idx[i], pl["ag"][i]) for i in range(pl["N"])]
    price, _ = M.env_step(sc, a, b)
    q = (1.0 - p)[:, None]
    pp = p[:, None]
    rew = np.stack([q * pl["rew"][i][tup] + pp * tabs["noise_reward"][i][tup] for i in range(pl["N"])])
    act = np.stack([sc[i][tup] for i in range(pl["N"])])
    return rew, act, q * price[tup] + pp * tabs["noise_price"][tup]


def ordered_sum(x):
    """Sum over the last axis in ascending order from 0.0."""
    s = np.zeros(x.shape[:-1])
    for k in range(x.shape[-1]):
        s = s + x[..., k]
    return s


def outputs(config, tabs, tup, p, mu):
    rew, act, price = values(config, tabs, tup, p)
    return dict(mass=ordered_sum(mu), stat_reward=ordered_sum(mu[None] * rew), stat_action=ordered_sum(mu[None] * act),
                stat_price=ordered_sum(mu * price))


def iterate(config, tabs, policy, noise_prob, state0=None, tol=1e-12, max_iters=8192, n_games=None):
    """Every output of thrl_stationary (pi included).  policy [G, P]; noise_prob a number or [G]; state0 [G] = the
    start THRL_STAT_START_STATE, None = the reset distribution."""
    G = np.asarray(policy).shape[0] if n_games is None else int(n_games)
    J, N = tabs["n_cells"], tabs["cell_rows"].shape[0]
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    ok = (p > 0.0) & (p <= 1.0)
    tup = cell_tuples(config, policy, tabs, G)
    if state0 is None:
        mu = np.tile(np.asarray(tabs["cell_w"], np.float64), (G, 1))
    else:
        k0 = start_cells(config, tabs, np.asarray(state0, np.float64)[:G])
        ok &= k0 >= 0
        mu = np.zeros((G, J))
        mu[np.arange(G), np.maximum(k0, 0)] = 1.0
    pz = np.where(ok, p, 0.5)
    q = 1.0 - pz
    n = full_band(tabs)
    det = np.asarray(tabs["det_cell"], np.int64)[tup]                     # [G, J]
    cells = np.arange(J)[None, :]
    iters, change = np.zeros(G, np.int64), np.zeros(G)
    act = np.flatnonzero(ok)

    def row(gs, j):                                                       # P_g(j, .) of the games gs: [len(gs), J]
        Pj = pz[gs, None] * n[tup[gs, j]]
        return np.where(det[gs, j][:, None] == cells, q[gs, None] + Pj, Pj)

    # the rows do not change from step to step: kept, source-major, when they fit (the same values either way)
    Pt = np.stack([row(np.arange(G), j) for j in range(J)]) if G * J * J <= 30_000_000 else None
    while act.size:
        m = mu[act]
        s = np.zeros_like(m)
        for j in range(J):
            s = s + m[:, j:j + 1] * (Pt[j][act] if Pt is not None else row(act, j))
        new = 0.5 * m + 0.5 * s
        chg = np.abs(new - m).max(axis=1)
        mu[act] = new
        iters[act] += 1
        change[act] = chg
        act = act[~((chg <= tol) | (iters[act] >= max_iters))]
    out = outputs(config, tabs, tup, pz, mu)
    out.update(iters=iters.astype(np.int32), change=change, pi=mu)
    bad = ~ok
    out["iters"][bad] = -1
    for f in ("change", "mass", "stat_price"):
        out[f][bad] = 0.0
    out["pi"][bad] = 0.0
    out["stat_reward"][:, bad] = 0.0
    out["stat_action"][:, bad] = 0.0
    return out


# ---------------------------------------------------------------------------------------------- the direct solve
def closed_classes(P):
    """The closed communicating classes of the chain P [J, J] as a list of index arrays, and the transient states."""
    J = P.shape[0]
    R = (P > 0.0) | np.eye(J, dtype=bool)
    while True:
        R2 = (R.astype(np.int64) @ R.astype(np.int64)) > 0
        if (R2 == R).all():
            break
        R = R2
    same = R & R.T
    classes, seen = [], np.zeros(J, bool)
    for s in range(J):
        if seen[s]:
            continue
        members = np.flatnonzero(same[s])
        seen[members] = True
        if not (R[s] & ~same[s]).any():           # nothing outside the class is reachable
            classes.append(members)
    closed = np.zeros(J, bool)
    for c in classes:
        closed[c] = True
    return classes, np.flatnonzero(~closed)


def limit(P, mu0):
    """The Cesaro limit of mu0 P^m: sum over the closed classes of (the mass that ends in the class) x (its stationary
    vector)."""
    J = P.shape[0]
    classes, trans = closed_classes(P)
    out = np.zeros(J)
    if trans.size:
        Nf = np.linalg.solve(np.eye(trans.size) - P[np.ix_(trans, trans)].T, mu0[trans])      # expected visits
    for c in classes:
        m = mu0[c].sum()
        if trans.size:
            m += Nf @ P[np.ix_(trans, c)].sum(axis=1)
        Pc = P[np.ix_(c, c)]
        Amat = np.vstack([(Pc.T - np.eye(c.size))[:-1], np.ones(c.size)])
        rhs = np.zeros(c.size)
        rhs[-1] = 1.0
        out[c] = m * np.linalg.solve(Amat, rhs)
    return out, len(classes)


def solve(config, tabs, policy, noise_prob, state0=None, n_games=None):
    """pi [G, J], the outputs built from it, and the number of closed classes per game, without iterating."""
    G = np.asarray(policy).shape[0] if n_games is None else int(n_games)
    p = np.broadcast_to(np.asarray(noise_prob, np.float64), (G,)).copy()
    tup = cell_tuples(config, policy, tabs, G)
    J = tabs["n_cells"]
    pi, ncls = np.zeros((G, J)), np.zeros(G, np.int64)
    k0 = None if state0 is None else start_cells(config, tabs, np.asarray(state0, np.float64)[:G])
    for g in range(G):
        mu0 = np.asarray(tabs["cell_w"], np.float64) if k0 is None else np.eye(J)[k0[g]]
        pi[g], ncls[g] = limit(chain(tabs, tup[g], p[g]), mu0)
    out = outputs(config, tabs, tup, p, pi)
    out.update(pi=pi, classes=ncls)
    return out


def fresh_tables(config, G, seed):
    """[G, stride] float64 tables shaped like fresh ones: 12.5 / (1 - gamma) + randn."""
    ag, _, _ = M.params(config)
    rs = np.random.RandomState(seed)
    return np.concatenate([12.5 / (1.0 - p["gamma"]) + rs.randn(G, (p["states"] + 1) * p["actions"]) for p in ag], axis=1)


policies = A.policies
