"""numpy restatement of thrl_sampled_noise_chain (include/thrl.h) from given probability rows and policies at the
distinct prices and at the quadrature nodes and the per-config tables of th_rl_amd.sampled_play.noise_tables, written
from the definitions: every sum runs in the stated order (a loop over d and over j with vector operations over t' and
over the games), every operation is one numpy float64 operation.  The noise-free half (rows, M / W, the start, the
configs and the random networks) is tests/sampled_mirror.py's."""
import numpy as np

import sampled_mirror as SPM
from sampled_mirror import _ordered_sum

RESET = "reset"


def node_tabs(tabs):
    """`tabs` as sampled_mirror.rows_of reads it, over the nodes in place of the distinct prices."""
    return dict(tabs, n_prices=int(tabs["n_nodes"]))


def max_jump(tabs, nprobs, n_games):
    """[G]: the largest |Pn_i(k|j + 1) - Pn_i(k|j)| over the networks, the nodes 1 <= j < Jn - 1 and the actions."""
    out = np.zeros(n_games)
    for p in nprobs.values():
        p = np.asarray(p, np.float32).astype(np.float64)[:n_games]
        if p.shape[1] > 2:
            out = np.fmax(out, np.abs(p[:, 2:, :] - p[:, 1:-1, :]).max(axis=(1, 2)))
    return out


def node_mass(tabs, m):
    """nu [G, Jn] = sum_t m(t) nn(t, j), added in ascending t from 0.0 (a zero term changes nothing)."""
    nn = np.asarray(tabs["nn"], np.float64)
    nu = np.zeros((m.shape[0], nn.shape[1]))
    for t in range(nn.shape[0]):
        nu = nu + m[:, t:t + 1] * nn[t][None, :]
    return nu


def product_sum(V, P, act, skip=None):
    """[G, T]: sum_x ((V(x) * P_0(a_0(t')|x)) * P_1(a_1(t')|x)) * ... in ascending x from 0.0; an x with V(x) == 0.0 (or
    with skip[x]) is left out."""
    s = np.zeros((V.shape[0], act.shape[1]))
    for x in range(V.shape[1]):
        v = V[:, x]
        live = v != 0.0
        if skip is not None and skip[x]:
            continue
        if not live.any():
            continue
        term = v[:, None]
        for i, p in enumerate(P):
            term = term * p[:, x, :][:, act[i]]
        new = s + term
        s = new if live.all() else np.where(live[:, None], new, s)
    return s


def step(tabs, P, Z, Pn, Zn, act, m, p, q):
    """(m', chg [G]) for the iterates m [G, T] and the games' noise probabilities p, q = 1 - p [G]."""
    W = SPM.weights(tabs, Z, m)
    V = node_mass(tabs, m) / Zn
    sd = product_sum(W, P, act)
    sn = product_sum(V, Pn, act)
    s = q[:, None] * sd + p[:, None] * sn
    new = 0.5 * m + 0.5 * s
    return new, np.fmax.reduce(np.abs(new - m), axis=1, initial=0.0)


def reset_start(tabs, Pn, Zn, act):
    """m_0 [G, T] of THRL_SPN_START_RESET."""
    w = np.asarray(tabs["node_w"], np.float64)
    return product_sum(w[None, :] / Zn, Pn, act, skip=w == 0.0)


def analyse(tabs, probs, dpolicy, nprobs, npolicy, eps, noise_prob, start=None, tol=1e-12, max_iters=8192):
    """Every output of thrl_sampled_noise_chain.  probs {i: float32 [G, D, A_i]}, dpolicy uint16 [G, N, D], nprobs
    {i: float32 [G, Jn, A_i]}, npolicy uint16 [G, N, Jn], eps [N] numbers or [N, G], noise_prob a number or [G]; start
    None (uniform), RESET or int [G]."""
    dpolicy, npolicy = np.asarray(dpolicy), np.asarray(npolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T = int(tabs["n_tuples"])
    eps = np.asarray(eps, np.float64)
    eps = np.repeat(eps[:, None], G, axis=1) if eps.ndim == 1 else eps[:, :G]
    pr = np.asarray(noise_prob, np.float64) * np.ones(G)
    ok = (pr >= 0.0) & (pr <= 1.0)
    for i, kind in enumerate(tabs["kinds"]):
        if kind == "QTable":
            ok &= (eps[i] >= 0.0) & (eps[i] <= 1.0)
    reset = isinstance(start, str)
    if start is not None and not reset:
        start = np.asarray(start, np.int64).reshape(-1)[:G]
        ok &= (start >= 0) & (start < T)
    out = {"iters": np.full(G, -1, np.int32), "change": np.zeros(G), "mass": np.zeros(G), "samp_price": np.zeros(G),
           "agree": np.zeros(G), "samp_reward": np.zeros((N, G)), "samp_action": np.zeros((N, G)), "pi": np.zeros((G, T)),
           "max_jump": max_jump(tabs, nprobs, G)}
    idx = np.flatnonzero(ok)
    if not idx.size:
        return out
    e = np.where(ok[None, :], eps, 0.0)[:, idx]
    P, Z, greedy = SPM.rows_of(tabs, {i: np.asarray(x)[idx] for i, x in probs.items()}, dpolicy[idx], e)
    Pn, Zn, ngreedy = SPM.rows_of(node_tabs(tabs), {i: np.asarray(x)[idx] for i, x in nprobs.items()}, npolicy[idx], e)
    act = SPM.actions_of(tabs)
    p = pr[idx]
    q = 1.0 - p
    if reset:
        m = reset_start(tabs, Pn, Zn, act)
    elif start is None:
        m = np.full((idx.size, T), 1.0 / float(T))
    else:
        m = np.zeros((idx.size, T))
        m[np.arange(idx.size), start[idx]] = 1.0
    iters = np.zeros(idx.size, np.int32)
    change = np.zeros(idx.size)
    live = np.arange(idx.size)
    while live.size:
        new, chg = step(tabs, [x[live] for x in P], Z[live], [x[live] for x in Pn], Zn[live], act, m[live], p[live], q[live])
        m[live] = new
        iters[live] += 1
        change[live] = chg
        live = live[~((chg <= tol) | (iters[live] >= max_iters))]
    term = SPM.weights(tabs, Z, m)
    for i, x in enumerate(P):
        term = term * np.take_along_axis(x, greedy[:, i, :, None], axis=2)[:, :, 0]
    nterm = node_mass(tabs, m) / Zn
    for i, x in enumerate(Pn):
        nterm = nterm * np.take_along_axis(x, ngreedy[:, i, :, None], axis=2)[:, :, 0]
    out["iters"][idx], out["change"][idx], out["pi"][idx] = iters, change, m
    out["mass"][idx] = _ordered_sum(m)
    out["agree"][idx] = q * _ordered_sum(term) + p * _ordered_sum(nterm)
    price, nprice = np.asarray(tabs["price"])[None, :], np.asarray(tabs["noise_price"])[None, :]
    out["samp_price"][idx] = _ordered_sum(m * (q[:, None] * price + p[:, None] * nprice))
    for i in range(N):
        r, nr = np.asarray(tabs["reward"])[i][None, :], np.asarray(tabs["noise_reward"])[i][None, :]
        out["samp_reward"][i, idx] = _ordered_sum(m * (q[:, None] * r + p[:, None] * nr))
        out["samp_action"][i, idx] = _ordered_sum(m * np.asarray(tabs["scaled"])[i][None, :])
    return out


# ------------------------------------------------------------------------------------------------ shared inputs
AG, RF, ENV = SPM.AG, SPM.RF, SPM.ENV
ATOM, NO_ATOM = [0.2, 0.4], [0.0, 0.3]                  # action ranges: some redrawn prices clip to 0 / none does


def two_agents(kind0, a0, kind1, a1, action_range=ATOM):
    mk = lambda kind, n: dict(AG if kind == "QTable" else dict(RF, name=kind), actions=n, action_range=list(action_range))
    return {"agents": [mk(kind0, a0), mk(kind1, a1)], "environment": dict(ENV)}


def three_agents(action_range=ATOM):
    """Reinforce 2 x QTable 3 x ActorCritic 2: T = 12, the kernel's variant for more than two agents."""
    ag = [dict(RF, actions=2), dict(AG, actions=3, states=30), dict(RF, name="ActorCritic", actions=2)]
    return {"agents": [dict(x, action_range=list(action_range)) for x in ag], "environment": dict(ENV, nplayers=3, max_steps=40)}


def make_inputs(config, resolution, n_games, seed):
    """dict(tabs, probs, dpolicy, nprobs, npolicy, eps [N, G], noise_prob [G], start [G]): random networks (peaked in three
    games of four) evaluated by numpy at the distinct prices and at the nodes, random QTable strategies with entries at or
    above the action count mixed in, epsilon in [0, 0.2], noise_prob in [0, 0.5]."""
    from th_rl_amd import sampled_play as sp
    tabs = sp.noise_tables(config, resolution)
    rs = np.random.RandomState(seed)
    N, T = len(tabs["kinds"]), int(tabs["n_tuples"])
    probs, nprobs = {}, {}
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            A = int(tabs["n_actions"][i])
            w = SPM.random_weights(rs, n_games, A, k, 0.0, float(tabs["price"].max()))
            probs[i], nprobs[i] = SPM.net_probs(w, A, tabs["dprice"]), SPM.net_probs(w, A, tabs["xn"])
    pol = SPM.greedy_of(probs, tabs, rs, n_games)
    npol = SPM.greedy_of(nprobs, node_tabs(tabs), rs, n_games)
    return dict(tabs=tabs, probs=probs, dpolicy=pol, nprobs=nprobs, npolicy=npol, eps=rs.uniform(0.0, 0.2, (N, n_games)),
                noise_prob=rs.uniform(0.0, 0.5, n_games), start=rs.randint(0, T, n_games).astype(np.int32))
