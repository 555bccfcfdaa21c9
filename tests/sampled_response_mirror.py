"""numpy restatement of thrl_sampled_response (include/thrl_response.h) from given probability rows, dpolicy and the
per-config tables of th_rl_amd.sampled_play.tables, written from the definitions: every sum runs in the stated order
(np.add.accumulate from 0.0 along the summed axis), every operation is one numpy float64 operation.  One (agent, game) at
a time, vectorised over the prices and actions.  The configs, weights and row generators are tests/sampled_mirror.py's.
Also dense(): an independent dense solution (numpy.linalg.solve and value iteration on normalised probabilities) that the
host test holds the mirror against, and write_case(): the binary case files of tests/sampled_response_check.cpp."""
import numpy as np

import sampled_mirror as SPM

EQ_MAX_ITERS = 64


def _gamma_of(gamma, N, G):
    g = np.asarray(gamma, np.float64)
    if g.ndim == 0:
        g = np.full(N, float(g))
    return np.repeat(g[:, None], G, axis=1) if g.ndim == 1 else g[:, :G]


def _eps_of(eps, N, G):
    e = np.asarray(eps, np.float64)
    if e.ndim == 0:
        e = np.full(N, float(e))
    return np.repeat(e[:, None], G, axis=1) if e.ndim == 1 else e[:, :G]


def agent_tables(tabs, P, i):
    """For one game's rows P (list of float64 [D, A_j]) and agent i: S [N, D]; w [D, T] (the product over j != i in
    ascending j, the first factor as is); Zm [D]; idx int [A_i, T / A_i], the tuples in which agent i plays k, ascending."""
    act = SPM.actions_of(tabs)
    N, T = act.shape
    D = P[0].shape[0]
    S = np.stack([np.ones(D) if k == "QTable" else SPM._ordered_sum(p) for k, p in zip(tabs["kinds"], P)])
    w = zm = None
    for j in range(N):
        if j == i:
            continue
        f = P[j][:, act[j]]
        w = f if w is None else w * f
        zm = S[j] if zm is None else zm * S[j]
    if w is None:
        w, zm = np.ones((D, T)), np.ones(D)
    A = int(tabs["n_actions"][i])
    idx = np.stack([np.flatnonzero(act[i] == k) for k in range(A)])
    return S, w, zm, idx


def q_values(w, zm, idx, U):
    """Q_V [D, A_i] from U [T]."""
    terms = w[:, idx] * U[idx][None, :, :]
    return SPM._ordered_sum(terms) / zm[:, None]


def solve_one(tabs, P, greedy_i, i, gam, eval_tol, max_sweeps):
    """One (agent, game): dict(iters, sweeps, sigma, modal, V, Vpi, S_i, P_i) -- V and Vpi None when not solved."""
    kinds = tabs["kinds"]
    row = np.asarray(tabs["row"], np.int64)
    R = np.asarray(tabs["reward"], np.float64)[i]
    D = P[0].shape[0]
    S, w, zm, idx = agent_tables(tabs, P, i)
    Pi, Si = P[i], S[i]
    modal = np.asarray(greedy_i, np.int64) if kinds[i] == "QTable" else Pi.argmax(axis=1)
    out = dict(iters=-1, sweeps=0, sigma=modal.copy(), modal=modal, V=None, Vpi=None, S_i=Si, P_i=Pi)
    if not (gam >= 0.0 and gam < 1.0):
        return out
    ar = np.arange(D)

    def evaluate(V, sigma):
        m = 0
        while True:
            U = R + gam * V[row]
            Q = q_values(w, zm, idx, U)
            Vn = SPM._ordered_sum(Pi * Q) / Si if sigma is None else Q[ar, sigma]
            c = np.fmax.reduce(np.abs(Vn - V), initial=0.0)
            V = Vn
            m += 1
            out["sweeps"] += 1
            if c <= eval_tol:
                return V, False
            if m >= max_sweeps:
                return V, True

    V, capped = evaluate(np.zeros(D), None)
    if capped:
        return out
    Vpi = V
    margin = (((2.0 * gam) * gam) * eval_tol) / (1.0 - gam)
    sigma = modal.copy()
    n = 0
    while True:
        V, capped = evaluate(V, sigma)
        if capped or n == EQ_MAX_ITERS:
            return out
        Q = q_values(w, zm, idx, R + gam * V[row])
        ba = Q.argmax(axis=1)
        better = Q[ar, ba] > Q[ar, sigma] + margin
        if not better.any():
            break
        sigma = np.where(better, ba, sigma)
        n += 1
    out.update(iters=n, sigma=sigma, V=V, Vpi=Vpi)
    return out


def rel_loss(vs, vp):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((vs == vp) | (vs == 0.0), 0.0, (vs - vp) / vs)


def analyse(tabs, probs, dpolicy, eps, gamma, agents=None, eval_tol=1e-12, max_sweeps=8192, pi=None):
    """Every output of thrl_sampled_response.  probs {i: float32 [G, D, A_i]}, dpolicy uint16 [G, N, D], eps and gamma a
    number, [N] numbers or [N, G]; agents: the selected ones (default all); pi [G, T] or None.  Entries of agents that are
    not selected stay zero."""
    dpolicy = np.asarray(dpolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    eps, gamma = _eps_of(eps, N, G), _gamma_of(gamma, N, G)
    agents = list(range(N)) if agents is None else list(agents)
    first, perm = np.asarray(tabs["grp_first"]), np.asarray(tabs["grp_perm"])
    ok = np.ones(G, bool)
    for i, kind in enumerate(tabs["kinds"]):
        if kind == "QTable":
            ok &= (eps[i] >= 0.0) & (eps[i] <= 1.0)
    out = {f: np.zeros((N, G), np.int32) for f in ("iters", "sweeps", "n_diff")}
    out.update({f: np.zeros((N, G)) for f in ("loss_all", "loss_mean", "loss_w", "gain_w", "v_w", "br_prob_w")})
    out.update(br_policy=np.zeros((N, G, D), np.uint16), v_opt=np.zeros((N, G, D)), v_pi=np.zeros((N, G, D)))
    weighted = ("loss_w", "gain_w", "v_w", "br_prob_w")
    for g in range(G):
        if not ok[g]:
            out["iters"][agents, g] = -1
            continue
        sub = {i: np.asarray(p)[g:g + 1] for i, p in probs.items()}
        P, _, greedy = SPM.rows_of(tabs, sub, dpolicy[g:g + 1], eps[:, g:g + 1])
        P = [p[0] for p in P]
        for i in agents:
            r = solve_one(tabs, P, greedy[0, i], i, float(gamma[i, g]), eval_tol, max_sweeps)
            out["iters"][i, g], out["sweeps"][i, g] = r["iters"], r["sweeps"]
            if r["iters"] < 0:
                for f in ("loss_all", "loss_mean") + (weighted if pi is not None else ()):
                    out[f][i, g] = np.nan
                out["br_policy"][i, g] = r["modal"]
                out["v_opt"][i, g] = out["v_pi"][i, g] = np.nan
                continue
            V, Vpi, sigma = r["V"], r["Vpi"], r["sigma"]
            loss = rel_loss(V, Vpi)
            out["n_diff"][i, g] = int((sigma != r["modal"]).sum())
            out["loss_all"][i, g] = loss.max()
            out["loss_mean"][i, g] = SPM._ordered_sum(loss) / float(D)
            out["br_policy"][i, g], out["v_opt"][i, g], out["v_pi"][i, g] = sigma, V, Vpi
            if pi is not None:
                M = np.zeros(D)
                for d in range(D):
                    M[d] = SPM._ordered_sum(np.asarray(pi, np.float64)[g, perm[first[d]:first[d + 1]]])
                out["loss_w"][i, g] = SPM._ordered_sum(M * loss)
                out["gain_w"][i, g] = SPM._ordered_sum(M * (V - Vpi))
                out["v_w"][i, g] = SPM._ordered_sum(M * Vpi)
                out["br_prob_w"][i, g] = SPM._ordered_sum((M * r["P_i"][np.arange(D), sigma]) / r["S_i"])
    return out


# ------------------------------------------------------------------------------------------------ an independent solution
def dense(tabs, P, i, gam, vi_tol=0.0, vi_max=200000):
    """(V_pi [D], V* [D]) of agent i for one game's rows P, from NORMALISED probabilities and a dense D x D chain:
    V_pi by numpy.linalg.solve, V* by value iteration to a fixed point (no change at all, or below vi_tol).  Shares no
    code with solve_one but the action digits."""
    act = SPM.actions_of(tabs)
    N, T = act.shape
    D = P[0].shape[0]
    row = np.asarray(tabs["row"], np.int64)
    R = np.asarray(tabs["reward"], np.float64)[i]
    A = int(tabs["n_actions"][i])
    norm = [p / p.sum(axis=1, keepdims=True) for p in P]
    rival = np.ones((D, T))
    for j in range(N):
        if j != i:
            rival = rival * norm[j][:, act[j]]
    onehot = np.zeros((T, D))
    onehot[np.arange(T), row] = 1.0
    # per action k: the transition matrix and the expected reward when agent i plays k at every price
    Pk = np.zeros((A, D, D))
    rk = np.zeros((A, D))
    for k in range(A):
        m = (act[i] == k).astype(np.float64)
        Pk[k] = (rival * m[None, :]) @ onehot
        rk[k] = (rival * m[None, :]) @ R
    own = norm[i]                                                   # [D, A]
    Ppi = np.einsum("dk,kde->de", own, Pk)
    rpi = np.einsum("dk,kd->d", own, rk)
    Vpi = np.linalg.solve(np.eye(D) - gam * Ppi, rpi)
    V = Vpi.copy()
    for _ in range(vi_max):
        Vn = (rk + gam * (Pk @ V)).max(axis=0)
        done = np.abs(Vn - V).max() <= vi_tol
        V = Vn
        if done:
            break
    return Vpi, V


# ------------------------------------------------------------------------------------------------ case files
KIND = {"QTable": 0, "Reinforce": 1, "ActorCritic": 2}


def write_case(path, tabs, probs, dpolicy, eps, gamma, agents, eval_tol, max_sweeps, pi, ref, n_blocks):
    """The inputs and the expected outputs `ref` (analyse's) as tests/sampled_response_check.cpp reads them."""
    dpolicy = np.asarray(dpolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    eps, gamma = np.asarray(eps, np.float64), np.asarray(gamma, np.float64)
    kind, nact = np.zeros(8, np.int32), np.zeros(8, np.int32)
    kind[:N] = [KIND[k] for k in tabs["kinds"]]
    nact[:N] = tabs["n_actions"]
    e8, g8 = np.zeros(8), np.zeros(8)
    if eps.ndim < 2:
        e8[:N] = eps
    if gamma.ndim < 2:
        g8[:N] = gamma
    mask = sum(1 << i for i in agents)
    with open(path, "wb") as f:
        np.array([G, N, T, D, mask, max_sweeps, int(eps.ndim == 2), int(gamma.ndim == 2), int(pi is not None), n_blocks],
                 np.int32).tofile(f)
        kind.tofile(f), nact.tofile(f), e8.tofile(f), g8.tofile(f), np.array([eval_tol]).tofile(f)
        if eps.ndim == 2:
            np.ascontiguousarray(eps[:, :G]).tofile(f)
        if gamma.ndim == 2:
            np.ascontiguousarray(gamma[:, :G]).tofile(f)
        for i in range(N):
            if i in probs:
                np.ascontiguousarray(probs[i], np.float32).tofile(f)
        np.ascontiguousarray(dpolicy, np.uint16).tofile(f)
        for name, dt in (("grp_first", np.int32), ("grp_perm", np.int32), ("reward", np.float64)):
            np.ascontiguousarray(tabs[name], dt).tofile(f)
        if pi is not None:
            np.ascontiguousarray(pi, np.float64).tofile(f)
        for name in ("iters", "sweeps", "n_diff"):
            np.ascontiguousarray(ref[name], np.int32).tofile(f)
        for name in ("loss_all", "loss_mean", "loss_w", "gain_w", "v_w", "br_prob_w"):
            np.ascontiguousarray(ref[name], np.float64).tofile(f)
        np.ascontiguousarray(ref["br_policy"], np.uint16).tofile(f)
        np.ascontiguousarray(ref["v_opt"], np.float64).tofile(f)
        np.ascontiguousarray(ref["v_pi"], np.float64).tofile(f)


# ------------------------------------------------------------------------------------------------ shared inputs
def make_inputs(config, n_games, seed):
    """(tabs, probs, dpolicy, eps [N, G], pi [G, T]) for a config: sampled_mirror's random networks and strategies, the
    networks' entries of dpolicy their rows' first maxima, epsilon in [0, 0.2], pi a random distribution per game."""
    from th_rl_amd import sampled_play as sp
    tabs = sp.tables(config)
    rs = np.random.RandomState(seed)
    N, T = len(tabs["kinds"]), int(tabs["n_tuples"])
    probs = {}
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            w = SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, tabs["price"].min(), tabs["price"].max())
            probs[i] = SPM.net_probs(w, int(tabs["n_actions"][i]), tabs["dprice"])
    pol = SPM.greedy_of(probs, tabs, rs, n_games)
    eps = rs.uniform(0, 0.2, (N, n_games))
    pi = rs.dirichlet(np.ones(T), n_games)
    return tabs, probs, pol, eps, pi


def own_gammas(config):
    return [float(a["gamma"]) for a in config["agents"]]


def host_cases():
    """The cases of the stand-alone host program: (what, dict of analyse()'s arguments, blocks).  QQ with per-game epsilon
    and gamma and an unsolved game of each kind (a bad epsilon, a gamma of 1.0, an agent capped by max_sweeps = 3 in
    another case), QRA on a subset of agents, RR (D < T, a team per price), SHIP at gamma 0.5 (D > 256)."""
    out = []
    tabs, probs, pol, eps, pi = make_inputs(SPM.QQ, 6, 11)
    gam = np.repeat(np.array([0.6, 0.5])[:, None], 6, axis=1)
    eps[0, 1] = np.nan
    gam[1, 2] = 1.0
    gam[0, 4] = -0.5
    out.append(("QQ per-game epsilon and gamma, a bad epsilon, gammas outside [0, 1)",
                dict(tabs=tabs, probs=probs, dpolicy=pol, eps=eps, gamma=gam, agents=[0, 1], eval_tol=1e-12, max_sweeps=8192, pi=pi), 2))
    tabs, probs, pol, eps, pi = make_inputs(SPM.QQ, 3, 12)
    out.append(("QQ capped by max_sweeps = 3",
                dict(tabs=tabs, probs=probs, dpolicy=pol, eps=eps[:, 0].copy(), gamma=0.9, agents=[1], eval_tol=1e-12, max_sweeps=3,
                     pi=None), 1))
    tabs, probs, pol, eps, pi = make_inputs(SPM.QRA, 3, 13)
    out.append(("QRA agents 0 and 2", dict(tabs=tabs, probs=probs, dpolicy=pol, eps=eps, gamma=[0.6, 0.5, 0.4], agents=[0, 2],
                                             eval_tol=1e-12, max_sweeps=8192, pi=pi), 2))
    tabs, probs, pol, eps, pi = make_inputs(SPM.RR, 2, 14)
    out.append(("RR D < T", dict(tabs=tabs, probs=probs, dpolicy=pol, eps=eps[:, 0].copy(), gamma=0.5, agents=[0, 1],
                                 eval_tol=1e-12, max_sweeps=8192, pi=pi), 1))
    tabs, probs, pol, eps, pi = make_inputs(SPM.SHIP, 2, 15)
    out.append(("SHIP gamma 0.5", dict(tabs=tabs, probs=probs, dpolicy=pol, eps=eps, gamma=0.5, agents=[0, 1], eval_tol=1e-12,
                                       max_sweeps=8192, pi=pi), 2))
    return out
