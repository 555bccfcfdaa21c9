"""numpy restatement of thrl_sampled_response_noise (include/thrl_response_noise.h) from given probability rows and
policies at the distinct prices and at the quadrature nodes and the per-config tables of
th_rl_amd.sampled_play.noise_tables, written from the definitions: every sum runs in the stated order (np.add.accumulate
from 0.0 along the summed axis), every operation is one numpy float64 operation.  One (agent, game) at a time, vectorised
over the S = D + Jn states and the actions.  The configs and row generators are tests/sampled_mirror.py's and
tests/sampled_noise_mirror.py's, the tables of one agent and Q_V tests/sampled_response_mirror.py's (over the states in
place of the prices).  Also dense(): an independent dense solution on the S x S chain that the host test holds the mirror
against, and write_case(): the binary case files of tests/sampled_response_noise_check.cpp."""
import numpy as np

import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import sampled_response_mirror as SRM

EQ_MAX_ITERS = SRM.EQ_MAX_ITERS
INT = ("iters", "sweeps", "n_diff_prices", "n_diff_nodes")
FLOAT = ("loss_all", "loss_prices_mean", "loss_nodes_mean")
WEIGHTED = ("loss_w", "gain_w", "v_w", "br_prob_w")


def _per_game(x, G):
    return np.asarray(x, np.float64) * np.ones(G)


def band_terms(tabs):
    """(node int [T, W] clipped into [0, Jn), valid bool [T, W], band [T, W]): nn(t, .) as the kernel walks it."""
    lo, band = np.asarray(tabs["band_lo"], np.int64), np.asarray(tabs["band"], np.float64)
    Jn = int(tabs["n_nodes"])
    node = lo[:, None] + np.arange(band.shape[1])[None, :]
    valid = (node >= 0) & (node < Jn)
    return np.clip(node, 0, Jn - 1), valid, band


def u_of(tabs, bt, Rn, V, gam, p, q):
    """U_V [T].  A skipped node enters the ordered sum as +0.0, which changes no partial sum that started from 0.0."""
    D = int(tabs["n_prices"])
    node, valid, band = bt
    b = SPM._ordered_sum(np.where(valid, band * V[D:][node], 0.0))
    z = q * V[:D][np.asarray(tabs["row"], np.int64)] + p * b
    return Rn + gam * z


def solve_one(tabs, PS, greedy_i, i, gam, p, eval_tol, max_sweeps, bt=None):
    """One (agent, game).  PS: list of float64 [S, A_j], the rows at the prices, then at the nodes; greedy_i int [S].
    dict(iters, sweeps, sigma, modal, V, Vpi, S_i, P_i) -- V and Vpi None when not solved."""
    kinds = tabs["kinds"]
    bt = band_terms(tabs) if bt is None else bt
    q = 1.0 - p
    Rn = q * np.asarray(tabs["reward"], np.float64)[i] + p * np.asarray(tabs["noise_reward"], np.float64)[i]
    S = PS[0].shape[0]
    Ssum, w, zm, idx = SRM.agent_tables(tabs, PS, i)
    Pi, Si = PS[i], Ssum[i]
    modal = np.asarray(greedy_i, np.int64) if kinds[i] == "QTable" else Pi.argmax(axis=1)
    out = dict(iters=-1, sweeps=0, sigma=modal.copy(), modal=modal, V=None, Vpi=None, S_i=Si, P_i=Pi)
    if not (gam >= 0.0 and gam < 1.0):
        return out
    ar = np.arange(S)

    def evaluate(V, sigma):
        m = 0
        while True:
            Q = SRM.q_values(w, zm, idx, u_of(tabs, bt, Rn, V, gam, p, q))
            Vn = SPM._ordered_sum(Pi * Q) / Si if sigma is None else Q[ar, sigma]
            c = np.fmax.reduce(np.abs(Vn - V), initial=0.0)
            V = Vn
            m += 1
            out["sweeps"] += 1
            if c <= eval_tol:
                return V, False
            if m >= max_sweeps:
                return V, True

    V, capped = evaluate(np.zeros(S), None)
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
        Q = SRM.q_values(w, zm, idx, u_of(tabs, bt, Rn, V, gam, p, q))
        ba = Q.argmax(axis=1)
        better = Q[ar, ba] > Q[ar, sigma] + margin
        if not better.any():
            break
        sigma = np.where(better, ba, sigma)
        n += 1
    out.update(iters=n, sigma=sigma, V=V, Vpi=Vpi)
    return out


def state_rows(tabs, probs, dpolicy, nprobs, npolicy, eps, g):
    """(PS: list of float64 [S, A_j], greedy int [N, S]) of game g: the rows at the prices, then at the nodes."""
    e = eps[:, g:g + 1]
    P, _, gr = SPM.rows_of(tabs, {i: np.asarray(x)[g:g + 1] for i, x in probs.items()}, dpolicy[g:g + 1], e)
    Pn, _, ngr = SPM.rows_of(SNM.node_tabs(tabs), {i: np.asarray(x)[g:g + 1] for i, x in nprobs.items()}, npolicy[g:g + 1], e)
    return [np.concatenate([a[0], b[0]]) for a, b in zip(P, Pn)], np.concatenate([gr[0], ngr[0]], axis=1)


def weights(tabs, pi_g, p):
    """w [S]: q M(d) over the prices, then p nu(j) over the nodes."""
    first, perm = np.asarray(tabs["grp_first"]), np.asarray(tabs["grp_perm"])
    D = int(tabs["n_prices"])
    pi_g = np.asarray(pi_g, np.float64)
    M = np.array([SPM._ordered_sum(pi_g[perm[first[d]:first[d + 1]]]) for d in range(D)])
    nu = SNM.node_mass(tabs, pi_g[None, :])[0]
    return np.concatenate([(1.0 - p) * M, p * nu])


def analyse(tabs, probs, dpolicy, nprobs, npolicy, eps, gamma, noise_prob, agents=None, eval_tol=1e-12, max_sweeps=8192,
            pi=None):
    """Every output of thrl_sampled_response_noise.  probs {i: float32 [G, D, A_i]}, dpolicy uint16 [G, N, D], nprobs
    {i: float32 [G, Jn, A_i]}, npolicy uint16 [G, N, Jn], eps and gamma a number, [N] numbers or [N, G], noise_prob a number
    or [G]; agents: the selected ones (default all); pi [G, T] or None.  Entries of agents that are not selected stay
    zero."""
    dpolicy, npolicy = np.asarray(dpolicy), np.asarray(npolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    D, Jn = int(tabs["n_prices"]), int(tabs["n_nodes"])
    S = D + Jn
    eps, gamma, pr = SRM._eps_of(eps, N, G), SRM._gamma_of(gamma, N, G), _per_game(noise_prob, G)
    agents = list(range(N)) if agents is None else list(agents)
    ok = (pr > 0.0) & (pr <= 1.0)
    for i, kind in enumerate(tabs["kinds"]):
        if kind == "QTable":
            ok &= (eps[i] >= 0.0) & (eps[i] <= 1.0)
    out = {f: np.zeros((N, G), np.int32) for f in INT}
    out.update({f: np.zeros((N, G)) for f in FLOAT + WEIGHTED})
    out.update(br_policy=np.zeros((N, G, S), np.uint16), v_opt=np.zeros((N, G, S)), v_pi=np.zeros((N, G, S)))
    bt = band_terms(tabs)
    for g in range(G):
        if not ok[g]:
            out["iters"][agents, g] = -1
            continue
        p = float(pr[g])
        PS, greedy = state_rows(tabs, probs, dpolicy, nprobs, npolicy, eps, g)
        for i in agents:
            r = solve_one(tabs, PS, greedy[i], i, float(gamma[i, g]), p, eval_tol, max_sweeps, bt)
            out["iters"][i, g], out["sweeps"][i, g] = r["iters"], r["sweeps"]
            if r["iters"] < 0:
                for f in FLOAT + (WEIGHTED if pi is not None else ()):
                    out[f][i, g] = np.nan
                out["br_policy"][i, g] = r["modal"]
                out["v_opt"][i, g] = out["v_pi"][i, g] = np.nan
                continue
            V, Vpi, sigma = r["V"], r["Vpi"], r["sigma"]
            loss = SRM.rel_loss(V, Vpi)
            diff = sigma != r["modal"]
            out["n_diff_prices"][i, g], out["n_diff_nodes"][i, g] = int(diff[:D].sum()), int(diff[D:].sum())
            out["loss_all"][i, g] = loss.max()
            out["loss_prices_mean"][i, g] = SPM._ordered_sum(loss[:D]) / float(D)
            out["loss_nodes_mean"][i, g] = SPM._ordered_sum(loss[D:]) / float(Jn)
            out["br_policy"][i, g], out["v_opt"][i, g], out["v_pi"][i, g] = sigma, V, Vpi
            if pi is not None:
                w = weights(tabs, np.asarray(pi)[g], p)
                out["loss_w"][i, g] = SPM._ordered_sum(w * loss)
                out["gain_w"][i, g] = SPM._ordered_sum(w * (V - Vpi))
                out["v_w"][i, g] = SPM._ordered_sum(w * Vpi)
                out["br_prob_w"][i, g] = SPM._ordered_sum((w * r["P_i"][np.arange(S), sigma]) / r["S_i"])
    return out


# ------------------------------------------------------------------------------------------------ an independent solution
def dense(tabs, PS, i, gam, p, vi_tol=0.0, vi_max=200000):
    """(V_pi [S], V* [S], P_pi [S, S]) of agent i for one game's state rows PS, from NORMALISED probabilities and a dense
    S x S chain: after tuple t the next state is the price row(t) with probability q and node j with probability
    p nn(t, j).  V_pi by numpy.linalg.solve, V* by value iteration to a fixed point.  Shares no code with solve_one but the
    action digits."""
    act = SPM.actions_of(tabs)
    N, T = act.shape
    S = PS[0].shape[0]
    D = int(tabs["n_prices"])
    q = 1.0 - p
    R = q * np.asarray(tabs["reward"], np.float64)[i] + p * np.asarray(tabs["noise_reward"], np.float64)[i]
    A = int(tabs["n_actions"][i])
    norm = [x / x.sum(axis=1, keepdims=True) for x in PS]
    rival = np.ones((S, T))
    for j in range(N):
        if j != i:
            rival = rival * norm[j][:, act[j]]
    nxt = np.zeros((T, S))
    nxt[np.arange(T), np.asarray(tabs["row"], np.int64)] = q
    nxt[:, D:] = p * np.asarray(tabs["nn"], np.float64)
    Pk = np.zeros((A, S, S))
    rk = np.zeros((A, S))
    for k in range(A):
        m = (act[i] == k).astype(np.float64)
        Pk[k] = (rival * m[None, :]) @ nxt
        rk[k] = (rival * m[None, :]) @ R
    own = norm[i]
    Ppi = np.einsum("sk,kse->se", own, Pk)
    rpi = np.einsum("sk,ks->s", own, rk)
    Vpi = np.linalg.solve(np.eye(S) - gam * Ppi, rpi)
    V = Vpi.copy()
    for _ in range(vi_max):
        Vn = (rk + gam * (Pk @ V)).max(axis=0)
        done = np.abs(Vn - V).max() <= vi_tol
        V = Vn
        if done:
            break
    return Vpi, V, Ppi


# ------------------------------------------------------------------------------------------------ case files
def write_case(path, kw, ref, n_blocks):
    """The inputs `kw` (analyse's arguments) and the expected outputs `ref` as tests/sampled_response_noise_check.cpp
    reads them."""
    tabs, probs, nprobs = kw["tabs"], kw["probs"], kw["nprobs"]
    dpolicy, npolicy = np.asarray(kw["dpolicy"]), np.asarray(kw["npolicy"])
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D, Jn, W = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"]), int(tabs["band_w"])
    eps, gamma, pr = np.asarray(kw["eps"], np.float64), np.asarray(kw["gamma"], np.float64), np.asarray(kw["noise_prob"], np.float64)
    pi = kw.get("pi")
    kind, nact = np.zeros(8, np.int32), np.zeros(8, np.int32)
    kind[:N] = [SRM.KIND[k] for k in tabs["kinds"]]
    nact[:N] = tabs["n_actions"]
    e8, g8 = np.zeros(8), np.zeros(8)
    if eps.ndim < 2:
        e8[:N] = eps
    if gamma.ndim < 2:
        g8[:N] = gamma
    mask = sum(1 << i for i in kw["agents"])
    with open(path, "wb") as f:
        np.array([G, N, T, D, Jn, W, mask, kw["max_sweeps"], int(eps.ndim == 2), int(gamma.ndim == 2), int(pr.ndim == 1),
                  int(pi is not None), n_blocks], np.int32).tofile(f)
        kind.tofile(f), nact.tofile(f), e8.tofile(f), g8.tofile(f)
        np.array([kw["eval_tol"], float(pr) if pr.ndim == 0 else 0.0]).tofile(f)
        if eps.ndim == 2:
            np.ascontiguousarray(eps[:, :G]).tofile(f)
        if gamma.ndim == 2:
            np.ascontiguousarray(gamma[:, :G]).tofile(f)
        if pr.ndim == 1:
            np.ascontiguousarray(pr[:G]).tofile(f)
        for i in range(N):
            if i in probs:
                np.ascontiguousarray(probs[i], np.float32).tofile(f)
                np.ascontiguousarray(nprobs[i], np.float32).tofile(f)
        np.ascontiguousarray(dpolicy, np.uint16).tofile(f)
        np.ascontiguousarray(npolicy, np.uint16).tofile(f)
        for name, dt in (("grp_first", np.int32), ("grp_perm", np.int32), ("reward", np.float64), ("band_lo", np.int32),
                         ("band", np.float64), ("noise_reward", np.float64)):
            np.ascontiguousarray(tabs[name], dt).tofile(f)
        if pi is not None:
            np.ascontiguousarray(pi, np.float64).tofile(f)
        for name in INT:
            np.ascontiguousarray(ref[name], np.int32).tofile(f)
        for name in FLOAT + WEIGHTED:
            np.ascontiguousarray(ref[name], np.float64).tofile(f)
        np.ascontiguousarray(ref["br_policy"], np.uint16).tofile(f)
        np.ascontiguousarray(ref["v_opt"], np.float64).tofile(f)
        np.ascontiguousarray(ref["v_pi"], np.float64).tofile(f)


# ------------------------------------------------------------------------------------------------ shared inputs
def make_inputs(config, resolution, n_games, seed):
    """sampled_noise_mirror.make_inputs' dict with analyse()'s keys: noise_prob [G] in (0, 0.5], pi [G, T] a random
    distribution per game, no start."""
    d = SNM.make_inputs(config, resolution, n_games, seed)
    rs = np.random.RandomState(seed + 7000)
    d.pop("start")
    d["noise_prob"] = np.maximum(d["noise_prob"], 0.01)
    d["pi"] = rs.dirichlet(np.ones(int(d["tabs"]["n_tuples"])), n_games)
    return d


def host_cases():
    """The cases of the stand-alone host program: (what, analyse()'s arguments, blocks).  QQ with per-game epsilon, gamma
    and noise and an unsolved game of each kind (a bad epsilon, a bad noise_prob, gammas outside [0, 1); an agent capped by
    max_sweeps = 3 in another case), three agents of mixed kinds on a subset, QR with scalars, RR (D < T) and SHIP at
    resolution 16 and gamma 0.5 (S > 256)."""
    out = []
    kw = make_inputs(SPM.QQ, 8, 7, 21)
    gam = np.repeat(np.array([0.6, 0.5])[:, None], 7, axis=1)
    kw["eps"][0, 1] = np.nan
    kw["noise_prob"][5] = 0.0
    gam[1, 2] = 1.0
    gam[0, 4] = -0.5
    out.append(("QQ per-game epsilon, gamma and noise; a bad epsilon, a bad noise_prob, gammas outside [0, 1)",
                dict(kw, gamma=gam, agents=[0, 1], eval_tol=1e-12, max_sweeps=8192), 2))
    kw = make_inputs(SPM.QQ, 8, 3, 22)
    out.append(("QQ capped by max_sweeps = 3",
                dict(kw, eps=kw["eps"][:, 0].copy(), gamma=0.9, noise_prob=0.25, agents=[1], eval_tol=1e-12, max_sweeps=3, pi=None), 1))
    kw = make_inputs(SNM.three_agents(), 8, 3, 23)
    out.append(("three agents, 0 and 2 solved", dict(kw, gamma=[0.6, 0.5, 0.4], agents=[0, 2], eval_tol=1e-12, max_sweeps=8192), 2))
    kw = make_inputs(SPM.QR, 12, 2, 24)
    out.append(("QR scalars", dict(kw, eps=kw["eps"][:, 0].copy(), gamma=[0.7, 0.8], noise_prob=0.05, agents=[0, 1], eval_tol=1e-12,
                                   max_sweeps=8192), 1))
    kw = make_inputs(SPM.RR, 8, 2, 25)
    out.append(("RR D < T", dict(kw, gamma=0.5, agents=[0, 1], eval_tol=1e-12, max_sweeps=8192), 1))
    kw = make_inputs(SPM.SHIP, 16, 2, 26)
    out.append(("SHIP resolution 16, gamma 0.5", dict(kw, gamma=0.5, agents=[0, 1], eval_tol=1e-12, max_sweeps=8192), 2))
    return out
