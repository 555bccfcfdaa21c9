"""numpy restatement of thrl_sampled_deviation_noise (include/thrl_sampled_deviation_noise.h) from given probability rows
and policies at the distinct prices and at the quadrature nodes, start distributions and the per-config tables of
th_rl_amd.sampled_play.noise_tables, written from the header: every sum runs in the stated order, every operation is one
numpy float64 operation.  The rows, M / W and the configs are tests/sampled_mirror.py's, nu and the ordered product sums
tests/sampled_noise_mirror.py's, the strategy's Q_V at V = 0 tests/sampled_response_mirror.py's (on the price rows and on
the node rows), the names of the outputs tests/sampled_deviation_mirror.py's.  Also dense(): an independent solution by
T x T matrices of normalised probabilities that the host test holds the mirror against, and write_case(): the binary case
files of tests/sampled_deviation_noise_check.cpp."""
import numpy as np

import sampled_deviation_mirror as SDM
import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import sampled_response_mirror as SRM

FLOAT, INT, AGENT, ROWS_AGENT, ROWS_GAME = SDM.FLOAT, SDM.INT, SDM.AGENT, SDM.ROWS_AGENT, SDM.ROWS_GAME


def strategy(tabs, P, Pn, Rn, deviator, action, dev_policy=None):
    """ad int [G, D + Jn], the prices first: action >= 0 that action at every state; action = -1 the first maximum of the
    one-period Q at the state with U = Rn [G, T]; or with dev_policy (uint16 [G, D + Jn]) its entries clamped to A - 1."""
    G, D, Jn = P[0].shape[0], P[0].shape[1], Pn[0].shape[1]
    A = int(tabs["n_actions"][deviator])
    if dev_policy is not None:
        return np.minimum(np.asarray(dev_policy).view(np.uint16).astype(np.int64), A - 1)
    if action >= 0:
        return np.full((G, D + Jn), int(action), np.int64)
    ad = np.zeros((G, D + Jn), np.int64)
    for g in range(G):
        for rows, lo, hi in ((P, 0, D), (Pn, D, D + Jn)):
            _, w, zm, idx = SRM.agent_tables(tabs, [p[g] for p in rows], deviator)
            ad[g, lo:hi] = SRM.q_values(w, zm, idx, Rn[g]).argmax(axis=1)
    return ad


def replaced(P, S, ad, dv):
    """(rows, Z) of a step in which agent dv plays ad [G, X] for sure: its row 1.0 at ad and 0.0 elsewhere, its sum 1.0."""
    n, X = ad.shape
    hot = np.zeros((n, X, P[dv].shape[2]))
    np.put_along_axis(hot, ad[:, :, None], 1.0, axis=2)
    Z = None
    for i in range(len(P)):
        Si = np.ones((n, X)) if i == dv else S[i]
        Z = Si if Z is None else Z * Si
    return [hot if i == dv else p for i, p in enumerate(P)], Z


def step(tabs, P, Z, Pn, Zn, act, x, p, q):
    """x' [G, T]: one step of thrl_sampled_noise_chain's chain without the lazy half."""
    W = SPM.weights(tabs, Z, x)
    V = SNM.node_mass(tabs, x) / Zn
    return q[:, None] * SNM.product_sum(W, P, act) + p[:, None] * SNM.product_sum(V, Pn, act)


def outcome(tabs, m, x0, p, q):
    """(reward [N, G], action [N, G], price [G], dist [G], mass [G]) of the distributions m against x0, the rewards and
    the price in expectation over the redrawn demand."""
    R, NR, Sc = (np.asarray(tabs[f], np.float64) for f in ("reward", "noise_reward", "scaled"))
    N = R.shape[0]
    rew = np.stack([SPM._ordered_sum(m * (q[:, None] * R[i][None, :] + p[:, None] * NR[i][None, :])) for i in range(N)])
    sca = np.stack([SPM._ordered_sum(m * Sc[i][None, :]) for i in range(N)])
    pr, npr = np.asarray(tabs["price"], np.float64)[None, :], np.asarray(tabs["noise_price"], np.float64)[None, :]
    price = SPM._ordered_sum(m * (q[:, None] * pr + p[:, None] * npr))
    return rew, sca, price, 0.5 * SPM._ordered_sum(np.abs(m - x0)), SPM._ordered_sum(m)


def analyse(tabs, probs, dpolicy, nprobs, npolicy, eps, noise_prob, weights, deviator=0, steps=12, dev_len=1, action=-1,
            dev_policy=None, gamma=0.95, ret_tol=1e-6):
    """Every output of thrl_sampled_deviation_noise and all K rows.  probs {i: float32 [G, D, A_i]}, dpolicy uint16
    [G, N, D], nprobs {i: float32 [G, Jn, A_i]}, npolicy uint16 [G, N, Jn], eps [N] numbers or [N, G], noise_prob a number
    or [G], weights [G, T], gamma a number or [G] (the deviator's), dev_policy uint16 [G, D + Jn] or None.  Also "ad"
    int [G, D + Jn]."""
    dpolicy, npolicy = np.asarray(dpolicy), np.asarray(npolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D, Jn = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"])
    K, L, dv = int(steps), int(dev_len), int(deviator)
    eps = SRM._eps_of(eps, N, G)
    gamma = np.asarray(gamma, np.float64) * np.ones(G)
    pr = np.asarray(noise_prob, np.float64) * np.ones(G)
    x0_all = np.asarray(weights, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (pr >= 0.0) & (pr <= 1.0)
        for i, kind in enumerate(tabs["kinds"]):
            if kind == "QTable":
                ok &= (eps[i] >= 0.0) & (eps[i] <= 1.0)
    out = {f: np.zeros(G) for f in FLOAT}
    out.update({f: np.full(G, -1, np.int32) for f in INT})
    out.update({f: np.zeros((N, G)) for f in AGENT})
    out.update({f: np.zeros((K, N, G)) for f in ROWS_AGENT})
    out.update({f: np.zeros((K, G)) for f in ROWS_GAME})
    out["ad"] = np.zeros((G, D + Jn), np.int64)
    idx = np.flatnonzero(ok)
    if not idx.size:
        return out
    n = idx.size
    e = np.where(ok[None, :], eps, 0.0)[:, idx]
    P, Z, _ = SPM.rows_of(tabs, {i: np.asarray(x)[idx] for i, x in probs.items()}, dpolicy[idx], e)
    ntabs = SNM.node_tabs(tabs)
    Pn, Zn, _ = SPM.rows_of(ntabs, {i: np.asarray(x)[idx] for i, x in nprobs.items()}, npolicy[idx], e)
    act = SPM.actions_of(tabs)
    S, Sn = SDM.row_sums(tabs, P), SDM.row_sums(tabs, Pn)
    p = pr[idx]
    q = 1.0 - p
    R, NR = np.asarray(tabs["reward"], np.float64), np.asarray(tabs["noise_reward"], np.float64)
    Rn = q[:, None] * R[dv][None, :] + p[:, None] * NR[dv][None, :]
    ad = strategy(tabs, P, Pn, Rn, dv, action, None if dev_policy is None else np.asarray(dev_policy)[idx])
    out["ad"][idx] = ad
    Pd, Zd = replaced(P, S, ad[:, :D], dv)
    Pnd, Znd = replaced(Pn, Sn, ad[:, D:], dv)
    x0 = x0_all[idx]
    M0 = SPM.weights(tabs, np.ones((n, D)), x0)
    nu0 = SNM.node_mass(tabs, x0)
    own = np.take_along_axis(P[dv], ad[:, :D, None], axis=2)[:, :, 0] / S[dv]
    ownn = np.take_along_axis(Pn[dv], ad[:, D:, None], axis=2)[:, :, 0] / Sn[dv]
    out["dev_share"][idx] = q * SPM._ordered_sum(M0 * (1.0 - own)) + p * SPM._ordered_sum(nu0 * (1.0 - ownn))
    rew, sca, price, _, _ = outcome(tabs, x0, x0, p, q)
    out["base_reward"][:, idx], out["base_action"][:, idx], out["base_price"][idx] = rew, sca, price
    base = rew[dv]
    gam = gamma[idx]
    w = np.ones(n)
    gain, gain_dev, low = np.zeros(n), np.zeros(n), np.zeros(n)
    low_step, ret = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    x = x0
    dist = np.zeros(n)
    mass = np.zeros(n)
    for tau in range(K):
        x = step(tabs, Pd, Zd, Pnd, Znd, act, x, p, q) if tau < L else step(tabs, P, Z, Pn, Zn, act, x, p, q)
        rew, sca, price, dist, mass = outcome(tabs, x, x0, p, q)
        out["reward_rows"][tau][:, idx], out["action_rows"][tau][:, idx] = rew, sca
        out["price_rows"][tau][idx], out["dist_rows"][tau][idx] = price, dist
        diff = rew[dv] - base
        term = w * diff
        gain = gain + term
        if tau < L:
            gain_dev = gain_dev + term
        else:
            lower = np.ones(n, bool) if tau == L else diff < low
            low = np.where(lower, diff, low)
            low_step = np.where(lower, tau, low_step).astype(np.int32)
            back = (ret < 0) & (dist <= ret_tol)
            ret = np.where(back, tau, ret).astype(np.int32)
        w = w * gam
    out["gain"][idx], out["gain_dev"][idx], out["low"][idx], out["low_step"][idx] = gain, gain_dev, low, low_step
    out["ret_step"][idx], out["dist"][idx], out["mass"][idx] = ret, dist, mass
    return out


# ------------------------------------------------------------------------------------------------ an independent solution
def dense(tabs, P, Pn, ad, x0, p, deviator, steps, dev_len):
    """For ONE game's rows P (list of float64 [D, A_j]) and Pn ([Jn, A_j]), its strategy ad [D + Jn], start x0 [T] and
    noise probability p: dict(reward [K, N], action [K, N], price [K], dist [K], mass [K], base_reward [N], dev_share)
    from the T x T matrices q * (normalised price rows) + p * (nn . normalised node rows) of the plain and the deviation
    step, numpy matrix products and numpy sums.  Shares no code with analyse() but the action digits."""
    act = SPM.actions_of(tabs)
    N, T = act.shape
    D, Jn = P[0].shape[0], Pn[0].shape[0]
    q = 1.0 - p
    row = np.asarray(tabs["row"], np.int64)
    nn = np.asarray(tabs["nn"], np.float64)

    def normal(rows):
        return [r / r.sum(axis=1, keepdims=True) for r in rows]

    def hot(like, a):
        h = np.zeros_like(like)
        h[np.arange(like.shape[0]), a] = 1.0
        return h

    def matrix(rows, nrows):
        by_price, by_node = np.ones((D, T)), np.ones((Jn, T))
        for j in range(N):
            by_price = by_price * rows[j][:, act[j]]
            by_node = by_node * nrows[j][:, act[j]]
        return q * by_price[row] + p * (nn @ by_node)               # [T, T]: from tuple t to t'

    norm, nnorm = normal(P), normal(Pn)
    plain = matrix(norm, nnorm)
    devm = matrix([hot(norm[j], ad[:D]) if j == deviator else norm[j] for j in range(N)],
                  [hot(nnorm[j], ad[D:]) if j == deviator else nnorm[j] for j in range(N)])
    R = q * np.asarray(tabs["reward"]) + p * np.asarray(tabs["noise_reward"])
    Sc = np.asarray(tabs["scaled"])
    price = q * np.asarray(tabs["price"]) + p * np.asarray(tabs["noise_price"])
    out = dict(reward=np.zeros((steps, N)), action=np.zeros((steps, N)), price=np.zeros(steps), dist=np.zeros(steps),
               mass=np.zeros(steps), base_reward=R @ x0)
    M0 = np.bincount(row, weights=x0, minlength=D)
    out["dev_share"] = float(q * np.sum(M0 * (1.0 - norm[deviator][np.arange(D), ad[:D]]))
                             + p * np.sum((x0 @ nn) * (1.0 - nnorm[deviator][np.arange(Jn), ad[D:]])))
    x = x0
    for tau in range(steps):
        x = x @ (devm if tau < dev_len else plain)
        out["reward"][tau], out["action"][tau], out["price"][tau] = R @ x, Sc @ x, price @ x
        out["dist"][tau], out["mass"][tau] = 0.5 * np.abs(x - x0).sum(), x.sum()
    return out


# ------------------------------------------------------------------------------------------------ case files
def write_case(path, tabs, probs, dpolicy, nprobs, npolicy, eps, noise_prob, weights, ref, n_blocks, deviator=0, steps=12,
               dev_len=1, action=-1, dev_policy=None, gamma=0.95, ret_tol=1e-6, row_begin=0, row_count=None):
    """The inputs and the expected outputs `ref` (analyse's) as tests/sampled_deviation_noise_check.cpp reads them."""
    dpolicy = np.asarray(dpolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D, Jn, W = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"]), int(tabs["band_w"])
    K = int(steps)
    rc = K - row_begin if row_count is None else int(row_count)
    eps, gamma, noise_prob = np.asarray(eps, np.float64), np.asarray(gamma, np.float64), np.asarray(noise_prob, np.float64)
    kind, nact = np.zeros(8, np.int32), np.zeros(8, np.int32)
    kind[:N] = [SRM.KIND[k] for k in tabs["kinds"]]
    nact[:N] = tabs["n_actions"]
    e8 = np.zeros(8)
    if eps.ndim < 2:
        e8[:N] = eps
    with open(path, "wb") as f:
        np.array([G, N, T, D, Jn, W, deviator, dev_len, K, action, int(dev_policy is not None), int(eps.ndim == 2),
                  int(gamma.ndim == 1), int(noise_prob.ndim == 1), row_begin, rc, n_blocks], np.int32).tofile(f)
        kind.tofile(f), nact.tofile(f), e8.tofile(f)
        np.array([float(gamma) if gamma.ndim == 0 else 0.0, ret_tol, float(noise_prob) if noise_prob.ndim == 0 else 0.0]).tofile(f)
        if eps.ndim == 2:
            np.ascontiguousarray(eps[:, :G]).tofile(f)
        if gamma.ndim == 1:
            sweep = np.full((N, G), np.nan)
            sweep[deviator] = gamma
            sweep.tofile(f)
        if noise_prob.ndim == 1:
            np.ascontiguousarray(noise_prob[:G]).tofile(f)
        for rows in (probs, nprobs):
            for i in range(N):
                if i in rows:
                    np.ascontiguousarray(rows[i], np.float32).tofile(f)
        np.ascontiguousarray(dpolicy, np.uint16).tofile(f)
        np.ascontiguousarray(npolicy, np.uint16).tofile(f)
        if dev_policy is not None:
            np.ascontiguousarray(dev_policy, np.uint16).tofile(f)
        for name, dt in (("grp_first", np.int32), ("grp_perm", np.int32), ("reward", np.float64), ("scaled", np.float64),
                         ("price", np.float64), ("band_lo", np.int32), ("band", np.float64), ("noise_price", np.float64),
                         ("noise_reward", np.float64)):
            np.ascontiguousarray(tabs[name], dt).tofile(f)
        np.ascontiguousarray(weights, np.float64).tofile(f)
        for name in AGENT + FLOAT:
            np.ascontiguousarray(ref[name], np.float64).tofile(f)
        for name in INT:
            np.ascontiguousarray(ref[name], np.int32).tofile(f)
        for name in ROWS_AGENT + ROWS_GAME:
            np.ascontiguousarray(ref[name][row_begin:row_begin + rc], np.float64).tofile(f)


# ------------------------------------------------------------------------------------------------ shared inputs
TILE = 64
RR5 = SNM.two_agents("Reinforce", 5, "Reinforce", 5)
# name: (config, resolution or None with n_nodes, games)
CASES = {
    "QQ": (SNM.two_agents("QTable", 2, "QTable", 2), 0, 5),
    "QQ0": (SNM.two_agents("QTable", 2, "QTable", 2, SNM.NO_ATOM), 0, 5),
    "QR": (SNM.two_agents("QTable", 2, "Reinforce", 3), 8, 4),
    "QR0": (SNM.two_agents("QTable", 2, "Reinforce", 3, SNM.NO_ATOM), 8, 4),
    "QRA": (SNM.three_agents(), 8, 3),
    "SHIP": (SNM.two_agents("QTable", 21, "Reinforce", 21), 64, 3),
}


def case_inputs(name):
    """sampled_noise_mirror.make_inputs' dict for a case, plus x0 [G, T] (random distributions), computed once per session."""
    def make():
        config, res, games = CASES[name]
        inp = SNM.make_inputs(config, res, games, 60 + len(name) + games)
        rs = np.random.RandomState(7 + games)
        x0 = rs.uniform(0.0, 1.0, (games, int(inp["tabs"]["n_tuples"])))
        inp["x0"] = x0 / x0.sum(axis=1, keepdims=True)
        inp["config"] = config
        return inp
    return SPM.cached(("sdevn-inputs", name), make)
