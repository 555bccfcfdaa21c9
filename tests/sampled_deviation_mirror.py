"""numpy restatement of thrl_sampled_deviation (include/thrl_sampled_deviation.h) from given probability rows, dpolicy,
start distributions and the per-config tables of th_rl_amd.sampled_play.tables, written from the definitions: every sum
runs in the stated order (np.add.accumulate from 0.0 along the summed axis, or a loop over d with vector operations over
the tuples and the games), every operation is one numpy float64 operation.  The configs, weights and row generators are
tests/sampled_mirror.py's, q(d, k) is tests/sampled_response_mirror.py's Q_V at V = 0.  Also dense(): an independent
solution by T x T matrices of normalised probabilities that the host test holds the mirror against, and write_case(): the
binary case files of tests/sampled_deviation_check.cpp."""
import numpy as np

import sampled_mirror as SPM
import sampled_response_mirror as SRM

FLOAT = ("base_price", "dev_share", "gain", "gain_dev", "low", "dist", "mass")
INT = ("low_step", "ret_step")
AGENT = ("base_reward", "base_action")
ROWS_AGENT = ("reward_rows", "action_rows")
ROWS_GAME = ("price_rows", "dist_rows")


def row_sums(tabs, P):
    """S [N, G, D]: 1.0 exactly for a QTable agent, else the ascending sum of the widened row."""
    return np.stack([np.ones(p.shape[:2]) if k == "QTable" else SPM._ordered_sum(p) for k, p in zip(tabs["kinds"], P)])


def strategy(tabs, P, deviator, action, dev_policy=None):
    """ad int [G, D]: action >= 0 that action at every price; action = -1 the first maximum of q(d, .), or with
    dev_policy (uint16 [G, D]) its entries clamped to A - 1."""
    G, D = P[0].shape[0], P[0].shape[1]
    A = int(tabs["n_actions"][deviator])
    if dev_policy is not None:
        return np.minimum(np.asarray(dev_policy).view(np.uint16).astype(np.int64), A - 1)
    if action >= 0:
        return np.full((G, D), int(action), np.int64)
    R = np.asarray(tabs["reward"], np.float64)[deviator]
    ad = np.zeros((G, D), np.int64)
    for g in range(G):
        _, w, zm, idx = SRM.agent_tables(tabs, [p[g] for p in P], deviator)
        ad[g] = SRM.q_values(w, zm, idx, R).argmax(axis=1)
    return ad


def price_sums(tabs, P, Z, act, m):
    """x' [G, T]: one step of the chain without the lazy half."""
    W = SPM.weights(tabs, Z, m)
    s = np.zeros_like(m)
    for d in range(W.shape[1]):
        w = W[:, d]
        live = w != 0.0
        if not live.any():
            continue
        term = w[:, None]
        for i, p in enumerate(P):
            term = term * p[:, d, :][:, act[i]]
        new = s + term
        s = new if live.all() else np.where(live[:, None], new, s)
    return s


def outcome(tabs, m, x0):
    """(reward [N, G], action [N, G], price [G], dist [G], mass [G]) of the distributions m against x0."""
    R, Sc = np.asarray(tabs["reward"], np.float64), np.asarray(tabs["scaled"], np.float64)
    N = R.shape[0]
    rew = np.stack([SPM._ordered_sum(m * R[i][None, :]) for i in range(N)])
    sca = np.stack([SPM._ordered_sum(m * Sc[i][None, :]) for i in range(N)])
    price = SPM._ordered_sum(m * np.asarray(tabs["price"], np.float64)[None, :])
    return rew, sca, price, 0.5 * SPM._ordered_sum(np.abs(m - x0)), SPM._ordered_sum(m)


def analyse(tabs, probs, dpolicy, eps, weights, deviator=0, steps=12, dev_len=1, action=-1, dev_policy=None, gamma=0.95,
            ret_tol=1e-6):
    """Every output of thrl_sampled_deviation and all K rows.  probs {i: float32 [G, D, A_i]}, dpolicy uint16 [G, N, D],
    eps [N] numbers or [N, G], weights [G, T], gamma a number or [G] (the deviator's), dev_policy uint16 [G, D] or None."""
    dpolicy = np.asarray(dpolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    K, L, dv = int(steps), int(dev_len), int(deviator)
    eps = SRM._eps_of(eps, N, G)
    gamma = np.asarray(gamma, np.float64) * np.ones(G)
    x0_all = np.asarray(weights, np.float64)
    ok = np.ones(G, bool)
    for i, kind in enumerate(tabs["kinds"]):
        if kind == "QTable":
            ok &= (eps[i] >= 0.0) & (eps[i] <= 1.0)
    out = {f: np.zeros(G) for f in FLOAT}
    out.update({f: np.full(G, -1, np.int32) for f in INT})
    out.update({f: np.zeros((N, G)) for f in AGENT})
    out.update({f: np.zeros((K, N, G)) for f in ROWS_AGENT})
    out.update({f: np.zeros((K, G)) for f in ROWS_GAME})
    out["ad"] = np.zeros((G, D), np.int64)
    idx = np.flatnonzero(ok)
    if not idx.size:
        return out
    n = idx.size
    sub = {i: np.asarray(p)[idx] for i, p in probs.items()}
    P, Z, _ = SPM.rows_of(tabs, sub, dpolicy[idx], np.where(ok[None, :], eps, 0.0)[:, idx])
    act = SPM.actions_of(tabs)
    S = row_sums(tabs, P)
    A = int(tabs["n_actions"][dv])
    ad = strategy(tabs, P, dv, action, None if dev_policy is None else np.asarray(dev_policy)[idx])
    out["ad"][idx] = ad
    onehot = np.zeros((n, D, A))
    np.put_along_axis(onehot, ad[:, :, None], 1.0, axis=2)
    Pd = [onehot if i == dv else p for i, p in enumerate(P)]
    Zd = None
    for i in range(N):
        Si = np.ones((n, D)) if i == dv else S[i]
        Zd = Si if Zd is None else Zd * Si
    x0 = x0_all[idx]
    M0 = SPM.weights(tabs, np.ones((n, D)), x0)
    own = np.take_along_axis(P[dv], ad[:, :, None], axis=2)[:, :, 0] / S[dv]
    out["dev_share"][idx] = SPM._ordered_sum(M0 * (1.0 - own))
    rew, sca, price, _, _ = outcome(tabs, x0, x0)
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
        x = price_sums(tabs, Pd, Zd, act, x) if tau < L else price_sums(tabs, P, Z, act, x)
        rew, sca, price, dist, mass = outcome(tabs, x, x0)
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
def dense(tabs, P, ad, x0, deviator, steps, dev_len):
    """For ONE game's rows P (list of float64 [D, A_j]), its strategy ad [D] and start x0 [T]: dict(reward [K, N], action
    [K, N], price [K], dist [K], mass [K], base_reward [N], dev_share) from the T x T matrices of the plain and the
    deviation step built from NORMALISED probabilities, numpy matrix products and numpy sums.  Shares no code with
    analyse() but the action digits."""
    act = SPM.actions_of(tabs)
    N, T = act.shape
    D = P[0].shape[0]
    row = np.asarray(tabs["row"], np.int64)
    norm = [p / p.sum(axis=1, keepdims=True) for p in P]
    hot = np.zeros_like(norm[deviator])
    hot[np.arange(D), ad] = 1.0

    def matrix(rows):
        by_price = np.ones((D, T))
        for j in range(N):
            by_price = by_price * rows[j][:, act[j]]
        return by_price[row]                                        # [T, T]: from tuple t to t'

    plain = matrix(norm)
    devm = matrix([hot if j == deviator else norm[j] for j in range(N)])
    R, Sc, price = np.asarray(tabs["reward"]), np.asarray(tabs["scaled"]), np.asarray(tabs["price"])
    out = dict(reward=np.zeros((steps, N)), action=np.zeros((steps, N)), price=np.zeros(steps), dist=np.zeros(steps),
               mass=np.zeros(steps), base_reward=R @ x0)
    M0 = np.bincount(row, weights=x0, minlength=D)
    out["dev_share"] = float(np.sum(M0 * (1.0 - norm[deviator][np.arange(D), ad])))
    x = x0
    for tau in range(steps):
        x = x @ (devm if tau < dev_len else plain)
        out["reward"][tau], out["action"][tau], out["price"][tau] = R @ x, Sc @ x, price @ x
        out["dist"][tau], out["mass"][tau] = 0.5 * np.abs(x - x0).sum(), x.sum()
    return out


# ------------------------------------------------------------------------------------------------ case files
def write_case(path, tabs, probs, dpolicy, eps, weights, ref, n_blocks, deviator=0, steps=12, dev_len=1, action=-1,
               dev_policy=None, gamma=0.95, ret_tol=1e-6, row_begin=0, row_count=None):
    """The inputs and the expected outputs `ref` (analyse's) as tests/sampled_deviation_check.cpp reads them."""
    dpolicy = np.asarray(dpolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    K = int(steps)
    rc = K - row_begin if row_count is None else int(row_count)
    eps, gamma = np.asarray(eps, np.float64), np.asarray(gamma, np.float64)
    kind, nact = np.zeros(8, np.int32), np.zeros(8, np.int32)
    kind[:N] = [SRM.KIND[k] for k in tabs["kinds"]]
    nact[:N] = tabs["n_actions"]
    e8 = np.zeros(8)
    if eps.ndim < 2:
        e8[:N] = eps
    with open(path, "wb") as f:
        np.array([G, N, T, D, deviator, dev_len, K, action, int(dev_policy is not None), int(eps.ndim == 2),
                  int(gamma.ndim == 1), row_begin, rc, n_blocks], np.int32).tofile(f)
        kind.tofile(f), nact.tofile(f), e8.tofile(f)
        np.array([float(gamma) if gamma.ndim == 0 else 0.0, ret_tol]).tofile(f)
        if eps.ndim == 2:
            np.ascontiguousarray(eps[:, :G]).tofile(f)
        if gamma.ndim == 1:
            sweep = np.full((N, G), np.nan)
            sweep[deviator] = gamma
            sweep.tofile(f)
        for i in range(N):
            if i in probs:
                np.ascontiguousarray(probs[i], np.float32).tofile(f)
        np.ascontiguousarray(dpolicy, np.uint16).tofile(f)
        if dev_policy is not None:
            np.ascontiguousarray(dev_policy, np.uint16).tofile(f)
        for name, dt in (("grp_first", np.int32), ("grp_perm", np.int32), ("reward", np.float64), ("scaled", np.float64),
                         ("price", np.float64)):
            np.ascontiguousarray(tabs[name], dt).tofile(f)
        np.ascontiguousarray(weights, np.float64).tofile(f)
        for name in AGENT + FLOAT:
            np.ascontiguousarray(ref[name], np.float64).tofile(f)
        for name in INT:
            np.ascontiguousarray(ref[name], np.int32).tofile(f)
        for name in ROWS_AGENT + ROWS_GAME:
            np.ascontiguousarray(ref[name][row_begin:row_begin + rc], np.float64).tofile(f)


# ------------------------------------------------------------------------------------------------ shared inputs
CONFIGS = {"QQ": SPM.QQ, "QR": SPM.QR, "QRA": SPM.QRA, "RR": SPM.RR, "SHIP": SPM.SHIP}
GAMES = {"QQ": 5, "QR": 4, "QRA": 3, "RR": 1, "SHIP": 3}


def case_inputs(name):
    """(tabs, probs, dpolicy, eps [N, G], x0 [G, T]) of a case, computed once per session."""
    return SPM.cached(("sdev-inputs", name), lambda: SRM.make_inputs(CONFIGS[name], GAMES[name], 40 + len(name) + GAMES[name]))
