"""numpy restatement of thrl_sampled_chain (include/thrl.h) from given probability rows, dpolicy and the per-config
tables of th_rl_amd.sampled_play.tables, written from the definitions: every sum runs in the stated order (a loop over d
with vector operations over t' and over the games), every operation is one numpy float64 operation.  Also the inputs the
host and device tests share: the configs, random networks (peaked in part of the games), a numpy forward pass of the
1 -> 256 -> A network (close to the device's, not bit-equal: the device tests take the device's own probabilities) and a
cache of the references, so that a session computes each once."""
import numpy as np

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
RF = dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])
QQ = {"agents": [dict(AG, actions=2), dict(AG, actions=2)], "environment": dict(ENV)}                      # T = 4, no network
QR = {"agents": [dict(AG, actions=2), dict(RF, actions=3)], "environment": dict(ENV)}                      # T = 6
QRA = {"agents": [dict(AG, actions=2, states=30, action_range=[0.1, 0.3]), dict(RF, actions=3, action_range=[0.05, 0.25]),
                  dict(RF, name="ActorCritic", actions=2, action_range=[0.0, 0.3])],
       "environment": dict(ENV, nplayers=3, max_steps=40)}                                                 # T = 12
SHIP = {"agents": [dict(AG), dict(RF)], "environment": dict(ENV)}                                          # T = D = 441
# two networks on one k / A grid whose sums are exact in float64 (steps of 1 / 128): 41 distinct prices
RR = {"agents": [dict(RF, action_range=[0.125, 0.125 + 21.0 / 128.0]), dict(RF, action_range=[0.125, 0.125 + 21.0 / 128.0])],
      "environment": dict(ENV)}
CAC = {"agents": [dict(AG), dict(name="CAC", gamma=0.99, states=1, action_range=[0.2, 0.4])], "environment": dict(ENV)}
WIDE = {"agents": [dict(AG, actions=129), dict(RF, actions=32)], "environment": dict(ENV)}                 # 4128 tuples
# (config, T, games, max_iters, seed): the three action sets with networks the device is compared on, and T = 4
CASES = {"QR": (QR, 6, 203, 64, 71), "QRA": (QRA, 12, 203, 64, 72), "SHIP": (SHIP, 441, 203, 12, 73), "QQ": (QQ, 4, 203, 64, 74)}
NETWORK_CASES = ("QR", "QRA", "SHIP")
H = 256


# ------------------------------------------------------------------------------------------------ inputs
def param_count(A, kind):
    return 2 * H + A * H + A + (H + 1 if kind == "ActorCritic" else 0)


def random_weights(rs, n_games, A, kind, lo, hi):
    """w1 ~ U(-1, 1), b1 = -w1 * c with c ~ U(lo, hi) per hidden unit (kinks inside the price range), fc_pi ~ U(-1, 1)
    / 4, so that an untouched game's softmax is spread; fc_pi scaled by 8 in the games g with g % 4 != 0: peaked rows.  A
    value head keeps zeros."""
    w = np.zeros((n_games, param_count(A, kind)), np.float32)
    w1 = rs.uniform(-1, 1, (n_games, H))
    c = rs.uniform(lo, hi, (n_games, H))
    w[:, :H], w[:, H:2 * H] = w1, -w1 * c
    n2 = A * H + A
    pi = rs.uniform(-1, 1, (n_games, n2)) / 4.0
    pi[np.arange(n_games) % 4 != 0] *= 8.0
    w[:, 2 * H:2 * H + n2] = pi
    return w


def case_weights(name, tabs):
    """{agent index: float32 [G, P]} for the networks of CASES[name]."""
    config, _, n_games, _, seed = CASES[name]
    rs = np.random.RandomState(seed)
    price = tabs["price"]
    return {i: random_weights(rs, n_games, int(tabs["n_actions"][i]), k, price.min(), price.max())
            for i, k in enumerate(tabs["kinds"]) if k != "QTable"}


def net_probs(w, A, prices):
    """float32 [G, J, A]: softmax(fc_pi(relu(fc1(x)))) at the float32 prices, in float32 numpy (agents.py:148-163)."""
    w = np.asarray(w, np.float32)
    x = np.asarray(prices, np.float64).astype(np.float32)
    h = np.maximum(w[:, None, :H] * x[None, :, None] + w[:, None, H:2 * H], np.float32(0))      # [G, J, H]
    W2 = w[:, 2 * H:2 * H + A * H].reshape(-1, A, H)
    z = np.einsum("gjh,gah->gja", h, W2).astype(np.float32) + w[:, None, 2 * H + A * H:2 * H + A * H + A]
    e = np.exp(z - z.max(axis=2, keepdims=True)).astype(np.float32)
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def random_dpolicy(rs, n_games, tabs, n_runs=2):
    """uint16 [G, N, D]: per agent a few random runs of one action over the ascending prices, as a strategy that is
    piecewise constant in the price has; 3 % of the entries at or above the action count, game 3's agent 0 at 65535
    throughout."""
    D, acts = int(tabs["n_prices"]), [int(a) for a in tabs["n_actions"]]
    pol = np.zeros((n_games, len(acts), D), np.uint16)
    for i, A in enumerate(acts):
        runs = rs.randint(0, A, (n_games, n_runs))
        edge = np.sort(rs.randint(0, D + 1, (n_games, n_runs - 1)), axis=1)
        which = (np.arange(D)[None, None, :] >= edge[:, :, None]).sum(axis=1)
        pol[:, i] = np.take_along_axis(runs, which, axis=1)
        pol[:, i][rs.rand(n_games, D) < 0.03] += np.uint16(A)
    if n_games > 3:
        pol[3, 0, :] = 65535
    return pol


def greedy_of(probs, tabs, rs, n_games):
    """dpolicy whose network entries are the rows' first maxima (what thrl_price_policy gives up to ties in the last
    bit) and whose QTable entries are random."""
    pol = random_dpolicy(rs, n_games, tabs)
    for i, p in probs.items():
        pol[:, i] = p.argmax(axis=2).astype(np.uint16)
    return pol


def case_epsilon(name, tabs):
    """float64 [N, G] in [0, 0.1], 0 in every fourth game; the caller mixes bad entries in."""
    _, _, n_games, _, seed = CASES[name]
    e = np.random.RandomState(seed + 500).uniform(0.0, 0.1, (len(tabs["kinds"]), n_games))
    e[:, ::4] = 0.0
    return e


def case_starts(name, tabs):
    _, T, n_games, _, seed = CASES[name]
    s = np.random.RandomState(seed + 900).randint(0, T, n_games).astype(np.int32)
    if n_games > 8:
        s[2], s[5] = -1, T
    return s


# ------------------------------------------------------------------------------------------------ the chain
def _ordered_sum(x):
    """sum over the last axis in ascending index from 0.0, one addition per term."""
    z = np.zeros(x.shape[:-1] + (1,), np.float64)
    return np.add.accumulate(np.concatenate([z, x], axis=-1), axis=-1)[..., -1]


def actions_of(tabs):
    """int [N, T]: a_i(t), agent 0 slowest."""
    acts = [int(a) for a in tabs["n_actions"]]
    return np.stack(np.unravel_index(np.arange(int(tabs["n_tuples"])), acts))


def rows_of(tabs, probs, dpolicy, eps):
    """(P: list of float64 [G, D, A_i], Z [G, D], greedy int [G, N, D]) by the header's "Probabilities"."""
    acts = [int(a) for a in tabs["n_actions"]]
    G = dpolicy.shape[0]
    D = int(tabs["n_prices"])
    greedy = np.minimum(np.asarray(dpolicy).view(np.uint16).astype(np.int64), np.asarray(acts)[None, :, None] - 1)
    P, Z = [], None
    for i, (kind, A) in enumerate(zip(tabs["kinds"], acts)):
        if kind == "QTable":
            e = np.asarray(eps[i], np.float64) * np.ones(G)
            lo = e / float(A)
            hi = (1.0 - e) + lo
            p = np.repeat(np.repeat(lo[:, None, None], D, axis=1), A, axis=2)
            np.put_along_axis(p, greedy[:, i, :, None], hi[:, None, None], axis=2)
            S = np.ones((G, D))
        else:
            p = np.asarray(probs[i], np.float32).astype(np.float64)
            S = _ordered_sum(p)
        P.append(p)
        Z = S if Z is None else Z * S
    return P, Z, greedy


def weights(tabs, Z, m):
    """W [G, D] = M / Z with M(d) the mass on the tuples of price d, added in ascending t from 0.0."""
    first, perm = np.asarray(tabs["grp_first"]), np.asarray(tabs["grp_perm"])
    D = int(tabs["n_prices"])
    M = np.zeros((m.shape[0], D))
    size = np.diff(first)
    for j in range(int(size.max())):
        d = np.flatnonzero(size > j)
        M[:, d] = M[:, d] + m[:, perm[first[d] + j]]
    return M / Z


def step(tabs, P, Z, act, m):
    """(m', chg [G]) for the iterates m [G, T]."""
    W = weights(tabs, Z, m)
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
    new = 0.5 * m + 0.5 * s
    return new, np.fmax.reduce(np.abs(new - m), axis=1, initial=0.0)


def analyse(tabs, probs, dpolicy, eps, start=None, tol=1e-12, max_iters=8192):
    """Every output of thrl_sampled_chain.  probs {i: float32 [G, D, A_i]}, dpolicy uint16 [G, N, D], eps [N] numbers or
    [N, G]; start None (uniform) or int [G]."""
    dpolicy = np.asarray(dpolicy)
    G, N = dpolicy.shape[0], dpolicy.shape[1]
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    eps = np.asarray(eps, np.float64)
    eps = np.repeat(eps[:, None], G, axis=1) if eps.ndim == 1 else eps[:, :G]
    ok = np.ones(G, bool)
    for i, kind in enumerate(tabs["kinds"]):
        if kind == "QTable":
            ok &= (eps[i] >= 0.0) & (eps[i] <= 1.0)
    if start is not None:
        start = np.asarray(start, np.int64).reshape(-1)[:G]
        ok &= (start >= 0) & (start < T)
    out = {"iters": np.full(G, -1, np.int32), "change": np.zeros(G), "mass": np.zeros(G), "samp_price": np.zeros(G),
           "agree": np.zeros(G), "samp_reward": np.zeros((N, G)), "samp_action": np.zeros((N, G)), "pi": np.zeros((G, T))}
    idx = np.flatnonzero(ok)
    if not idx.size:
        return out
    sub = {i: np.asarray(p)[idx] for i, p in probs.items()}
    P, Z, greedy = rows_of(tabs, sub, dpolicy[idx], np.where(ok[None, :], eps, 0.0)[:, idx])
    act = actions_of(tabs)
    if start is None:
        m = np.full((idx.size, T), 1.0 / float(T))
    else:
        m = np.zeros((idx.size, T))
        m[np.arange(idx.size), start[idx]] = 1.0
    iters = np.zeros(idx.size, np.int32)
    change = np.zeros(idx.size)
    live = np.arange(idx.size)
    while live.size:
        new, chg = step(tabs, [p[live] for p in P], Z[live], act, m[live])
        m[live] = new
        iters[live] += 1
        change[live] = chg
        live = live[~((chg <= tol) | (iters[live] >= max_iters))]
    W = weights(tabs, Z, m)
    term = W
    for i, p in enumerate(P):
        term = term * np.take_along_axis(p, greedy[:, i, :, None], axis=2)[:, :, 0]
    out["iters"][idx], out["change"][idx], out["pi"][idx] = iters, change, m
    out["mass"][idx] = _ordered_sum(m)
    out["agree"][idx] = _ordered_sum(term)
    out["samp_price"][idx] = _ordered_sum(m * np.asarray(tabs["price"])[None, :])
    for i in range(N):
        out["samp_reward"][i, idx] = _ordered_sum(m * np.asarray(tabs["reward"])[i][None, :])
        out["samp_action"][i, idx] = _ordered_sum(m * np.asarray(tabs["scaled"])[i][None, :])
    return out


# ------------------------------------------------------------------------------------------------ shared references
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]
