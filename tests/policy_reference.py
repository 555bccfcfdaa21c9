"""Float64 mirror of the device policy (th_rl_amd/csrc/thrl_policy.h: the 1 -> 256 -> A network, softmax, inverse-CDF
sample, argmax) and the bounds the device is held to -- TEST INFRASTRUCTURE ONLY, plain numpy.

The device works in float32 (u = 2^-24, gamma_n = n u / (1 - n u)).  A logit is formed by one fma for the hidden unit,
four chained fmas per lane, six reduction levels, the bias add and the subtraction of the maximum: at most 13 roundings
on terms whose absolute values sum to S_k = sum_j |W2_kj h_j| + |b2_k|, so its error is at most gamma_13 * max_k S_k.
A softmax whose logits move by at most e moves each probability by a factor within exp(+-2 e) (numerator and sum);
expf, the six-level sum and the division add 16 u.  Hence

    |dp_k| <= p_k * (2 gamma_13 max_k S_k + 16 u) + 1e-8                                          (prob_bound)

(1e-8 is the project's absolute tolerance: probabilities that underflow).  The bound is derived, not tuned; at the
initial weight scale it is about 3.5e-5 relative, and tests there take the tighter of it and the project's
rtol 2e-5 / atol 1e-8 (init_scale=True).

The sampler takes the first action whose float32 running sum exceeds the float32-rounded draw, the last action if none
does.  With C_k the float64 CDF, any summation order of k + 1 float32 terms errs by at most (k + 1) u C_k, so with

    tau_k = sum_{j<=k} bound_j + (k + 1) u C_k

action a can come out only if  C_{a-1} - tau_{a-1} <= u32 < C_a + tau_a  (window), the last action also when
u32 >= C_{A-1} - tau_{A-1} (the fallback).
"""
import numpy as np

H = 256
U = 2.0 ** -24
GAMMA13 = 13 * U / (1 - 13 * U)
ATOL = 1e-8
PROJECT_RTOL = 2e-5


def n_policy_params(A):
    return 2 * H + A * H + A


def probs64(w, A, price, value_head=False):
    """Probabilities [n, A] in float64 and S [n, A] (see above) of the policy with the float32 parameters `w` at the
    float32-rounded prices [n].  w is one parameter vector [P] (every price uses it) or one per price [n, P].
    value_head: w carries ActorCritic's fc_v (256 weights and a bias) behind the policy's parameters; it is not read."""
    A = int(A)
    Pp = n_policy_params(A)
    w = np.asarray(w)
    assert w.dtype == np.float32, w.dtype
    assert w.shape[-1] == Pp + (H + 1 if value_head else 0), (w.shape, A, value_head)
    x = np.atleast_1d(np.asarray(price, np.float64)).astype(np.float32).astype(np.float64)
    w = w.astype(np.float64)
    if w.ndim == 1:
        w = np.broadcast_to(w, (len(x), w.shape[0]))
    assert w.shape[0] == len(x), (w.shape, x.shape)
    w1, b1 = w[:, :H], w[:, H:2 * H]
    W2 = w[:, 2 * H:2 * H + A * H].reshape(len(x), A, H)
    b2 = w[:, 2 * H + A * H:Pp]
    h = np.maximum(w1 * x[:, None] + b1, 0.0)
    terms = W2 * h[:, None, :]
    z = terms.sum(axis=2) + b2
    S = np.abs(terms).sum(axis=2) + np.abs(b2)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), S


def prob_bound(p64, S, init_scale=False):
    """The derived bound on |p_device - p64| per entry.  init_scale: the tighter of it and the project's rtol / atol."""
    p64 = np.asarray(p64, np.float64)
    rel = 2.0 * GAMMA13 * np.asarray(S, np.float64).max(axis=-1, keepdims=True) + 16.0 * U
    if init_scale:
        rel = np.minimum(rel, PROJECT_RTOL)
    return p64 * rel + ATOL


def _cdf_tau(p64, bound):
    C = np.cumsum(p64, axis=-1)
    k1 = np.arange(1, p64.shape[-1] + 1, dtype=np.float64)
    return C, np.cumsum(bound, axis=-1) + k1 * U * C


def window(p64, bound, u32):
    """Admissible sampled actions: bool [n, A] for the draws u32 [n] (already rounded to float32)."""
    p64 = np.atleast_2d(np.asarray(p64, np.float64)); bound = np.atleast_2d(np.asarray(bound, np.float64))
    u = np.atleast_1d(np.asarray(u32))
    assert u.dtype == np.float32, "the draw is rounded to float32 as the kernels round it"
    u = u.astype(np.float64)[:, None]
    C, tau = _cdf_tau(p64, bound)
    lo = np.concatenate([np.zeros_like(C[:, :1]), (C - tau)[:, :-1]], axis=1)
    ok = (lo <= u) & (u < C + tau)
    ok[:, -1] |= u[:, 0] >= (C - tau)[:, -1]
    return ok


def argmax_set(p64, bound):
    """Actions whose probability could be the maximum within the bound: bool [n, A]."""
    p64 = np.atleast_2d(np.asarray(p64, np.float64)); bound = np.atleast_2d(np.asarray(bound, np.float64))
    return p64 + bound >= (p64 - bound).max(axis=1, keepdims=True)


def decisive_draws(p64, bound):
    """Draws at which the window admits exactly one action.  With tau = tau_{A-1} (the largest), every action with
    p_k > 8 tau gives the midpoint of its CDF interval and the two points 4 tau inside its ends (rounding a draw to
    float32 moves it by at most u <= tau / 2, so it stays 3 tau inside).  One row [A] in; returns (draws float64 [m],
    actions int [m])."""
    p64 = np.asarray(p64, np.float64); bound = np.asarray(bound, np.float64)
    assert p64.ndim == 1
    C, tau = _cdf_tau(p64, bound)
    t = tau[-1]
    lo = np.concatenate([[0.0], C[:-1]])
    ks = np.flatnonzero(p64 > 8.0 * t)
    draws = np.stack([lo[ks] + 4.0 * t, 0.5 * (lo[ks] + C[ks]), C[ks] - 4.0 * t], axis=1).ravel()
    return draws, np.repeat(ks, 3)


def decisive_actions(p64, bound):
    """The actions decisive_draws covers: p_k > 8 tau_{A-1}."""
    p64 = np.asarray(p64, np.float64)
    _, tau = _cdf_tau(p64, np.asarray(bound, np.float64))
    return np.flatnonzero(p64 > 8.0 * tau[-1])


# ------------------------------------------------------------------------------------------------ weight regimes
A_GRID = (2, 3, 7, 8, 9, 16, 17, 21, 24, 25, 31, 32)       # dispatch edges 8|9 and 24|25, DPP row edges, odd A, all 64 lanes


def host_init(G, A, value_head, rs):
    """Weights with the distribution of the device's init (thrl_nn_init): fc1 ~ U(-1, 1), fc_pi / fc_v.weight ~
    U(-1/16, 1/16), fc_v.bias = 1000 -- for the host tests, which have no device to draw them."""
    Pp = n_policy_params(A)
    w = np.empty((G, Pp + (H + 1 if value_head else 0)), np.float32)
    w[:, :2 * H] = rs.uniform(-1, 1, (G, 2 * H))
    w[:, 2 * H:] = rs.uniform(-1, 1, (G, w.shape[1] - 2 * H)) / 16.0
    if value_head:
        w[:, Pp + H] = 1000.0
    return w


def regimes(w, A):
    """The weight regimes of the policy tests from initial weights w [G, P]: name -> (weights, init_scale)."""
    return {"init": (np.array(w, np.float32, copy=True), True), "x8": (scale_head(w, A, 8), False),
            "x40": (scale_head(w, A, 40), False), "uniform": (zero_head(w, A), False),
            "ties": (planted_ties(w, A)[0], False)}


def scale_head(w, A, factor):
    """fc_pi weights and bias times `factor` (peaked policies, probabilities that underflow, flat CDF tails)."""
    w = np.array(w, np.float32, copy=True)
    w[..., 2 * H:n_policy_params(A)] *= np.float32(factor)
    return w


def zero_head(w, A):
    """fc_pi.weight = 0 and b2 = 0: p = 1 / A exactly."""
    w = np.array(w, np.float32, copy=True)
    w[..., 2 * H:n_policy_params(A)] = 0.0
    return w


def tie_sets(A):
    """Positions of planted equal biases: pairs and triples, with {0, A-1} and pairs straddling every DPP row edge
    (8 actions per row) that A reaches."""
    sets = [(0, A - 1)] if A > 1 else []
    for edge in (8, 16, 24):
        if A > edge:
            sets.append((edge - 1, edge))
    if A >= 3:
        sets.append((0, A // 2, A - 1))
        sets.append((A - 3, A - 2, A - 1))
    if A >= 4:
        sets.append((A // 2 - 1, A // 2))
    if A > 9:
        sets.append((1, 7, 8))
    return sets


def planted_ties(w, A, value=2.0):
    """fc_pi.weight = 0, b2 = `value` at the positions of tie_sets(A)[g % len] for game g, 0 elsewhere.  w is [G, P];
    returns (weights, list of the tied positions per game)."""
    w = zero_head(w, A)
    sets = tie_sets(A)
    tied = []
    for g in range(w.shape[0]):
        s = sets[g % len(sets)]
        w[g, 2 * H + A * H + np.asarray(s)] = np.float32(value)
        tied.append(s)
    return w, tied


def probe_prices(n, rs, grid=None):
    """0.0, grid prices and continuous values in [0, 10): n of them, in that order of preference."""
    grid = np.round(np.linspace(2.0, 6.0, 41), 10) if grid is None else np.asarray(grid, np.float64)
    p = rs.uniform(0.0, 10.0, n)
    p[::3] = grid[rs.randint(0, len(grid), len(p[::3]))]
    p[0] = 0.0
    return p
