"""Float64 mirror of the forward side of the continuous agent CAC (th_rl_amd/csrc/thrl_cac.h: cac_policy, softplus_f,
sigmoid_f, box_muller_f; k_cac_act of thrl_cac.hip; the same code with the weights in LDS in the fused episode kernel
of thrl_mixed.hip) and the bounds the device is held to -- TEST INFRASTRUCTURE ONLY, plain numpy.

The device works in float32 (u = 2^-24, gamma_n = n u / (1 - n u)); the library is built with -ffp-contract=off, so
every operation below rounds on its own.

Pre-activation.  m, s and v are each formed by one fma for the hidden unit, four chained fmas per lane, six reduction
levels of wave_all and the bias add: 12 roundings on terms whose absolute values sum to S = sum_j |w_j h_j| + |b|, so
    |m_dev - m| <= E_m = gamma_12 S_m          (likewise E_s, E_v; v has no function behind it: bound_v = E_v + floor).

Propagation.  tanh, softplus and the sigmoid are monotone, so a pre-activation within [x - E, x + E] gives a value
between f(x - E) and f(x + E): the first-order term |f'| E (f' = 4 (1 - tanh^2 m), sigmoid(s), a (1 - a)) is taken as
the larger endpoint difference max |f(x +- E) - f(x)| = |f'(xi)| E for a xi of the interval, which stays valid where
f' changes over E (tanh saturating, s around 20).  The float32 intrinsic adds K u |value|:
    bound_mu = max |4 tanh(m +- E_m) - mu| + K_mu u |mu| + floor          (tanhf, the exact product by 4)
    bound_sd = max |softplus(s +- E_s) - sd| + K_sd u sd + floor          (expf + log1pf; s > 20: the value itself)
The sigmoid a = 1 / (1 + expf(-x)) errs by K_a q(a), q(a) = min(u a, 1 - a): a relative error d of expf moves a by
a (1 - a) d, and neither the add nor the divide can err by more than the distance to the float 1.0, which is e = expf(-x)
(a^2 e = a (1 - a) on the action) for the add and 1 - a for the divide.  So where expf(-x) is below u / 2 the action
is exactly 1.0f, and the bound says so.
    x = mu (mean action), or x = fl(mu + fl(sd z32)): two separately rounded operations, with
    E_prod = bound_sd (|z| + E_z) + sd E_z + u (sd + bound_sd)(|z| + E_z) + floor
    E_x    = (bound_mu + E_prod)(1 + u) + u |x|
    bound_a = max |sigmoid(x +- E_x) - a| + K_a q(a) + floor

Flush to zero.  floor = 2^-126 on every output: the device may flush a subnormal sd or action to zero (the mirror's sd
at s = -104 is 6.8e-46).  Where value + (bound - floor) is below 2^-150, half the smallest subnormal, a float32 result
can only be 0 whether it is flushed or rounded (exact32).

Sampling.  z = sqrt(-2 ln(1 - u1)) cos(2 pi u2) in float64 on both sides, rounded to float32 on the device; the mirror
keeps the float64 value, so E_z = u |z| + e_libm.  1 - u1 is exact (u1 is a multiple of 2^-32).  With r the radius: a
log within 3 ulp and a correctly rounded sqrt leave r within 2.5 * 2^-53 r; the argument 2 pi u2 carries the rounding
of the constant and of the product, 2 * 2^-53 * 2 pi absolute, and a cos within 4 ulp adds 4 * 2^-53: 16.6 * 2^-53
absolute on the cosine, which is why the term is absolute (cos(2 pi 0.25) is 6e-17 here, not 0); the final product one
more 2^-53.  Per side |dz| <= 2^-53 (16.6 r + 3.5 |z|), and for the two sides
    e_libm = 2^-53 (34 r + 8 |z|)                                         (at most 2.6e-14, at r = 6.66).

The K's cannot be derived (no accuracy table of the device library is at hand); they are measured as
update_reference.ORACLE_ERR was: the float32 numpy oracle (oracle/nn_oracle.py: cac_forward, cac_sample_action,
cac_mean_action) against this mirror on the CPU, over every item of every case below, in units of the bound with one
rounding and K = 1 (unit = bounds(gam=u, K=1)), i.e. of  u S |f'| + u |value| + 2^-126:
    ORACLE_ERR = largest |oracle - mirror| / unit per output,    K = 4 x ORACLE_ERR
(4 for the device's other summation order and intrinsics, as in update_reference).  tests/test_cac_reference_host.py
asserts the recorded figures and that the oracle lies inside every bound.  No figure observed on the device enters a
bound.  Observed on an MI355X (tests/test_gpu_cac_policy.py prints them), worst |device - mirror| / bound:
    k_cac_act: mu 0.16, sd 0.03, v 0.03, mean action 0.09, sampled action 0.24; fused kernel: scaled action 0.19
(observed only).  Recorded oracle figures: ORACLE_ERR below.

Where a bound is below half an ulp of the mirror's float32 value the device must return that float32 (exact32).
"""
import numpy as np

H = 256
P = 2 * H + 3 * (H + 1)                                 # 1283
W1, B1, WMU, BMU, WSTD, BSTD, WV, BV = 0, H, 2 * H, 3 * H, 3 * H + 1, 4 * H + 1, 4 * H + 2, 5 * H + 2
U = 2.0 ** -24
GAMMA12 = 12 * U / (1 - 12 * U)
FLOOR = 2.0 ** -126
HALF_SUBNORMAL = 2.0 ** -150
D53 = 2.0 ** -53
OUTPUTS = ("mu", "sd", "v", "mean", "action")

# The float32 oracle's largest error against the mirror over all items of all cases, in units of bounds(gam=U, K=1)
# (measured, rounded up by less than a quarter; asserted by test_cac_reference_host.py).  v has no intrinsic: its entry
# is the oracle's summation error in units of u S_v and is reported only.
ORACLE_ERR = {"mu": 0.75, "sd": 1.75, "v": 0.39, "mean": 1.45, "action": 1.9}
DEVICE_MARGIN = 4.0
K = {"mu": DEVICE_MARGIN * ORACLE_ERR["mu"], "sd": DEVICE_MARGIN * ORACLE_ERR["sd"],
     "a": DEVICE_MARGIN * max(ORACLE_ERR["mean"], ORACLE_ERR["action"])}
K_ONE = {"mu": 1.0, "sd": 1.0, "a": 1.0}

# What a scratch copy of the mirror may get wrong (tests/test_cac_reference_host.py: each must be seen).
SLIPS = ("tanh-3.9", "softplus-no-threshold", "softplus-threshold-15", "u1-for-1-u1", "sin-for-cos", "other-word-pair",
         "no-value-bias", "price-unrounded")


# ------------------------------------------------------------------------------------------------ the mirror
def softplus64(s, threshold=20.0):
    s = np.asarray(s, np.float64)
    with np.errstate(over="ignore"):
        return np.where(s > threshold, s, np.log1p(np.exp(np.minimum(s, threshold))))


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def heads64(w, price, slip=None):
    """Pre-activations m, s, v, mu = 4 tanh(m), sd = softplus(s) (torch's threshold 20) and the absolute sums S_m, S_s,
    S_v of the float32 parameters `w` ([P], or one vector per price [n, P]) at the float32-rounded prices [n]."""
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.shape[-1] == P, (w.dtype, w.shape)
    x = np.atleast_1d(np.asarray(price, np.float64))
    if slip != "price-unrounded":
        x = x.astype(np.float32).astype(np.float64)
    w = w.astype(np.float64)
    if w.ndim == 1:
        w = np.broadcast_to(w, (len(x), P))
    assert w.shape[0] == len(x), (w.shape, x.shape)
    h = np.maximum(w[:, W1:W1 + H] * x[:, None] + w[:, B1:B1 + H], 0.0)
    out = {"x": x}
    for name, ow, ob in (("m", WMU, BMU), ("s", WSTD, BSTD), ("v", WV, BV)):
        t = w[:, ow:ow + H] * h
        b = w[:, ob] * (0.0 if (slip == "no-value-bias" and name == "v") else 1.0)
        out[name] = t.sum(axis=1) + b
        out["S_" + name] = np.abs(t).sum(axis=1) + np.abs(w[:, ob])
    out["mu"] = (3.9 if slip == "tanh-3.9" else 4.0) * np.tanh(out["m"])
    thr = {"softplus-no-threshold": np.inf, "softplus-threshold-15": 15.0}.get(slip, 20.0)
    out["sd"] = softplus64(out["s"], thr)
    return out


def z64(u1, u2, slip=None):
    """The standard normal of two uniforms in [0, 1) and the bound E_z on |z32_dev - z64| (module docstring)."""
    u1 = np.asarray(u1, np.float64); u2 = np.asarray(u2, np.float64)
    r = np.sqrt(-2.0 * np.log(u1 if slip == "u1-for-1-u1" else 1.0 - u1))
    z = r * (np.sin if slip == "sin-for-cos" else np.cos)(2.0 * np.pi * u2)
    e_libm = D53 * (34.0 * r + 8.0 * np.abs(z))
    return z, U * (np.abs(z) + e_libm) + e_libm


def mean_action64(hd):
    return sigmoid64(hd["mu"])


def action64(hd, z):
    return sigmoid64(hd["mu"] + hd["sd"] * z)


def scaled64(a, lo, hi):
    """CAC.scale as the fused kernel forms it: float64 from the (float32) action, a product and a sum."""
    return np.asarray(a, np.float64) * (float(hi) - float(lo)) + float(lo)


def _spread(f, x, E, fx):
    return np.maximum(np.abs(f(x + E) - fx), np.abs(f(x - E) - fx))


def bounds(hd, z=None, E_z=None, gam=GAMMA12, Kd=None):
    """The derived bounds on |device - mirror| for mu, sd, v, the mean action and (with z, E_z) the sampled action."""
    Kd = K if Kd is None else Kd
    mu, sd = hd["mu"], hd["sd"]
    b = {}
    b["mu"] = _spread(lambda t: 4.0 * np.tanh(t), hd["m"], gam * hd["S_m"], mu) + Kd["mu"] * U * np.abs(mu) + FLOOR
    b["sd"] = _spread(softplus64, hd["s"], gam * hd["S_s"], sd) + Kd["sd"] * U * sd + FLOOR
    b["v"] = gam * hd["S_v"] + FLOOR

    def act(x, E_x):
        a = sigmoid64(x)
        return _spread(sigmoid64, x, E_x, a) + Kd["a"] * np.minimum(U * a, sigmoid64(-x)) + FLOOR

    b["mean"] = act(mu, b["mu"])
    if z is not None:
        az = np.abs(z) + E_z
        e_prod = b["sd"] * az + sd * E_z + U * (sd + b["sd"]) * az + FLOOR
        x = mu + sd * z
        b["action"] = act(x, (b["mu"] + e_prod) * (1.0 + U) + U * np.abs(x))
    return b


def units(hd, z=None, E_z=None):
    """The yardstick of ORACLE_ERR: the bounds with one rounding on the pre-activation and K = 1."""
    return bounds(hd, z, E_z, gam=U, Kd=K_ONE)


def exact32(value, bound):
    """Where the bound pins the float32 result: (mask, float32 values).  Either the bound is below half an ulp of the
    mirror's float32 value, or value + (bound - floor) is below half the smallest subnormal (then 0 comes out, flushed
    or rounded)."""
    value = np.asarray(value, np.float64); bound = np.asarray(bound, np.float64)
    f = value.astype(np.float32)
    af = np.abs(f)
    half_ulp = 0.5 * np.minimum(np.spacing(af), af - np.nextafter(af, np.float32(0))).astype(np.float64)
    near = (bound < half_ulp) & (af >= np.float32(FLOOR))
    zero = np.abs(value) + (bound - FLOOR) < HALF_SUBNORMAL
    return near | zero, np.where(zero, np.float32(0), f).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the fused kernel's draws
def philox_counter(step, episode, game, pair):
    """Counter of the draw of agents 2 * pair and 2 * pair + 1 (thrl_device.h: step, episode, game_lo,
    game_hi & 0xFFFFFF | stream << 24; stream = pair) and the key words of `seed` are philox_key(seed)."""
    return [int(step), int(episode), int(game) & 0xFFFFFFFF, ((int(game) >> 32) & 0xFFFFFF) | (int(pair) << 24)]


def philox_key(seed):
    return [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]


def pair_draws(words, agent, slip=None):
    """(u1, u2) of `agent` from the four 32-bit words [..., 4] of its pair's draw: words 0, 1 for the even agent, 2, 3
    for the odd one, each times 2^-32."""
    words = np.asarray(words, np.float64)
    o = 2 * ((int(agent) & 1) ^ (1 if slip == "other-word-pair" else 0))
    return words[..., o] * 2.0 ** -32, words[..., o + 1] * 2.0 ** -32


def env_price(scaled, a=10.0, b=1.0):
    """NoisyPriceState.step without noise, in the device's order: Q = sum of (a / b) * scaled_i from 0, agent by agent;
    price = a - b Q, 0 unless positive.  scaled is [N, G]."""
    scaled = np.asarray(scaled, np.float64)
    ratio = float(a) / float(b)
    Q = np.zeros(scaled.shape[1])
    for i in range(scaled.shape[0]):
        Q = Q + ratio * scaled[i]
    p = float(a) - float(b) * Q
    return np.where(p > 0.0, p, 0.0)


# ------------------------------------------------------------------------------------------------ cases
ROWS = 8                                    # games (weight vectors) per random case
PLANTED_M = (0.0, 1e-4, -1e-4, 0.5, -0.5, 9.0, -9.0, 9.02, -9.02, 10.0, -10.0, 100.0, -100.0)
_F20 = np.float32(20.0)
# (15.5: where a threshold at 15 would show most; 100: expf overflows in float32 without the threshold; 800: exp does
# so in float64)
PLANTED_S = (-104.0, -90.0, -20.0, 0.0, 15.5, float(np.nextafter(_F20, np.float32(0))), 20.0,
             float(np.nextafter(_F20, np.float32(40))), 50.0, 100.0, 800.0)
PLANTED_V = (0.0, 1e-3, -1e-3, 1e3, -1e3)
KINK_X0 = 3.0                               # kink-planted: every hidden unit changes sign at this float32 price
RANDOM_CASES = ("init", "x8", "x40", "x8-neg", "x40-neg", "kink")
PLANTED_CASES = ("planted-m", "planted-s", "planted-v", "extremes", "sd0", "kink-planted")
N_RANDOM_DRAWS = 259


def case_names():
    return RANDOM_CASES + PLANTED_CASES


def host_init(n, rs):
    """Weights with the distribution of thrl_cac_init: fc1 ~ U(-1, 1), the heads ~ U(-1/16, 1/16)."""
    w = np.empty((n, P), np.float32)
    w[:, :2 * H] = rs.uniform(-1, 1, (n, 2 * H))
    w[:, 2 * H:] = rs.uniform(-1, 1, (n, P - 2 * H)) / 16.0
    return w


def scale_heads(w, factor):
    w = np.array(w, np.float32, copy=True)
    w[..., 2 * H:] *= np.float32(factor)
    return w


def negate_mu(w):
    w = np.array(w, np.float32, copy=True)
    w[..., WMU:BMU + 1] *= np.float32(-1)
    return w


def planted(w, m=0.0, s=0.0, v=0.0):
    """Head weights zero, the biases carry m, s, v: the pre-activations are exact whatever the price.  m, s, v are
    scalars or one value per row of w."""
    w = np.array(w, np.float32, copy=True)
    w[..., 2 * H:] = 0.0
    w[..., BMU] = np.asarray(m, np.float32); w[..., BSTD] = np.asarray(s, np.float32); w[..., BV] = np.asarray(v, np.float32)
    return w


def _seed(name):
    return 7000 + 13 * case_names().index(name)


def case(name):
    """The weight rows and prices of a case: dict(w float32 [n, P], price float64 [n])."""
    rs = np.random.RandomState(_seed(name))
    if name in RANDOM_CASES:
        w = host_init(ROWS, rs)
        price = rs.uniform(0.0, 10.0, ROWS)
        if name.startswith("x"):
            w = scale_heads(w, 40 if name.startswith("x40") else 8)
        if name.endswith("-neg"):
            w = negate_mu(w)
        if name == "kink":
            # the float64 price at which a hidden unit's w1 x + b1 changes sign (a unit whose kink lies in (0, 10))
            w = scale_heads(w, 8)
            for g in range(ROWS):
                k = -w[g, B1:B1 + H].astype(np.float64) / w[g, W1:W1 + H].astype(np.float64)
                ok = np.flatnonzero((k > 0.5) & (k < 9.5))
                price[g] = k[ok[g % len(ok)]]
        return {"w": w, "price": price}
    if name == "planted-m":
        n = len(PLANTED_M)
        return {"w": planted(host_init(n, rs), m=PLANTED_M, s=0.5, v=1.0), "price": rs.uniform(0, 10, n)}
    if name == "planted-s":
        n = len(PLANTED_S)
        return {"w": planted(host_init(n, rs), m=0.5, s=PLANTED_S, v=1.0), "price": rs.uniform(0, 10, n)}
    if name == "planted-v":
        n = len(PLANTED_V)
        return {"w": planted(host_init(n, rs), m=-0.5, s=-1.0, v=PLANTED_V), "price": rs.uniform(0, 10, n)}
    if name == "extremes":                  # mu = +-4 (tanh saturated), sd = 50: arguments to +-337 with z = +-6.66
        return {"w": planted(host_init(2, rs), m=(10.0, -10.0), s=50.0, v=0.0), "price": rs.uniform(0, 10, 2)}
    if name == "sd0":                       # sd underflows to 0: the action is sigmoid(mu) for every draw
        m = (0.0, 0.5, -0.5, 9.0, -9.0)
        return {"w": planted(host_init(len(m), rs), m=m, s=-104.0, v=0.0), "price": rs.uniform(0, 10, len(m))}
    if name == "kink-planted":
        # fc1.weight in {+-1/2, +-1} and fc1.bias = -weight * X0 exactly, so every unit is 0 at the float32 price X0; the
        # float64 prices X0 +- 4e-8 round to it (half an ulp of 3.0f is 1.2e-7).  Heads x 40 with zero biases: m = s = v = 0
        # exactly on the device, and 1e-6 away where the price is not rounded.
        w = scale_heads(host_init(2, rs), 40)
        w1 = rs.choice([-1.0, -0.5, 0.5, 1.0], (2, H)).astype(np.float32)
        w[:, W1:W1 + H] = w1; w[:, B1:B1 + H] = -w1 * np.float32(KINK_X0)
        w[:, BMU] = 0.0; w[:, BSTD] = 0.0; w[:, BV] = 0.0
        return {"w": w, "price": np.array([KINK_X0 + 4e-8, KINK_X0 - 4e-8])}
    raise KeyError(name)


def planted_draws():
    """The crossed edge draws and the ones that put the argument mu - 50 r of `extremes` into float32's subnormal range
    (u2 = 0.5, r in 1.7 .. 2.0: actions e^-89 .. e^-104) and its mirror image (u2 = 0)."""
    u1 = [0.0, 2.0 ** -32, 0.5, 1.0 - 2.0 ** -32]
    u2 = [0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -32]
    pairs = [(a, b) for a in u1 for b in u2]
    for r in (1.7, 1.82, 1.9, 2.0):
        q = np.floor((1.0 - np.exp(-0.5 * r * r)) * 2.0 ** 32) * 2.0 ** -32
        pairs += [(q, 0.5), (q, 0.0)]
    return np.array(pairs)


def items(name):
    """Every (weight row, price, draw) of a case: the rows crossed with planted_draws(), then N_RANDOM_DRAWS random
    pairs (multiples of 2^-32, as Philox gives them) dealt to the rows in turn.  dict(w [n, P], price, u1, u2 [n])."""
    c = case(name)
    n = len(c["price"])
    pd = planted_draws()
    rs = np.random.RandomState(_seed(name) + 1)
    rnd = rs.randint(0, 2 ** 32, (N_RANDOM_DRAWS, 2), dtype=np.uint64).astype(np.float64) * 2.0 ** -32
    row = np.concatenate([np.repeat(np.arange(n), len(pd)), np.arange(N_RANDOM_DRAWS) % n])
    d = np.concatenate([np.tile(pd, (n, 1)), rnd])
    return {"w": c["w"][row], "price": c["price"][row], "u1": d[:, 0], "u2": d[:, 1], "row": row}


def mirror(it, slip=None):
    """Everything the tests compare for the items `it`: the heads, z, the five outputs (OUTPUTS) and their bounds."""
    hd = heads64(it["w"], it["price"], slip)
    z, E_z = z64(it["u1"], it["u2"], slip)
    val = {"mu": hd["mu"], "sd": hd["sd"], "v": hd["v"], "mean": mean_action64(hd), "action": action64(hd, z)}
    return {"heads": hd, "z": z, "E_z": E_z, "value": val, "bound": bounds(hd, z, E_z), "unit": units(hd, z, E_z)}
