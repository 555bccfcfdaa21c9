"""Float64 mirror of the three network updates (Reinforce, ActorCritic, CAC) by autograd -- TEST INFRASTRUCTURE ONLY.

The device kernels (th_rl_amd/csrc/thrl_nn.hip: k_nn_reinforce_train<kPad, AC>, thrl_cac.hip: k_cac_train) and the numpy
oracle (oracle/nn_oracle.py) both evaluate hand-derived gradients: row / column sums of the [N, N] advantage, running
sums over sorted states, five batch sums for CAC.  This module writes the three LOSSES as DESIGN.md section 5.3 and the
oracle's docstrings define them and lets torch autograd differentiate them in float64 on the CPU; the [N, N] tensors
are built explicitly (N <= 1,300: 14 MB).  None of the closed forms appears here, so an error in one of them, in the
device or in the oracle, shows as a difference.

Conventions (those of _gradients_float64 in tests/test_gpu_nn.py): the inputs are the float32 weights, and the prices,
rewards and actions cast to float32, all widened to float64; gamma and the entropy coefficient are rounded to float32
as the kernels' arguments are; the ReLU activation test is float32's (x * w1 + b1 > 0 in float32), so a pre-activation of
exactly zero cannot flip between mirror and device.

Every gradient function returns a Grad: the raw gradient (float64, the device's parameter order), its norm, and the
gradient after clip_grad_norm_(1.0), which is what the kernels write to grad_out.  `scale` multiplies single terms of
the loss ("actor", "critic", "entropy", and "coupling" = the gamma * v' inside the advantage); `term` keeps one of
"actor" / "critic" / "entropy" and drops the others.

The second half of the module holds the input cases shared by tests/test_update_reference_host.py (CPU: the mirror
against the oracle, the sensitivity condition) and tests/test_gpu_update_terms.py (device against the mirror).
"""
import collections
import functools

import numpy as np
import torch

H = 256
U = 2.0 ** -24
EPS32 = float(np.finfo(np.float32).eps)
CAC_P = 2 * H + 3 * (H + 1)
TERMS = ("actor", "critic", "entropy", "coupling")

Grad = collections.namedtuple("Grad", "raw norm clipped")


def n_params(kernel, A=0):
    if kernel == "cac":
        return CAC_P
    return 2 * H + A * H + A + (H + 1 if kernel == "actorcritic" else 0)


def blocks(kernel, A=0):
    """The parameter blocks of a kernel's vector: name -> slice, in the device's order."""
    if kernel == "cac":
        o = 2 * H
        return {"fc1.weight": slice(0, H), "fc1.bias": slice(H, o), "fc_mu.weight": slice(o, o + H),
                "fc_mu.bias": slice(o + H, o + H + 1), "fc_std.weight": slice(o + H + 1, o + 2 * H + 1),
                "fc_std.bias": slice(o + 2 * H + 1, o + 2 * H + 2), "fc_v.weight": slice(o + 2 * H + 2, o + 3 * H + 2),
                "fc_v.bias": slice(o + 3 * H + 2, o + 3 * H + 3)}
    Pp = 2 * H + A * H + A
    b = {"fc1.weight": slice(0, H), "fc1.bias": slice(H, 2 * H), "fc_pi.weight": slice(2 * H, 2 * H + A * H),
         "fc_pi.bias": slice(2 * H + A * H, Pp)}
    if kernel == "actorcritic":
        b["fc_v.weight"] = slice(Pp, Pp + H)
        b["fc_v.bias"] = slice(Pp + H, Pp + H + 1)
    return b


# the head blocks a term of the loss feeds; every term also reaches the shared fc1 through its head
HEADS = {
    "reinforce": {"actor": ("fc_pi.weight", "fc_pi.bias"), "entropy": ("fc_pi.weight", "fc_pi.bias")},
    "actorcritic": {"actor": ("fc_pi.weight", "fc_pi.bias"), "entropy": ("fc_pi.weight", "fc_pi.bias"),
                    "critic": ("fc_v.weight", "fc_v.bias"), "coupling": ("fc_v.weight", "fc_v.bias")},
    "cac": {"actor": ("fc_mu.weight", "fc_mu.bias", "fc_std.weight", "fc_std.bias"), "entropy": ("fc_std.weight", "fc_std.bias"),
            "critic": ("fc_v.weight", "fc_v.bias"), "coupling": ("fc_v.weight", "fc_v.bias")},
}
FC1 = ("fc1.weight", "fc1.bias")


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float64)))


def _coef(scale, term):
    c = {k: 1.0 for k in TERMS}
    if scale:
        assert set(scale) <= set(TERMS), scale
        c.update({k: float(v) for k, v in scale.items()})
    if term is not None:
        assert term in ("actor", "critic", "entropy"), term
        for k in ("actor", "critic", "entropy"):
            if k != term:
                c[k] = 0.0
    return c


def relu_mask32(w, price):
    """The float32 activation test [n, H] of fc1 on the float32-cast prices."""
    w = np.asarray(w, np.float32)
    x = _f32(price)
    return (x[:, None] * w[None, :H] + w[None, H:2 * H]) > np.float32(0)


def _hidden(wt, w32, price):
    """fc1 + ReLU [n, H] in float64 with float32's activation pattern."""
    x = _t(_f32(price))
    pre = x[:, None] * wt[None, :H] + wt[None, H:2 * H]
    return pre * torch.from_numpy(relu_mask32(w32, price)).to(torch.float64)


def _finish(wt, loss):
    loss.backward()
    raw = wt.grad.detach().numpy().copy()
    norm = float(np.sqrt((raw * raw).sum()))
    return Grad(raw, norm, raw * min(1.0, 1.0 / (norm + 1e-6)))


def _leaf(w, P):
    w32 = np.asarray(w)
    assert w32.dtype == np.float32 and w32.shape == (P,), (w32.dtype, w32.shape, P)
    return torch.tensor(w32.astype(np.float64), requires_grad=True), w32


def zscored_returns(reward, gamma):
    """Reinforce.train_net's returns: the serial recurrence G_n = r_n + gamma G_(n+1) over the whole buffer, z-scored with
    the unbiased standard deviation."""
    r = _f32(reward).astype(np.float64)
    g = float(np.float32(gamma))
    d = r.copy()
    for i in range(len(r) - 2, -1, -1):
        d[i] = r[i] + g * d[i + 1]
    return (d - d.mean()) / d.std(ddof=1)


def _policy(wt, w32, A, price):
    """p [n, A], log(clamp(p)) and the entropy H [n] of the categorical policy."""
    h = _hidden(wt, w32, price)
    W2 = wt[2 * H:2 * H + A * H].reshape(A, H)
    b2 = wt[2 * H + A * H:2 * H + A * H + A]
    p = torch.softmax(h @ W2.T + b2[None, :], dim=1)
    logp = torch.log(torch.clamp(p, EPS32, 1.0 - EPS32))
    return h, p, logp, -(p * logp).sum(dim=1)


def reinforce(w, A, price, action, reward, gamma, entropy, scale=None, term=None):
    """loss = -mean(log p(a) * G) + entropy * (-mean H),  G the z-scored discounted returns (a constant)."""
    c = _coef(scale, term)
    wt, w32 = _leaf(w, n_params("reinforce", A))
    _, p, logp, Hn = _policy(wt, w32, A, price)
    a = torch.from_numpy(np.asarray(action, np.int64))
    G = torch.from_numpy(zscored_returns(reward, gamma))
    lp_a = logp.gather(1, a[:, None])[:, 0]
    loss = -c["actor"] * (lp_a * G).mean() + c["entropy"] * float(np.float32(entropy)) * (-Hn.mean())
    return _finish(wt, loss)


def actorcritic(w, A, price, action, reward, nprice, gamma, entropy, scale=None, term=None):
    """v, v' [N, 1] against rewards [N]:  adv[i, j] = r_j + gamma v'_i - v_i  (v' not detached),
    loss = mean(adv^2) - mean(log p_j(a_j) * adv.detach()) + entropy * (-mean H)."""
    c = _coef(scale, term)
    wt, w32 = _leaf(w, n_params("actorcritic", A))
    Pp = n_params("reinforce", A)
    h, p, logp, Hn = _policy(wt, w32, A, price)
    hp = _hidden(wt, w32, nprice)
    wv, bv = wt[Pp:Pp + H], wt[Pp + H]
    v = (h @ wv + bv)[:, None]
    vp = (hp @ wv + bv)[:, None]
    r = _t(_f32(reward))
    adv = (r[None, :] + c["coupling"] * float(np.float32(gamma)) * vp) - v                 # [N, N]
    a = torch.from_numpy(np.asarray(action, np.int64))
    lp_a = logp.gather(1, a[:, None])[:, 0]
    loss = (c["critic"] * (adv ** 2).mean() - c["actor"] * (lp_a[None, :] * adv.detach()).mean()
            + c["entropy"] * float(np.float32(entropy)) * (-Hn.mean()))
    return _finish(wt, loss)


def cac_logit(action):
    """y = logit(5e-5 + (1 - 1e-4) a) of the float32 actions, in float64."""
    a2 = 5e-5 + (1.0 - 1e-4) * _f32(action).astype(np.float64)
    return np.log(a2 / (1.0 - a2))


def cac(w, price, action, reward, nprice, gamma, entropy, scale=None, term=None):
    """mu = 4 tanh(fc_mu h), std = softplus(fc_std h), v = fc_v h, all [N, 1] against rewards / actions [N]:
    loss = mean_ij(adv^2 - log N(y_j; mu_i, std_i) * adv.detach()) + entropy * (-mean_i H_i),  H = 1/2 + log(2 pi)/2 + log std."""
    c = _coef(scale, term)
    wt, w32 = _leaf(w, CAC_P)
    b = blocks("cac")
    h = _hidden(wt, w32, price)
    hp = _hidden(wt, w32, nprice)
    head = lambda hh, name: hh @ wt[b["fc_%s.weight" % name]] + wt[b["fc_%s.bias" % name]][0]
    mu = 4.0 * torch.tanh(head(h, "mu"))[:, None]
    std = torch.nn.functional.softplus(head(h, "std"))[:, None]
    v = head(h, "v")[:, None]
    vp = head(hp, "v")[:, None]
    r = _t(_f32(reward))
    y = torch.from_numpy(cac_logit(action))
    adv = (r[None, :] + c["coupling"] * float(np.float32(gamma)) * vp) - v                 # [N, N]
    logprob = -((y[None, :] - mu) ** 2) / (2.0 * std ** 2) - torch.log(std) - 0.5 * float(np.log(2.0 * np.pi))
    Hn = 0.5 + 0.5 * float(np.log(2.0 * np.pi)) + torch.log(std[:, 0])
    loss = (c["critic"] * (adv ** 2).mean() - c["actor"] * (logprob * adv.detach()).mean()
            + c["entropy"] * float(np.float32(entropy)) * (-Hn.mean()))
    return _finish(wt, loss)


def adam_step64(w, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update number step + 1 in float64 (the bias corrections from Python floats, as torch takes them):
    returns (w, m, v) after it."""
    w, g, m, v = [np.asarray(a, np.float64) for a in (w, g, m, v)]
    t = int(step) + 1
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    return w - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps)), m, v


def bias_correction_error32(step):
    """Relative errors of float32's  1 - 0.9f^t  and  sqrt(1 - 0.999f^t),  t = step + 1, against the exact values, with
    numpy's float32 power standing for the device's powf.  The constants are rounded to float32 BEFORE the power is taken
    (0.999f = 0.999 (1 + 1.3e-8)): t times that lands on the power, and the subtraction from 1 magnifies it."""
    t = np.float32(int(step) + 1)
    one = np.float32(1)
    bc1 = float(one - np.power(np.float32(0.9), t))
    bc2s = float(np.sqrt(one - np.power(np.float32(0.999), t)))
    e1, e2 = 1.0 - 0.9 ** float(t), np.sqrt(1.0 - 0.999 ** float(t))
    return abs(bc1 - e1) / e1, abs(bc2s - e2) / e2


def block_errors(g, g64, kernel, A=0):
    """max |g - g64| / max |g64| per parameter block: name -> float (a block whose mirror gradient is all zero: 0.0 if g is
    zero there too, else inf)."""
    g = np.asarray(g, np.float64); g64 = np.asarray(g64, np.float64)
    out = {}
    for name, sl in blocks(kernel, A).items():
        top = np.abs(g64[sl]).max()
        d = np.abs(g[sl] - g64[sl]).max()
        out[name] = float(d / top) if top > 0 else (0.0 if d == 0 else float("inf"))
    return out


def outside(g, g64, bound, kernel, A=0, factor=1.0):
    """Per block, the share of elements with |g - g64| > factor * bound * max |g64_block|."""
    g = np.asarray(g, np.float64); g64 = np.asarray(g64, np.float64)
    out = {}
    for name, sl in blocks(kernel, A).items():
        top = np.abs(g64[sl]).max()
        out[name] = float((np.abs(g[sl] - g64[sl]) > factor * bound * top).mean())
    return out


# ------------------------------------------------------------------------------------------------ bounds
# The float32 numpy oracle against this mirror, measured on the CPU over every case below (all games, both `explicit`
# settings): the largest  max |g_oracle - g64| / max |g64_block|  of any parameter block, per kernel.  Asserted (and
# printed per block) by tests/test_update_reference_host.py::test_oracle_error_is_what_is_recorded.  The device, which
# sums in another order and uses float32 intrinsics where the oracle uses numpy's, is held to DEVICE_MARGIN times that.
# The saturated CAC case has a figure of its own: float32's 1 - a2 at a = 1.0f (a2 = 0.99995 +- 6e-8, so the logit is
# 1.2e-3 off) is an error source of that case alone, and it would loosen the bound of every other CAC case twentyfold.
ORACLE_ERR = {"reinforce": 1.9e-5, "actorcritic": 8.5e-5, "cac": 3.5e-5, "cac-saturated": 5.5e-4}
DEVICE_MARGIN = 4.0


def bound_key(name):
    """The ORACLE_ERR entry of a case (or kernel) name."""
    kernel = name.split("-")[0]
    return "cac-saturated" if name.endswith("saturated") else kernel


def device_bound(name):
    return DEVICE_MARGIN * ORACLE_ERR[bound_key(name)]


# ------------------------------------------------------------------------------------------------ cases
G = 4
LR = 2e-4
# name -> (kernel, A, distinct states (0: continuous prices), n, regime)
PATHS = {
    "reinforce": [("A21_s41", 21, 41, 1000), ("A24_s41", 24, 41, 391), ("A30_s41", 30, 41, 391), ("A21_cont", 21, 0, 1000),
                  ("A21_cont1300", 21, 0, 1300)],
    "actorcritic": [("A21_s41", 21, 41, 1000), ("A24_s41", 24, 41, 391), ("A30_s41", 30, 41, 391), ("A21_cont", 21, 0, 1000)],
    "cac": [("n64", 0, 0, 64), ("n391", 0, 0, 391), ("n1000", 0, 0, 1000)],
}
REGIMES = ("unclipped", "clipped")
NORM_RANGE = {"unclipped": (0.05, 0.8), "clipped": (1.5, 50.0)}
# the clip test: the rewards' spread times this still gives a pre-clip norm in the clipped range (CAC's norm is not
# monotonic in the spread: the advantage's mean and its covariance with the actions pull against each other)
CLIP_SPREAD = {"reinforce": 4.0, "actorcritic": 4.0, "cac": 16.0}
# the two entropy coefficients of the difference quotient (g(e2) - g(e1)) / (e2 - e1) in the unclipped regime: as far
# apart as keeps the norm below 0.8, so that the quotient is not a difference of nearly equal numbers
QUOTIENT_ENTROPY = {"reinforce": (0.0, 0.15), "actorcritic": (0.0, 0.03), "cac": (0.0, 0.025)}


def case_names(kernel=None, regime=None):
    out = []
    for k in PATHS if kernel is None else (kernel,):
        for path, _, _, _ in PATHS[k]:
            for r in REGIMES if regime is None else (regime,):
                out.append("%s-%s-%s" % (k, path, r))
    if kernel in (None, "cac") and regime in (None, "unclipped"):
        out.append("cac-n391-saturated")
    return out


def _host_init(kernel, A, rs):
    """Weights with the distribution of the device's init: fc1 ~ U(-1, 1), the heads ~ U(-1/16, 1/16)."""
    P = n_params(kernel, A)
    w = np.empty((G, P), np.float32)
    w[:, :2 * H] = rs.uniform(-1, 1, (G, 2 * H))
    w[:, 2 * H:] = rs.uniform(-1, 1, (G, P - 2 * H)) / 16.0
    return w


SWEEP_ENT = np.array([1.0, 0.8, 0.6, 1.2])      # a sweep's entropy coefficients, as multiples of the case's
ENT_R_CLIPPED = 0.08
# norm of the actor and critic terms together (ActorCritic, CAC); the entropy term comes on top
TARGET_NORM = {"unclipped": 0.3, "clipped": 1.5}


def _build(name, sweep, spread, f):
    kernel, path, regime = name.split("-")
    _, A, states, n = [p for p in PATHS[kernel] if p[0] == path][0]
    saturated = regime == "saturated"
    if saturated:
        regime = "unclipped"
    seed = sorted(PATHS).index(kernel) * 1000 + [p[0] for p in PATHS[kernel]].index(path) * 10 + REGIMES.index(regime)
    rs = np.random.RandomState(7000 + seed)
    w = _host_init(kernel, A, rs)
    if states:
        grid = np.sort(rs.choice(np.arange(500, 6500), states, replace=False)) / 1000.0
        idx = rs.randint(0, states, (n + 1, G)); idx[:states, :] = np.arange(states)[:, None]
        pr = grid[idx]
    else:
        pr = rs.uniform(0.5, 6.5, (n + 1, G))
    price, nprice = pr[:-1], pr[1:]
    u_act = rs.uniform(0, 1, (n, G))
    u_rew = rs.uniform(-1, 1, (n, G))
    f = np.asarray(f, np.float64)
    if kernel == "reinforce":
        gamma = np.array([0.93, 0.80, 0.60, 0.35]) if sweep else np.full(G, 0.93)
        ent = (0.12 if regime == "unclipped" else ENT_R_CLIPPED) * (SWEEP_ENT if sweep else np.ones(G))
        if regime == "clipped":
            w[:, 2 * H:] *= np.float32(0.4)
            w[:, :2 * H] *= np.float32(4.0)
        else:
            w[:, :2 * H] *= np.float32(0.5)
        action = np.minimum((u_act * A).astype(np.int64), A - 1)
        reward = 10.0 + 5.0 * spread * u_rew
    elif kernel == "actorcritic":
        gamma = np.array([0.90, 0.86, 0.80, 0.75]) if sweep else np.full(G, 0.9)
        e0 = 0.025 if regime == "unclipped" else 0.15
        ent = e0 * (SWEEP_ENT if sweep else np.ones(G))
        Pp = n_params("reinforce", A)
        w[:, Pp:Pp + H] *= (0.02 * f).astype(np.float32)[:, None]
        w[:, Pp + H] = ((1.0 - 0.025 * f) / (1.0 - gamma)).astype(np.float32)
        action = np.minimum((u_act * A).astype(np.int64), A - 1)
        reward = 1.0 + 0.25 * spread * f[None, :] * u_rew
    else:
        gamma = np.array([0.95, 0.92, 0.90, 0.85]) if sweep else np.full(G, 0.95)
        e0 = 0.012 if regime == "unclipped" else 0.06
        ent = e0 * (SWEEP_ENT if sweep else np.ones(G))
        b = blocks("cac")
        w[:, b["fc_v.weight"]] *= (0.004 * f).astype(np.float32)[:, None]
        w[:, b["fc_mu.weight"]] *= np.float32(0.25)
        w[:, b["fc_std.weight"]] *= np.float32(0.25)
        w[:, b["fc_v.bias"]] = ((0.01 - 0.004 * f) / (1.0 - gamma)).astype(np.float32)[:, None]
        action = (0.01 + 0.98 * u_act).astype(np.float32)
        if saturated:                       # sigmoid_f returns exactly 0.0f / 1.0f for a large |mu + std z|
            action[0::9] = 0.0
            action[4::9] = 1.0
        reward = 0.01 + 0.02 * spread * f[None, :] * u_rew
    return dict(name=name, kernel=kernel, A=A, n=n, regime=regime, w=w, price=price, nprice=nprice, action=action,
                reward=reward, gamma=gamma, entropy=ent)


@functools.lru_cache(maxsize=None)
def _advantage_scale(name, sweep):
    """The factor per game that brings the norm of the actor and critic terms to TARGET_NORM (see case)."""
    if name.startswith("reinforce"):
        return (1.0,) * G
    c = _build(name, sweep, 1.0, np.ones(G))
    return tuple(TARGET_NORM[c["regime"]] / mirror(c, k, entropy=0.0).norm for k in range(G))


@functools.lru_cache(maxsize=None)
def case(name, sweep=False, spread=1.0, entropy=None):
    """The inputs of a case: dict(kernel, A, n, w [G, P] float32, price / nprice / reward [n, G] float64, action [n, G],
    gamma [G], entropy [G]).  sweep: another gamma and entropy coefficient in every game (set_sweep), else one value.
    spread: the rewards' spread around their mean times this.  entropy: the entropy coefficient in place of the case's.

    Weights as the device's init draws them, then:
    Reinforce: rewards U(5, 15) as everywhere in the suite; unclipped: fc1 halved, entropy coefficient 0.12 (norms 0.25 -
    0.75); clipped: fc1 times 4, fc_pi times 0.4, coefficient 0.08 (norms 1.8 - 8; a larger hidden layer, not a more
    peaked policy, and an entropy term large enough that scaling the actor term turns the clipped gradient).  fc_pi is
    NOT scaled up to peaked policies: with uniformly drawn actions that puts
    p(a) below float32's eps, where the clamp inside log() is active and autograd's gradient of that transition is zero,
    while the oracle and the kernels keep G (p - onehot).  Sampled actions have p(a) >= eps, so the cases keep it so (the
    host test asserts it).
    ActorCritic and CAC: a value head consistent with the rewards, which keeps the advantage at the rewards' spread
    instead of the -90 of the initial fc_v.bias of 1000: rewards U(m - f s, m + f s), fc_v.bias = (m - f d) / (1 - gamma)
    (the head undershoots by d, so that the gradient of fc_v.bias is not a cancelled sum), fc_v.weight at 2 % (CAC 0.4 %)
    of its initial scale times f (not zero: the critic reaches fc1 through it).  ActorCritic m = 1, s = 0.25, d = 0.025;
    CAC m = 0.01, s = 0.02, d = 0.004, fc_mu / fc_std weights at a quarter of their initial scale.  (m is small so that
    float32's rounding of v near m / (1 - gamma) stays well below the advantage: with m = 10 it alone put the oracle's
    error at 5e-4 and more, and the sensitivity condition out of reach.)  The advantage is
    linear in f, and so are the actor and critic terms of the gradient: f is set per game so that their norm is
    TARGET_NORM of the regime.  The entropy term adds to that: coefficient 0.025 (ActorCritic) / 0.012 (CAC) unclipped,
    0.15 / 0.06 clipped, where it is the larger part of the gradient but not all of it (were it all, scaling it would leave the
    clipped gradient's direction where it was)."""
    c = _build(name, bool(sweep), float(spread), np.array(_advantage_scale(name, bool(sweep))))
    if entropy is not None:
        c["entropy"] = np.full(G, float(entropy))
    return c


def mirror(c, k, gamma=None, entropy=None, scale=None, term=None):
    """The mirror's Grad of game k of case dict c (gamma / entropy: in place of the game's own)."""
    gamma = c["gamma"][k] if gamma is None else gamma
    entropy = c["entropy"][k] if entropy is None else entropy
    kw = dict(scale=scale, term=term)
    if c["kernel"] == "reinforce":
        return reinforce(c["w"][k], c["A"], c["price"][:, k], c["action"][:, k], c["reward"][:, k], gamma, entropy, **kw)
    if c["kernel"] == "actorcritic":
        return actorcritic(c["w"][k], c["A"], c["price"][:, k], c["action"][:, k], c["reward"][:, k], c["nprice"][:, k],
                           gamma, entropy, **kw)
    return cac(c["w"][k], c["price"][:, k], c["action"][:, k], c["reward"][:, k], c["nprice"][:, k], gamma, entropy, **kw)


@functools.lru_cache(maxsize=None)
def case_mirror(name, sweep=False, spread=1.0, entropy=None, term=None):
    """The mirror's Grad of every game of a case (computed once, shared by the tests; do not modify)."""
    c = case(name, sweep, spread, entropy)
    return tuple(mirror(c, k, term=term) for k in range(G))
