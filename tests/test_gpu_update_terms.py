"""Every term of the three network update kernels -- k_nn_reinforce_train<kPad, false> (Reinforce), <kPad, true>
(ActorCritic), k_cac_train (CAC) -- against tests/update_reference.py, the float64 mirror that differentiates the
losses by autograd, through ReinforceBatch / ActorCriticBatch / CACBatch.

Why these inputs.  tests/test_gpu_nn.py runs ActorCritic and CAC in one regime only: fc_v at its initial bias, advantage
about -90, the critic's gradient dominating, clip_grad_norm_ dividing everything by 500 to 9,000 -- there the entropy
term, its sign, and a gamma off in the fourth digit all land below that file's tolerance
(test_update_reference_host.py::test_old_inputs_do_not_see_the_entropy_term_of_actorcritic_and_cac).  The cases here
(update_reference.case) keep the value head consistent with the rewards, so that actor, critic and entropy terms are
of one size, in an unclipped regime (pre-clip norm 0.05 - 0.8: grad_out is the raw gradient, the coef = 1 branch) and a
clipped one (1.5 - 50), on every path of the kernels: A = 21 / 24 / 30 (row paddings; ActorCritic with 24 actions has no
free value column and takes the plain path), 41 distinct states (folded), continuous prices (ActorCritic: plain;
Reinforce: the one-state-per-transition fold at n = 1,000, plain at n = 1,300), CAC at n = 64 / 391 / 1,000 (strided
loops).  test_update_reference_host.py shows on the CPU that each term of each case, 10 % off, leaves the bound below
by a factor of 10: no test here is blind to its term.

The bound.  Per parameter block (fc1.weight, fc1.bias, each head's weight, each head's bias):
    max |g_dev - g64| <= 4 x E x max |g64_block|,
E the float32 numpy oracle's error against the mirror in the same measure, the largest over all cases, games and blocks
of the kernel, measured on the CPU (update_reference.ORACLE_ERR, asserted by the host test):
    Reinforce 1.9e-5, ActorCritic 8.5e-5, CAC 3.5e-5, the CAC case with saturated actions 5.5e-4
(the last one's error is float32's 1 - a2 at a = 1.0f, which no other case has).  The margin of 4 is for the device's
other summation order and float32 intrinsics.  Elements that are exactly zero in the mirror (dead units) are exactly
zero on the device.  No figure observed on the device enters a bound; each test prints what it observes.  Observed on
an MI355X, largest over all tests of this file, in the same measure: Reinforce 1.1e-5, ActorCritic 1.2e-4, CAC 4.8e-5,
saturated 7.1e-4; the entropy term by difference quotient 2.2e-6 / 2.7e-6 / 2.3e-5; Adam at most 0.30 of the allowance on
the moments and 0.46 on the step.

Not pinned here: a policy so peaked that a REPLAYED action has p(a) < float32's eps.  There torch's clamp inside log()
cuts that transition's gradient to zero while the oracle and the kernels keep G (p - onehot); sampled actions do not
reach it, and the cases keep p(a) > 8 eps (asserted by the host test).  The sensitivity condition holds for every
term of every case listed; none was dropped.
"""
import numpy as np
import pytest

import update_reference as UR

pytestmark = pytest.mark.gpu

ALL = UR.case_names()
UNCLIPPED = UR.case_names(regime="unclipped")
CLIPPED = UR.case_names(regime="clipped")


def _run(name, sweep=False, spread=1.0, entropy=None, step=0, m0=None, v0=None):
    """One train() of the case on the device: (case, grad_out, params, adam_m, adam_v) as numpy arrays [G, P]."""
    import torch
    from th_rl_amd import nn
    c = UR.case(name, sweep, spread, entropy)
    kw = dict(gamma=float(c["gamma"][0]), entropy=float(c["entropy"][0]), lr=UR.LR)
    if c["kernel"] == "reinforce":
        b = nn.ReinforceBatch(UR.G, actions=c["A"], **kw)
    elif c["kernel"] == "actorcritic":
        b = nn.ActorCriticBatch(UR.G, actions=c["A"], **kw)
    else:
        b = nn.CACBatch(UR.G, **kw)
    assert b.P == c["w"].shape[1]
    b.set_params(c["w"])
    if sweep:
        b.set_sweep(gamma=c["gamma"], entropy=c["entropy"])
    if m0 is not None:
        b.adam_m.copy_(torch.from_numpy(m0)); b.adam_v.copy_(torch.from_numpy(v0))
    b.step = step
    g = b.train(c["price"], c["action"], c["reward"], want_grad=True, next_price=c["nprice"])
    assert b.step == step + 1
    return c, g.cpu().numpy(), b.params.cpu().numpy(), b.adam_m.cpu().numpy(), b.adam_v.cpu().numpy()


def _check_gradient(name, c, g, mirrors, what=""):
    """Assertion 1: per block within the device bound of the mirror's clipped gradient, exact zeros where the mirror has them."""
    bound = UR.device_bound(name)
    worst = {}
    for k in range(UR.G):
        assert np.isfinite(g[k]).all()
        errs = UR.block_errors(g[k], mirrors[k].clipped, c["kernel"], c["A"])
        for b, v in errs.items():
            worst[b] = max(worst.get(b, 0.0), v)
        assert not np.any(g[k][mirrors[k].raw == 0.0]), (name, k, "a zero-gradient element is not zero on the device")
    print("%s%s: device vs mirror, max |dg| / max |g64_block| (bound %.3g): %s"
          % (name, what, bound, ", ".join("%s %.2g" % kv for kv in worst.items())))
    assert max(worst.values()) <= bound, (name, what, worst)
    return worst


@pytest.mark.parametrize("name", ALL)
def test_gradient_matches_mirror_per_block(name):
    """Scalar gamma / entropy arguments.  Clipped cases also: the norm of what the device wrote is the clipped norm."""
    c, g, _, _, _ = _run(name)
    ms = UR.case_mirror(name)
    _check_gradient(name, c, g, ms)
    lo, hi = UR.NORM_RANGE[c["regime"]]
    for k in range(UR.G):
        assert lo <= ms[k].norm <= hi
        if c["regime"] == "clipped":
            ndev = float(np.sqrt((g[k].astype(np.float64) ** 2).sum()))
            assert abs(ndev - 1.0) <= UR.device_bound(name) + 1e-6 / ms[k].norm, (name, k, ndev)


@pytest.mark.parametrize("name", ALL)
def test_per_game_sweep_takes_each_game_its_own_gamma_and_entropy(name):
    """set_sweep with another gamma and entropy coefficient in every game: game k matches the mirror at game k's values
    and is outside the bound of the mirror at game k + 1's values (either one alone)."""
    c, g, _, _, _ = _run(name, sweep=True)
    _check_gradient(name, c, g, UR.case_mirror(name, True), " (sweep)")
    for k in range(UR.G):
        kn = (k + 1) % UR.G
        for kw in (dict(gamma=c["gamma"][kn]), dict(entropy=c["entropy"][kn])):
            other = UR.mirror(c, k, **kw).clipped
            assert max(UR.block_errors(g[k], other, c["kernel"], c["A"]).values()) > UR.device_bound(name), (name, k, kw)


@pytest.mark.parametrize("name", UNCLIPPED)
def test_each_term_alone_in_the_unclipped_regime(name):
    """grad_out is the raw gradient here, linear in the entropy coefficient: the difference quotient of two runs is the
    entropy term alone (the mirror's, at coefficient 1, under the block bound).  At coefficient 0 (ActorCritic, CAC) the
    policy heads' blocks are the actor term alone, the value head's the critic term alone, fc1 their sum."""
    kernel = name.split("-")[0]
    e1, e2 = UR.QUOTIENT_ENTROPY[kernel]
    c, g1, _, _, _ = _run(name, entropy=e1)
    _, g2, _, _, _ = _run(name, entropy=e2)
    ent = UR.case_mirror(name, False, 1.0, 1.0, "entropy")
    bound = UR.device_bound(name)
    worst = {}
    for k in range(UR.G):
        q = (g2[k].astype(np.float64) - g1[k]) / (e2 - e1)
        for b, v in UR.block_errors(q, ent[k].raw, kernel, c["A"]).items():
            worst[b] = max(worst.get(b, 0.0), v)
    print("%s: entropy term by difference quotient vs mirror (bound %.3g): %s" % (name, bound, ", ".join("%s %.2g" % kv for kv in worst.items())))
    assert max(worst.values()) <= bound, (name, worst)
    if kernel == "reinforce":
        return
    assert e1 == 0.0
    actor = UR.case_mirror(name, False, 1.0, 0.0, "actor")
    critic = UR.case_mirror(name, False, 1.0, 0.0, "critic")
    blocks = UR.blocks(kernel, c["A"])
    worst = {}
    for k in range(UR.G):
        assert UR.mirror(c, k, entropy=0.0).norm <= 0.8
        for b, sl in blocks.items():
            ref = actor[k].raw[sl] + critic[k].raw[sl] if b in UR.FC1 else (critic[k].raw[sl] if b.startswith("fc_v") else actor[k].raw[sl])
            other = actor[k].raw[sl] if b.startswith("fc_v") else critic[k].raw[sl]
            if b not in UR.FC1:
                assert not other.any()          # the mirror: the critic does not reach the policy heads, nor the actor fc_v
            worst[b] = max(worst.get(b, 0.0), float(np.abs(g1[k][sl] - ref).max() / np.abs(ref).max()))
    print("%s: actor / critic terms by block at entropy 0 (bound %.3g): %s" % (name, bound, ", ".join("%s %.2g" % kv for kv in worst.items())))
    assert max(worst.values()) <= bound, (name, worst)


@pytest.mark.parametrize("name", CLIPPED)
def test_clip_keeps_the_direction_when_the_rewards_spread_grows(name):
    """The rewards' spread times 4 (CAC: 16), another pre-clip norm and coef: the device's clipped gradient keeps unit
    norm and matches the mirror's clipped gradient per block."""
    spread = UR.CLIP_SPREAD[name.split("-")[0]]
    c, g, _, _, _ = _run(name, spread=spread)
    ms = UR.case_mirror(name, False, spread)
    _check_gradient(name, c, g, ms, " (spread x %g)" % spread)
    for k in range(UR.G):
        assert 1.5 <= ms[k].norm
        ndev = float(np.sqrt((g[k].astype(np.float64) ** 2).sum()))
        assert abs(ndev - 1.0) <= UR.device_bound(name) + 1e-6 / ms[k].norm, (name, k, ndev)


def _check_adam(name, step, c, g, w1, m1, v1, m0, v0):
    """Assertion 5.  Adam from the device's OWN grad_out in float64 (update_reference.adam_step64), every element.
    The device's update is  m = 0.9f m0 + 0.1f g;  v = 0.999f v0 + 0.001f g g;  w -= (lr / bc1) * (m / (sqrt(v) / bc2s + 1e-8f))
    in float32 (u = 2^-24), bc1 = 1 - powf(0.9f, t), bc2s = sqrtf(1 - powf(0.999f, t)):
      m: two rounded constants, two products, one sum -- 5 u on |0.9 m0| + |0.1 g| (the terms may cancel, so the bound is on
         their magnitudes, not on the result); allowed 8 u.
      v: the same with g g (one more product), both terms positive; allowed 8 u relative.
      w - w0: m (5 u, amplified by at most (|0.9 m0| + |0.1 g|) / |m|, covered below by taking the step's bound on lr, the
         step being at most ~1.4 lr at these moments), v (6 u / 2 under the root), sqrtf, the division by bc2s, + 1e-8f, m / denom,
         lr / bc1, the product, and the final subtraction which rounds to u |w|: a dozen operations; allowed 16 u (|w| + lr).
      bc1, bc2s are NOT a few u off: 0.999f is 1.3e-8 above 0.999, t times that lands on the power and 1 - power magnifies
         it -- 108 u on bc2s at t = 1, 164 u at t = 2, 63 u at t = 1000 (measured on the CPU in float32,
         test_update_reference_host.py::test_float32_bias_corrections_measured; the 64 u per powf the test was planned
         with does not cover t = 1).  As a relative error of the step: allowed twice the measured figures."""
    u, lr = UR.U, UR.LR
    e1, e2 = UR.bias_correction_error32(step)
    worst = [0.0, 0.0, 0.0]
    for k in range(UR.G):
        w0 = c["w"][k].astype(np.float64)
        w64, m64, v64 = UR.adam_step64(w0, g[k], m0[k], v0[k], step, lr)
        dm = np.abs(m1[k] - m64) / (8 * u * (np.abs(0.9 * m0[k].astype(np.float64)) + np.abs(0.1 * g[k].astype(np.float64))) + 1e-45)
        dv = np.abs(v1[k] - v64) / (8 * u * v64)
        st = w64 - w0
        dw = np.abs((w1[k].astype(np.float64) - w0) - st) / (16 * u * (np.abs(w0) + lr) + 2 * (e1 + e2) * np.abs(st))
        assert np.isfinite(w1[k]).all() and np.isfinite(m1[k]).all() and np.isfinite(v1[k]).all()
        worst = [max(a, float(b.max())) for a, b in zip(worst, (dm, dv, dw))]
    print("%s step %d: Adam vs float64 from the device's gradient, largest error / allowance: m %.2f, v %.2f, w %.2f" % ((name, step) + tuple(worst)))
    assert max(worst) <= 1.0, (name, step, worst)


def _moments(P, seed):
    rs = np.random.RandomState(seed)
    m0 = (rs.uniform(-1, 1, (UR.G, P)) * 1e-2).astype(np.float32)
    v0 = (rs.uniform(0.5, 1.5, (UR.G, P)) * 1e-4).astype(np.float32)      # no element near a zero sqrt(v)
    return m0, v0


@pytest.mark.parametrize("step", [0, 1, 9, 999])
@pytest.mark.parametrize("name", ["reinforce-A21_cont-unclipped", "reinforce-A30_s41-clipped", "actorcritic-A21_s41-unclipped",
                                  "actorcritic-A24_s41-clipped", "cac-n391-unclipped", "cac-n1000-clipped"])
def test_adam_step_from_planted_moments(name, step):
    """Adam isolated from the gradient: planted moments, step counter 0 / 1 / 9 / 999, every element of m, v and w1 - w0
    against float64 (see _check_adam for the derived allowance)."""
    P = UR.case(name)["w"].shape[1]
    m0, v0 = _moments(P, 40 + step)
    c, g, w1, m1, v1 = _run(name, step=step, m0=m0, v0=v0)
    _check_gradient(name, c, g, UR.case_mirror(name))         # the planted state does not reach the gradient
    _check_adam(name, step, c, g, w1, m1, v1, m0, v0)


def test_cac_saturated_actions_gradient_and_adam_step():
    """A tenth of the actions exactly 0.0f and a tenth exactly 1.0f (what sigmoid_f returns for a large |mu + std z|):
    y = logit(5e-5 + (1 - 1e-4) a) = -+9.9, everything finite, gradient and one Adam step as everywhere."""
    name = "cac-n391-saturated"
    c = UR.case(name)
    assert (c["action"] == 0.0).mean() >= 0.1 and (c["action"] == 1.0).mean() >= 0.1
    m0, v0 = _moments(UR.CAC_P, 77)
    c, g, w1, m1, v1 = _run(name, step=9, m0=m0, v0=v0)
    for a in (g, w1, m1, v1):
        assert np.isfinite(a).all()
    _check_gradient(name, c, g, UR.case_mirror(name))
    _check_adam(name, 9, c, g, w1, m1, v1, m0, v0)
