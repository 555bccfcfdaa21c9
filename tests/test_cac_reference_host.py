"""tests/cac_reference.py (the float64 mirror of CAC's heads and sampling) on the CPU:

a. against a float64 torch transcription of the reference's CAC.pi() / v() / sample_action arithmetic (agents.py:362-383:
   Linear -> relu -> three heads, 4 * tanh, softplus, sigmoid of mu + std * eps) on every case, to 1e-12;
b. the float32 numpy oracle (oracle/nn_oracle.py) lies inside every bound on every item of every case, and its largest
   error in the mirror's units is what the module records (CR.ORACLE_ERR; the K's of the bounds are 4 x that);
c. the sensitivity condition: each slip of CR.SLIPS, made in the mirror, leaves the DEVICE bound around the unchanged
   mirror by a factor of at least 10 on at least one item of a listed case -- so a kernel with that slip cannot pass
   tests/test_gpu_cac_policy.py.  One slip cannot meet it and is held to (a) instead, see
   test_softplus_threshold_at_15_is_below_float32_resolution;
d. the cases reach the regimes they exist for."""
import numpy as np
import pytest

import cac_reference as CR
from oracle import nn_oracle as NN

CASES = CR.case_names()
_CACHE = {}


def _items(name):
    if name not in _CACHE:
        it = CR.items(name)
        with np.errstate(all="ignore"):
            _CACHE[name] = (it, CR.mirror(it))
    return _CACHE[name]


def _rows(it):
    for r in np.unique(it["row"]):
        idx = np.flatnonzero(it["row"] == r)
        yield idx, it["w"][idx[0]]


# ------------------------------------------------------------------------------------------------ a. mirror vs torch
def _torch_outputs(w, x32, z):
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    H = CR.H
    x = t(x32).reshape(-1, 1)
    h = torch.relu(F.linear(x, t(w[CR.W1:CR.W1 + H]).reshape(H, 1), t(w[CR.B1:CR.B1 + H])))
    head = lambda ow, ob: F.linear(h, t(w[ow:ow + H]).reshape(1, H), t(w[ob:ob + 1]))
    mu = 4.0 * torch.tanh(head(CR.WMU, CR.BMU))
    std = F.softplus(head(CR.WSTD, CR.BSTD))
    v = head(CR.WV, CR.BV)
    action = torch.sigmoid(mu + std * t(z).reshape(-1, 1))
    return {"mu": mu, "sd": std, "v": v, "mean": torch.sigmoid(mu), "action": action}


@pytest.mark.parametrize("name", CASES)
def test_mirror_equals_float64_torch_transcription(name):
    it, mr = _items(name)
    for idx, w in _rows(it):
        x32 = it["price"][idx].astype(np.float32)
        ref = _torch_outputs(w, x32, mr["z"][idx])
        for k in CR.OUTPUTS:
            np.testing.assert_allclose(mr["value"][k][idx], ref[k].numpy()[:, 0], rtol=1e-12, atol=1e-12, err_msg="%s %s" % (name, k))


# ------------------------------------------------------------------------------------------------ b. the float32 oracle
def _oracle(it):
    out = {k: np.empty(len(it["price"])) for k in CR.OUTPUTS}
    with np.errstate(all="ignore"):
        for idx, w in _rows(it):
            pr = it["price"][idx]
            mu, sd, v, _ = NN.cac_forward(w, pr)
            out["mu"][idx], out["sd"][idx], out["v"][idx] = mu, sd, v
            out["mean"][idx] = NN.cac_mean_action(w, pr)
            out["action"][idx] = NN.cac_sample_action(w, pr, it["u1"][idx], it["u2"][idx])
    return out


def _oracle_ratios(name, against):
    it, mr = _items(name)
    o = _oracle(it)
    assert all(np.isfinite(o[k]).all() for k in CR.OUTPUTS), name
    return {k: float((np.abs(o[k] - mr["value"][k]) / mr[against][k]).max()) for k in CR.OUTPUTS}


@pytest.mark.parametrize("name", CASES)
def test_oracle_inside_every_bound(name):
    r = _oracle_ratios(name, "bound")
    print("%s: oracle vs mirror, largest |d| / bound: %s" % (name, ", ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r
    it, mr = _items(name)
    o = _oracle(it)
    for k in CR.OUTPUTS:                     # ... and equals the pinned float32 value wherever the bound pins one
        mask, f = CR.exact32(mr["value"][k], mr["bound"][k])
        assert np.array_equal(o[k][mask].astype(np.float32), f[mask]), (name, k)


def test_oracle_error_is_what_is_recorded():
    """CR.ORACLE_ERR is the measurement, rounded up by less than a quarter: the K's are derived from the oracle's own
    error, not chosen."""
    worst = {k: 0.0 for k in CR.OUTPUTS}
    for name in CASES:
        for k, v in _oracle_ratios(name, "unit").items():
            worst[k] = max(worst[k], v)
    print("oracle vs mirror in units of u S |f'| + u |value| + 2^-126: %s (recorded %s)"
          % (", ".join("%s %.3g" % kv for kv in worst.items()), CR.ORACLE_ERR))
    for k in CR.OUTPUTS:
        assert 0.8 * CR.ORACLE_ERR[k] <= worst[k] <= CR.ORACLE_ERR[k], (k, worst[k])
    assert CR.K == {"mu": 4 * CR.ORACLE_ERR["mu"], "sd": 4 * CR.ORACLE_ERR["sd"],
                    "a": 4 * max(CR.ORACLE_ERR["mean"], CR.ORACLE_ERR["action"])}
    assert CR.ORACLE_ERR["v"] < 12.0          # gamma_12 S_v holds the oracle's own summation


# ------------------------------------------------------------------------------------------------ c. sensitivity
# slip -> the outputs it must move, and the listed cases on which it has to show
SEEN_ON = {
    "tanh-3.9": (("mu", "mean", "action"), ("x8", "x40", "planted-m", "extremes")),
    "softplus-no-threshold": (("sd",), ("planted-s",)),
    "u1-for-1-u1": (("action",), ("init", "x8", "planted-s")),
    "sin-for-cos": (("action",), ("init", "x8", "planted-s")),
    "other-word-pair": (("action",), ("init", "x8")),
    "no-value-bias": (("v",), ("planted-v", "init")),
    "price-unrounded": (("mu", "v"), ("kink-planted",)),
}


def _factor(name, slip, outputs):
    """The largest |slipped mirror - mirror| / bound over the items of a case and the given outputs."""
    it, mr = _items(name)
    with np.errstate(all="ignore"):
        if slip == "other-word-pair":
            # the draws as four Philox words per item: the agent's own pair is (u1, u2), the other pair is random
            rs = np.random.RandomState(5)
            words = np.stack([it["u1"] * 2.0 ** 32, it["u2"] * 2.0 ** 32,
                              rs.randint(0, 2 ** 32, len(it["u1"])).astype(np.float64),
                              rs.randint(0, 2 ** 32, len(it["u1"])).astype(np.float64)], axis=1)
            assert np.array_equal(CR.pair_draws(words, 0), (it["u1"], it["u2"]))
            assert np.array_equal(CR.pair_draws(words[:, [2, 3, 0, 1]], 1), (it["u1"], it["u2"]))
            u1, u2 = CR.pair_draws(words, 0, slip)
            val = CR.mirror(dict(it, u1=u1, u2=u2))["value"]
        else:
            val = CR.mirror(it, slip)["value"]
        d = [np.abs(val[k] - mr["value"][k]) / mr["bound"][k] for k in outputs]
    return float(np.nanmax(np.where(np.isnan(np.stack(d)), 0.0, np.stack(d))))


@pytest.mark.parametrize("slip", sorted(SEEN_ON))
def test_every_slip_leaves_the_device_bound(slip):
    outputs, names = SEEN_ON[slip]
    f = {n: _factor(n, slip, outputs) for n in names}
    print("%s: largest |slipped - mirror| / bound: %s" % (slip, ", ".join("%s %.3g" % kv for kv in f.items())))
    assert max(f.values()) >= 10.0, (slip, f)
    for n in names:                           # ... and the mirror itself, fed through the bound, passes
        assert _factor(n, None, outputs) == 0.0


def test_every_slip_is_listed():
    assert set(SEEN_ON) | {"softplus-threshold-15"} == set(CR.SLIPS)


def test_softplus_threshold_at_15_is_below_float32_resolution():
    """softplus with its threshold at 15 returns s where the function is s + e^-s: at most e^-15 = 3.1e-7 off on a value
    of at least 15, a third of an ulp of float32 there (ulp 9.5e-7) and below u |sd|, the least any float32 result can
    be held to.  No bound on a float32 kernel can see it, whatever the case, so the factor of 10 is out of reach by
    arithmetic; its largest ratio to the device bound over all cases is asserted to be below 1 (the fact), and the slip
    is seen where it can be: against the float64 torch transcription, a factor of 10 beyond that test's 1e-12 (as is
    the threshold removed, at the float32 above 20)."""
    worst = max(_factor(n, "softplus-threshold-15", ("sd", "action")) for n in CASES)
    print("threshold at 15: largest |slipped - mirror| / device bound %.3g" % worst)
    assert worst < 1.0
    it, mr = _items("planted-s")
    for slip in ("softplus-threshold-15", "softplus-no-threshold"):
        seen = 0.0
        with np.errstate(all="ignore"):
            sl = CR.mirror(it, slip)["value"]["sd"]
        for idx, w in _rows(it):
            ref = _torch_outputs(w, it["price"][idx].astype(np.float32), mr["z"][idx])["sd"].numpy()[:, 0]
            seen = max(seen, float(np.max(np.abs(sl[idx] - ref) / (1e-12 + 1e-12 * np.abs(ref)))))
        assert seen >= 10.0, (slip, seen)


# ------------------------------------------------------------------------------------------------ d. regimes
def test_cases_reach_their_regimes():
    hd = {n: _items(n)[1]["heads"] for n in CASES}
    val = {n: _items(n)[1]["value"] for n in CASES}
    assert np.abs(hd["init"]["m"]).max() < 2.5 and np.abs(hd["init"]["s"]).max() < 2.5       # the old tests' regime
    for n in ("x40", "x40-neg"):
        assert np.abs(hd[n]["m"]).max() > 9.02, (n, np.abs(hd[n]["m"]).max())                # tanhf saturated
    s40 = np.concatenate([hd["x40"]["s"], hd["x40-neg"]["s"]])
    assert s40.max() > 20.0 and s40.min() < -50.0, (s40.min(), s40.max())
    for a, b in (("x8", "x8-neg"), ("x40", "x40-neg")):
        m = np.concatenate([hd[a]["m"], hd[b]["m"]])
        assert m.min() < -2.0 and m.max() > 2.0                                              # both signs of fc_mu
    # planted pre-activations are exact, the kink prices sit on a kink
    assert np.array_equal(np.unique(hd["planted-m"]["m"]), np.unique(np.float32(CR.PLANTED_M).astype(np.float64)))
    assert np.array_equal(np.unique(hd["planted-s"]["s"]), np.unique(np.float32(CR.PLANTED_S).astype(np.float64)))
    c = CR.case("kink")
    pre = c["w"][:, :CR.H].astype(np.float64) * c["price"][:, None] + c["w"][:, CR.H:2 * CR.H]
    assert (np.abs(pre).min(axis=1) < 1e-15).all()
    kp = hd["kink-planted"]
    assert np.all(kp["m"] == 0.0) and np.all(kp["S_m"] == 0.0) and np.all(kp["x"] == CR.KINK_X0)
    # argument extremes: the action is pinned to 1.0f, to 0, and lies in the subnormal range in between
    a = val["extremes"]["action"]
    mask, f = CR.exact32(a, _items("extremes")[1]["bound"]["action"])
    assert (mask & (f == np.float32(1.0))).sum() >= 4 and (mask & (f == 0) & (a > 0)).sum() >= 4
    assert ((a > 2.0 ** -149) & (a < 2.0 ** -126)).sum() >= 4
    z = _items("extremes")[1]["z"]
    assert z.max() > 6.66 and z.min() < -6.66
    # sd = 0: the sampled action is the mean action for every draw
    assert val["sd0"]["sd"].max() < 1e-45 and np.array_equal(val["sd0"]["action"], val["sd0"]["mean"])
