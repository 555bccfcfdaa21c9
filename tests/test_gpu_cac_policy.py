"""The forward side of the continuous agent CAC (cac_policy, softplus_f, sigmoid_f, box_muller_f of
th_rl_amd/csrc/thrl_cac.h) against the float64 mirror tests/cac_reference.py -- never against another device kernel:
k_cac_act through thrl_cac_act, and the same code with the weights in LDS in the fused episode kernel.  Random weights
at the initial scale and with the heads x 8 and x 40 (tanhf saturated, s above 20 and below -50), both signs of fc_mu,
prices on a hidden unit's kink, planted pre-activations, the edge draws of Philox crossed with all of them, arguments of
the sigmoid to +-337; 1, 5 and 259 games (four games per block: tails of one and three), output buffers pre-filled and
longer than G.  Each assertion is hard: every value within the derived bound, and equal to the float32 the bound pins
where it pins one.  The worst ratio to the bound seen per output is printed, never used."""
import numpy as np
import pytest

import cac_reference as CR

pytestmark = pytest.mark.gpu

GAMES = (1, 5, 259)
SENTINEL = -7.0
GUARD = 64
WORST = {}                      # output -> worst |device - mirror| / bound seen in this session
_MIRROR = {}


def _items(name):
    if name not in _MIRROR:
        it = CR.items(name)
        with np.errstate(all="ignore"):
            _MIRROR[name] = (it, CR.mirror(it))
    return _MIRROR[name]


class _Act:
    """thrl_cac_act on G games with every output buffer pre-filled and GUARD entries longer than G."""

    def __init__(self, G):
        from th_rl_amd.nn import CACBatch
        self.cb = CACBatch(G)
        self.G = G

    def __call__(self, w, price, u1=None, u2=None, heads=("mu", "sd", "v")):
        import torch
        cb, G = self.cb, self.G
        cb.set_params(w)
        with torch.cuda.device(cb.device):
            dev = lambda a: None if a is None else cb._dev(np.asarray(a, np.float64), torch.float64).reshape(G)
            d_price, d_u1, d_u2 = dev(price), dev(u1), dev(u2)
            buf = {k: torch.full((G + GUARD,), SENTINEL, dtype=torch.float32, device=cb.device)
                   for k in ("action",) + tuple(heads)}
            rc = cb.L.thrl_cac_act(G, cb._p(cb.params), cb._p(d_price), cb._p(d_u1), cb._p(d_u2), cb._p(buf["action"]),
                                   cb._p(buf.get("mu")), cb._p(buf.get("sd")), cb._p(buf.get("v")), cb._stream())
            assert rc == 0, rc
            out = {k: b.cpu().numpy() for k, b in buf.items()}
        for k, b in out.items():
            assert np.all(b[G:] == np.float32(SENTINEL)), "%s written past game G - 1" % k
            out[k] = b[:G]
        return out


def _run(act, it, sel):
    """The items `sel` in launches of act.G games (the last one filled up with the first item): the device's mu, sd, v,
    mean action (u1 = NULL) and sampled action per item."""
    G = act.G
    got = {k: np.empty(len(sel), np.float32) for k in CR.OUTPUTS}
    for c in range(0, len(sel), G):
        idx = sel[c:c + G]
        pad = np.concatenate([idx, np.full(G - len(idx), sel[0], idx.dtype)])
        mean = act(it["w"][pad], it["price"][pad])
        samp = act(it["w"][pad], it["price"][pad], it["u1"][pad], it["u2"][pad])
        for k in ("mu", "sd", "v"):
            assert np.array_equal(mean[k].view(np.uint32), samp[k].view(np.uint32)), k      # the heads do not see the draw
            got[k][c:c + len(idx)] = mean[k][:len(idx)]
        got["mean"][c:c + len(idx)] = mean["action"][:len(idx)]
        got["action"][c:c + len(idx)] = samp["action"][:len(idx)]
    return got


def _check(what, key, dev, value, bound, worst_key=None):
    assert np.isfinite(dev).all(), (what, key)
    ratio = np.abs(dev.astype(np.float64) - value) / bound
    wk = worst_key or key
    WORST[wk] = max(WORST.get(wk, 0.0), float(ratio.max()))
    assert ratio.max() <= 1.0, (what, key, float(ratio.max()), int(ratio.argmax()), float(dev[ratio.argmax()]),
                                float(value[ratio.argmax()]))
    mask, f = CR.exact32(value, bound)
    assert np.array_equal(dev[mask], f[mask]), (what, key, "pinned values", dev[mask][:4], f[mask][:4])


@pytest.mark.parametrize("name", CR.case_names())
def test_act_kernel_against_the_float64_mirror(name):
    it, mr = _items(name)
    n = len(it["price"])
    for G in GAMES:
        # every item at 259 games per launch; at 1 and 5 a spread of them (the arithmetic does not depend on G, the
        # grid's tail and the guards do)
        sel = np.arange(n) if G == 259 else np.arange(0, n, 97 if G == 1 else 19)
        got = _run(_Act(G), it, sel)
        for k in CR.OUTPUTS:
            _check("%s G=%d" % (name, G), k, got[k], mr["value"][k][sel], mr["bound"][k][sel])
        assert ((got["mean"] >= 0) & (got["mean"] <= 1) & (got["action"] >= 0) & (got["action"] <= 1)).all()
        if name == "sd0":
            # z is always finite: where sd came out as 0 the sampled action is the mean action, bit for bit
            flat = got["sd"] == 0
            assert flat.any()
            assert np.array_equal(got["action"][flat].view(np.uint32), got["mean"][flat].view(np.uint32))
    print("%s: worst |device - mirror| / bound so far: %s" % (name, {k: round(v, 4) for k, v in sorted(WORST.items())}))


@pytest.mark.parametrize("G", GAMES)
def test_absent_head_pointers_change_nothing(G):
    """mu_out / std_out / v_out all NULL, only v_out, only mu_out: the action is bit-identical to the call with all
    three, the buffers that are there hold what that call wrote, nothing is written past game G - 1."""
    it, _ = _items("x8")
    sel = np.arange(len(it["price"]))[-G:]                      # the random draws
    act = _Act(G)
    for u in (True, False):
        args = (it["w"][sel], it["price"][sel]) + ((it["u1"][sel], it["u2"][sel]) if u else ())
        full = act(*args)
        assert not np.any(full["action"] == np.float32(SENTINEL))
        for heads in ((), ("v",), ("mu",), ("sd",)):
            part = act(*args, heads=heads)
            assert sorted(part) == sorted(("action",) + heads)
            for k in part:
                assert np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32)), (G, u, heads, k)


# ------------------------------------------------------------------------------------------------ the fused kernel
Q_AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001, epsilon=0.5, eps_step=0.9995,
               action_range=[0.2, 0.4], min_memory=1)
RANGES = ([0.05, 0.25], [0.1, 0.3], [0.15, 0.35], [0.2, 0.4])
EPISODES = 3


def _cac(i):
    # min_memory 1000: no network update within the three one-step episodes
    return {"name": "CAC", "gamma": 0.98, "states": 1, "action_range": RANGES[i], "min_memory": 1000, "entropy": 0.01}


FUSED = {"cac-cac-cac-cac": [_cac(0), _cac(1), _cac(2), _cac(3)], "qtable-cac": [dict(Q_AGENT), _cac(1)],
         "cac-qtable": [_cac(0), dict(Q_AGENT)]}


def _game_weights(w0):
    """Per game, in turn: the device's own initial weights, the heads x 40, and two planted sets (tanhf saturated with
    sd = softplus(1); sd = 0)."""
    w = np.array(w0, np.float32, copy=True)
    w[1::4] = CR.scale_heads(w0[1::4], 40)
    w[2::4] = CR.planted(w0[2::4], m=9.02, s=1.0, v=0.0)
    w[3::4] = CR.planted(w0[3::4], m=-0.5, s=-104.0, v=0.0)
    return w


@pytest.mark.parametrize("label", sorted(FUSED))
def test_fused_kernel_actions_against_the_float64_mirror(label):
    """max_steps = 1: the per-game action log is the scaled action of the episode's single step.  The draws are Philox's
    at the counter layout of thrl_device.h (the oracle's Philox is pinned to the Random123 vectors), the price of the
    next episode is recomputed in float64 from the device's logged actions, so every episode is checked on its own."""
    from oracle import oracle as O
    from th_rl_amd.mixed import MixedGameBatch
    agents = FUSED[label]
    N = len(agents)
    config = {"agents": agents, "environment": dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=N, max_steps=1)}
    for G in (5, 259):
        seed = 31 + G
        mb = MixedGameBatch(config, n_games=G, dtype="float64", seed=seed).init_tables()
        W = {}
        for i, nb in mb.nn.items():
            W[i] = _game_weights(nb.params.cpu().numpy())
            nb.set_params(W[i])
        price = mb.states_numpy().copy()
        out = mb.run(EPISODES, fused=True)
        assert out["kernel"] == "mixed-fused" and all(nb.step == 0 for nb in mb.nn.values())
        al = out["game_action_log"]
        assert al.shape == (EPISODES, N, G)
        for e in range(EPISODES):
            for i in sorted(W):
                words = np.array([O.philox(CR.philox_counter(0, e, g, i >> 1), CR.philox_key(seed)) for g in range(G)])
                u1, u2 = CR.pair_draws(words, i)
                with np.errstate(all="ignore"):
                    hd = CR.heads64(W[i], price)
                    z, E_z = CR.z64(u1, u2)
                    a = CR.action64(hd, z)
                    b = CR.bounds(hd, z, E_z)["action"]
                lo, hi = agents[i]["action_range"]
                want = CR.scaled64(a, lo, hi)
                # (the kernel's float64 product and sum: 2^-52 of the value)
                bound = b * (hi - lo) + 2.0 ** -52 * np.abs(want)
                ratio = np.abs(al[e, i] - want) / bound
                WORST["fused scaled action"] = max(WORST.get("fused scaled action", 0.0), float(ratio.max()))
                assert ratio.max() <= 1.0, (label, G, "episode", e, "agent", i, float(ratio.max()), int(ratio.argmax()))
                flat = np.arange(G) % 4 == 3                    # sd = 0: sigmoid(mu) whatever the draw
                mean = CR.scaled64(CR.mean_action64(hd), lo, hi)
                assert (np.abs(al[e, i][flat] - mean[flat]) <= bound[flat]).all()
            price = CR.env_price(al[e])
        assert np.array_equal(price, mb.states_numpy()), (label, G)
    print("%s: worst |device - mirror| / bound so far: %s" % (label, {k: round(v, 4) for k, v in sorted(WORST.items())}))


def test_print_worst_observed_ratios():
    """Runs last in this module: what the device was seen to use of each bound (reported, never used)."""
    print("worst |device - mirror| / bound on the device: %s" % {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())
