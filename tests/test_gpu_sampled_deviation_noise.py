"""The deviation test of sampled play under demand noise on the device (thrl_sampled_deviation_noise,
MixedGameBatch.sampled_deviation_noise, training.sampled_play.deviation with "noise"): every output and row bit-equal to the
numpy mirror (tests/sampled_deviation_noise_mirror.py) on every shape, deviator, length and action mode, with the node count
on the tile's edges, the rows in chunks, in halves and at the edge of the working-set plan; unsolved games beside solved
neighbours; at p = 0 bit-equal to thrl_sampled_deviation; the cross-checks through sampled_play and sampled_response_noise;
the trainer's artefacts.  A handful of games per case."""
import json
import os

import numpy as np
import pytest

import sampled_deviation_mirror as SDM
import sampled_deviation_noise_mirror as SDNM
import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import sampled_response_mirror as SRM
from sampled_mirror import AG, ENV, RF
from sampled_noise_mirror import NO_ATOM, three_agents, two_agents

pytestmark = pytest.mark.gpu

OUT = SDM.AGENT + SDM.FLOAT + SDM.INT
ROWS = SDM.ROWS_AGENT + SDM.ROWS_GAME
TILE = SDNM.TILE
RR5 = two_agents("Reinforce", 5, "Reinforce", 5)
# name -> (config, resolution, games)
SHAPES = {
    "QQ": (two_agents("QTable", 2, "QTable", 2), 0, 5),                    # no network: table node rows only
    "QQ0": (two_agents("QTable", 2, "QTable", 2, NO_ATOM), 0, 5),
    "QR": (two_agents("QTable", 2, "Reinforce", 3), 8, 4),                 # mixed kinds
    "QR0": (two_agents("QTable", 2, "Reinforce", 3, NO_ATOM), 8, 4),
    "QRA": (three_agents(), 8, 3),                                         # the kSpMaxA variant
    "S5a": (RR5, TILE - 1, 3),                                             # the deviator's replaced node row and the
    "S5b": (two_agents("Reinforce", 5, "Reinforce", 5, NO_ATOM), TILE, 3), # best-response pass cross a tile edge
    "S5c": (RR5, 2 * TILE - 2, 3),
    "S5d": (RR5, 2 * TILE, 3),
    "SHIP": (two_agents("QTable", 21, "Reinforce", 21), 64, 3),            # the shipped grid
}
S5_NODES = {"S5a": TILE, "S5b": TILE + 1, "S5c": 2 * TILE - 1, "S5d": 2 * TILE + 1}


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _mixed(config, n_games, seed=3):
    from th_rl_amd.mixed import MixedGameBatch
    return MixedGameBatch(config, n_games=n_games, dtype="float32", seed=seed).init_tables()


def _dev(mb, x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(mb.state.device)


def _inputs(config, resolution, n_games, seed):
    """dict(mb, tabs, probs / nprobs on the device and as numpy (host / nhost), pol, npol, eps [N, G], p [G] with entries at
    exactly 0 and 1, x0 [G, T]): random networks evaluated by thrl_price_probs at the distinct prices and at the nodes."""
    from th_rl_amd import sampled_play as sp
    tabs = sp.noise_tables(config, resolution)
    mb = _mixed(config, n_games)
    rs = np.random.RandomState(seed)
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            mb.nn[i].set_params(SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, 0.0, float(tabs["price"].max())))
    probs, nprobs = sp.price_probs(mb, tabs["dprice"]), sp.price_probs(mb, tabs["xn"])
    host = {i: x.cpu().numpy() for i, x in probs.items()}
    nhost = {i: x.cpu().numpy() for i, x in nprobs.items()}
    pol = SPM.greedy_of(host, tabs, rs, n_games)
    npol = SPM.greedy_of(nhost, SNM.node_tabs(tabs), rs, n_games)
    eps = rs.uniform(0.0, 0.2, (len(tabs["kinds"]), n_games))
    p = rs.uniform(0.0, 0.5, n_games)
    p[0], p[-1] = 0.0, 1.0
    x0 = rs.dirichlet(np.ones(int(tabs["n_tuples"])), n_games)
    return dict(mb=mb, tabs=tabs, probs=probs, nprobs=nprobs, host=host, nhost=nhost, pol=pol, npol=npol, eps=eps, p=p, x0=x0,
                config=config)


def _case(name):
    config, resolution, n_games = SHAPES[name]
    return SPM.cached(("deviation noise case", name), lambda: _inputs(config, resolution, n_games, 400 + sorted(SHAPES).index(name)))


def _run(c, sl=slice(None), **kw):
    mb = c["mb"]
    n = len(range(*sl.indices(c["pol"].shape[0])))
    cut = lambda d: {i: x[sl].contiguous() for i, x in d.items()}
    kw.setdefault("weights", c["x0"][sl])
    kw.setdefault("noise_prob", c["p"][sl])
    return mb.sampled_deviation_noise(n_games=n, probs=cut(c["probs"]), dpolicy=_dev(mb, c["pol"][sl]), tabs=c["tabs"],
                                      nprobs=cut(c["nprobs"]), npolicy=_dev(mb, c["npol"][sl]), **kw)


def _mirror(c, eps, p, x0, **kw):
    return SDNM.analyse(c["tabs"], c["host"], c["pol"], c["nhost"], c["npol"], eps, p, x0, **kw)


def _same(out, ref, fields, what):
    for f in fields:
        _bits_equal(out[f], ref[f], "%s %s" % (what, f))


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_device_equals_the_mirror(name):
    c = _case(name)
    mb, tabs, eps, p, x0 = c["mb"], c["tabs"], c["eps"], c["p"], c["x0"]
    G = SHAPES[name][2]
    N, S = mb.N, int(tabs["n_prices"]) + int(tabs["n_nodes"])
    if name in S5_NODES:
        assert tabs["n_nodes"] == S5_NODES[name]                         # the node count sits on the tile's edge
    assert (tabs["nn"][:, 0] > 0).any() == (not name.endswith("0") and name != "S5b")     # the atom is hit / never hit
    assert p[0] == 0.0 and p[-1] == 1.0
    rs = np.random.RandomState(500 + G)
    gam_g = rs.uniform(0.0, 1.0, (N, G))
    own = SRM.own_gammas(c["config"])
    for dv in range(N):
        A = int(tabs["n_actions"][dv])
        given = rs.randint(0, A + 2, (G, S)).astype(np.uint16)         # entries at and above A: clamped
        # L = 1 of K = 12, the one-period best response, per-game epsilon, gamma and noise
        out = _run(c, deviator=dv, steps=12, dev_len=1, epsilon=eps, gamma=gam_g, rows=True)
        ref = _mirror(c, eps, p, x0, deviator=dv, steps=12, dev_len=1, action=-1, gamma=gam_g[dv])
        _same(out, ref, OUT + ROWS, "%s deviator %d best response" % (name, dv))
        _bits_equal(out["gamma"], gam_g[dv], "gamma")
        _bits_equal(out["epsilon"], eps, "epsilon")
        _bits_equal(out["noise_prob"], p, "noise_prob")
        _bits_equal(out["max_jump"], SNM.max_jump(tabs, c["nhost"], G), "max_jump")
        assert out["solved"].all() and np.abs(out["mass"] - 1.0).max() < 1e-12
        assert out["n_nodes"] == tabs["n_nodes"] and out["lds_bytes"] > 0
        # the rows in tau-chunks of five periods (row_begin > 0) are the rows of one chunk
        chunked = _run(c, deviator=dv, steps=12, dev_len=1, epsilon=eps, gamma=gam_g, rows=True, budget=8 * N * G * 5)
        _same(chunked, out, OUT + ROWS, "%s deviator %d chunked" % (name, dv))
        # L = 3 of K = 12, a fixed action, scalar epsilon, gamma and noise; without rows
        fixed = _run(c, deviator=dv, steps=12, dev_len=3, action=1, epsilon=0.125, gamma=0.9, noise_prob=0.05)
        ref = _mirror(c, 0.125, 0.05, x0, deviator=dv, steps=12, dev_len=3, action=1, gamma=0.9)
        _same(fixed, ref, OUT, "%s deviator %d fixed action" % (name, dv))
        assert not any(f in fixed for f in ROWS)
        # L = K = 5, a given strategy, the deviator's own gamma
        lasting = _run(c, deviator=dv, steps=5, dev_len=5, action=given, epsilon=eps, rows=True)
        ref = _mirror(c, eps, p, x0, deviator=dv, steps=5, dev_len=5, dev_policy=given, gamma=own[dv])
        _same(lasting, ref, OUT + ROWS, "%s deviator %d given strategy" % (name, dv))
        assert (lasting["low_step"] == -1).all() and (lasting["ret_step"] == -1).all() and not lasting["low"].any()
        _bits_equal(lasting["dev_policy"], given, "dev_policy")
        # K = 1
        single = _run(c, deviator=dv, steps=1, dev_len=1, epsilon=eps, gamma=gam_g, rows=True)
        ref = _mirror(c, eps, p, x0, deviator=dv, steps=1, dev_len=1, action=-1, gamma=gam_g[dv])
        _same(single, ref, OUT + ROWS, "%s deviator %d one step" % (name, dv))
    print("%s: dev_share %.3g..%.3g, gain %.3g..%.3g, LDS %d bytes"
          % (name, out["dev_share"].min(), out["dev_share"].max(), out["gain"].min(), out["gain"].max(), out["lds_bytes"]))


@pytest.mark.parametrize("name", ["QQ", "QRA", "S5d"])
def test_one_game_and_the_batch_in_halves(name):
    c = _case(name)
    mb, eps, p = c["mb"], c["eps"], c["p"]
    G = c["pol"].shape[0]
    gam_g = np.random.RandomState(8).uniform(0.3, 0.9, (mb.N, G))
    kw = dict(deviator=mb.N - 1, steps=8, dev_len=2, rows=True)
    whole = _run(c, epsilon=eps, gamma=gam_g, **kw)
    h = G // 2
    for sl in (slice(0, h), slice(h, G), slice(G - 1, G)):
        part = _run(c, sl, epsilon=eps[:, sl], gamma=gam_g[:, sl], **kw)
        for f in OUT + ROWS:
            _bits_equal(part[f], whole[f][..., sl], "%s %s %s" % (name, sl, f))


# ------------------------------------------------------------------------------------------------ unsolved games
def test_unsolved_games_get_zeros_and_leave_their_neighbours_alone():
    """A bad eps_g entry and bad noise_prob_g entries (NaN, < 0, > 1) are device data: zeros, -1 in the steps, zeros in the
    rows, and the solved games beside them as without them."""
    c = _case("QQ")
    eps, p, x0 = c["eps"], c["p"], c["x0"]
    kw = dict(deviator=1, steps=8, dev_len=2, gamma=0.9, rows=True)
    clean = _run(c, epsilon=eps, **kw)
    bad_e, bad_p = eps.copy(), p.copy()
    bad_e[0, 1] = 1.5
    bad_p[2], bad_p[3] = np.nan, -0.1
    out = _run(c, epsilon=bad_e, noise_prob=bad_p, **kw)
    _same(out, _mirror(c, bad_e, bad_p, x0, deviator=1, steps=8, dev_len=2, action=-1, gamma=0.9), OUT + ROWS, "unsolved")
    ok = np.array([True, False, False, False, True])
    assert (out["low_step"][~ok] == -1).all() and (out["ret_step"][~ok] == -1).all() and np.array_equal(out["solved"], ok)
    for f in SDM.AGENT + SDM.FLOAT + ROWS:
        assert not out[f][..., ~ok].any(), f
    for f in OUT + ROWS:
        _bits_equal(out[f][..., ok], clean[f][..., ok], "neighbours " + f)
    bad_p[3] = 1.5
    bad_e[0, 1] = np.nan
    again = _run(c, epsilon=bad_e, noise_prob=bad_p, **kw)
    assert not again["gain"][~ok].any() and np.array_equal(again["solved"], ok)
    _bits_equal(again["gain"][ok], clean["gain"][ok], "neighbours")


# ------------------------------------------------------------------------------------------------ through existing code
@pytest.mark.parametrize("name", ["QR", "QRA", "S5c"])
def test_without_noise_the_call_is_the_noise_free_one_bit_for_bit(name):
    """p = 0: every output and row has the bits of thrl_sampled_deviation on the same inputs."""
    c = _case(name)
    mb, tabs, eps, x0 = c["mb"], c["tabs"], c["eps"], c["x0"]
    G, D = c["pol"].shape[0], int(tabs["n_prices"])
    rs = np.random.RandomState(9)
    free = lambda **kw: mb.sampled_deviation(probs=c["probs"], dpolicy=_dev(mb, c["pol"]), tabs=tabs, weights=x0, epsilon=eps, rows=True, **kw)
    for dv in range(mb.N):
        A = int(tabs["n_actions"][dv])
        given = rs.randint(0, A, (G, D + int(tabs["n_nodes"]))).astype(np.uint16)
        for kw, action in ((dict(steps=9, dev_len=2, gamma=0.9), "best_response"), (dict(steps=4, dev_len=4, gamma=0.5), given),
                           (dict(steps=6, dev_len=1, gamma=1.0), A - 1)):
            for zero in (0.0, np.zeros(G)):                  # the scalar and the per-game form
                out = _run(c, deviator=dv, action=action, epsilon=eps, rows=True, noise_prob=zero, **kw)
                ref = free(deviator=dv, action=given[:, :D] if action is given else action, **kw)
                _same(out, ref, OUT + ROWS, "%s deviator %d p = 0" % (name, dv))


def test_the_baseline_is_sampled_plays_long_run_profit_under_the_same_noise():
    """weights = "stationary": x_0 is sampled_play(noise_prob=...)'s pi on the same rows, so base_* are its samp_* bit for
    bit, and the call returns its step counts and its max_jump."""
    c = _case("QR")
    mb, tabs, eps, p = c["mb"], c["tabs"], c["eps"], c["p"]
    rows = dict(probs=c["probs"], dpolicy=_dev(mb, c["pol"]), tabs=tabs, nprobs=c["nprobs"], npolicy=_dev(mb, c["npol"]))
    for max_iters in (8192, 3):
        st = mb.sampled_play(epsilon=eps, pi=True, max_iters=max_iters, noise_prob=p, **rows)
        out = _run(c, deviator=0, steps=4, epsilon=eps, weights="stationary", max_iters=max_iters)
        _bits_equal(out["base_reward"], st["samp_reward"], "base_reward")
        _bits_equal(out["base_action"], st["samp_action"], "base_action")
        _bits_equal(out["base_price"], st["samp_price"], "base_price")
        _bits_equal(out["max_jump"], st["max_jump"], "max_jump")
        assert np.array_equal(out["stat_iters"], st["iters"]) and (st["iters"] == 3).all() == (max_iters == 3)
        own = SRM.own_gammas(c["config"])[0]
        _same(out, _mirror(c, eps, p, st["pi"], deviator=0, steps=4, gamma=own), OUT, "stationary")


def test_best_reply_deviates_to_sampled_response_noises_policy():
    c = _case("QRA")
    mb, tabs, eps = c["mb"], c["tabs"], c["eps"]
    G = c["pol"].shape[0]
    dv = 1
    p = np.maximum(c["p"], 0.05)                         # the best responses under noise need p > 0
    rows = dict(probs=c["probs"], dpolicy=_dev(mb, c["pol"]), ntabs=tabs, nprobs=c["nprobs"], npolicy=_dev(mb, c["npol"]))
    br = mb.sampled_response_noise(agents=[dv], epsilon=eps, gamma=0.6, policies=True, pi=False, noise_prob=p, **rows)
    assert (br["iters"][dv] >= 0).all()
    out = _run(c, deviator=dv, steps=8, dev_len=8, action="best_reply", epsilon=eps, gamma=0.6, rows=True, noise_prob=p)
    _bits_equal(out["dev_policy"], br["br_policy"][dv], "dev_policy")
    _same(out, _run(c, deviator=dv, steps=8, dev_len=8, action=br["br_policy"][dv], epsilon=eps, gamma=0.6, rows=True, noise_prob=p),
          OUT + ROWS, "best_reply")
    assert out["solved"].all()
    # a game sampled_response_noise refuses (its p is 0) is not solved here; its neighbours are
    part = _run(c, deviator=dv, steps=8, dev_len=8, action="best_reply", epsilon=eps, gamma=0.6, rows=True,
                noise_prob=np.where(np.arange(G) == 0, 0.0, p))
    assert not part["solved"][0] and part["low_step"][0] == -1 and part["ret_step"][0] == -1
    for f in SDM.AGENT + SDM.FLOAT + ROWS:
        assert not part[f][..., 0].any(), f
        _bits_equal(part[f][..., 1:], out[f][..., 1:], "neighbours " + f)


def test_group_stats_curves_are_the_rows_reduced_on_the_host():
    from th_rl_amd.group_stats import GroupSpec, reduce_host, resolve_ranges
    c = _case("QQ")
    eps = c["eps"]
    G = c["pol"].shape[0]
    ids = np.arange(G) % 2
    spec = GroupSpec(2, ids, 2, resolve_ranges(c["config"]), bins=64)
    one = _run(c, deviator=0, steps=9, dev_len=2, epsilon=eps, gamma=0.9, rows=True)
    st = _run(c, deviator=0, steps=9, dev_len=2, epsilon=eps, gamma=0.9, group_stats=spec, budget=8 * 2 * G * 4)
    assert "reward_rows" not in st
    _same(st, one, OUT, "with group_stats")
    raw = reduce_host(one["reward_rows"], one["action_rows"], ids, 2, spec.describe())
    for k in ("hist", "sums", "minmax"):
        assert np.array_equal(np.asarray(st["group_stats"][k]).view(np.uint8), np.asarray(raw[k]).view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ the working set
def test_the_largest_accepted_working_set_and_the_first_refused_shape():
    """Of QTable A x Reinforce B for A in 20..39 and B in 21 / 24 / 28 / 32 at the default resolution the heaviest shape the
    plan accepts is 27 x 32 (163,696 of 163,840 bytes), run here for one game and equal to the mirror; the lightest it
    refuses is 35 x 28 (164,544 bytes), THRL_ERR_UNSUPPORTED without a launch."""
    from th_rl_amd import _lib
    from th_rl_amd import sampled_deviation as sd
    from th_rl_amd import sampled_play as sp
    from th_rl_amd._lib import ThrlError

    def cfg(A, B):
        return {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}
    ws, over = sd.working_set_noise(cfg(27, 32)), sd.working_set_noise(cfg(35, 28))
    assert ws["bytes"] == 163696 and ws["fits"] and ws["bytes"] <= sd.MAX_LDS
    assert over["bytes"] == 164544 and not over["fits"]
    c = _inputs(cfg(27, 32), 1024, 1, 31)
    c["p"][:] = 0.25
    out = _run(c, deviator=1, steps=3, dev_len=1, epsilon=c["eps"], gamma=0.9, rows=True)
    assert out["lds_bytes"] == ws["bytes"] and out["n_nodes"] == ws["Jn"]
    _same(out, _mirror(c, c["eps"], c["p"], c["x0"], deviator=1, steps=3, dev_len=1, action=-1, gamma=0.9), OUT + ROWS, "largest")
    # the next shape: refused by the library from the shape alone (no tensor is valid, none is touched)
    mb2 = _mixed(cfg(35, 28), 1)
    tabs2 = sp.noise_tables(cfg(35, 28))
    with pytest.raises(ThrlError) as e:
        mb2.sampled_deviation_noise(tabs=tabs2, weights=np.zeros((1, over["T"])), noise_prob=0.05)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a = _lib.SampledDeviationNoiseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.dev_len, a.n_steps, a.dev_action = 1, over["T"], over["D"], 1, 4, -1
    a.n_nodes, a.band_w, a.noise_prob = over["Jn"], int(tabs2["band_w"]), 0.05
    a.kind[1] = 1
    assert mb2.L.thrl_sampled_deviation_noise(mb2.cfg, a, None) == _lib.ERR_UNSUPPORTED
    assert b"164544 bytes of LDS per game" in mb2.L.thrl_last_error()


# ------------------------------------------------------------------------------------------------ the trainer
def test_train_one_writes_the_deviation_test_under_noise_beside_sampled_play(tmp_path):
    from th_rl_amd import utils
    from th_rl_amd.trainer import train_one
    base = {"agents": [dict(AG, actions=3, states=10), dict(RF, actions=3)], "environment": dict(ENV, max_steps=10)}
    noise = {"noise_prob": 0.05, "resolution": 16}
    dev = {"steps": 6, "dev_len": 2, "ret_tol": 1e-3}
    runs = {}
    for key, extra in (("plain", {"noise": noise}), ("free", {"deviation": dev}), ("dev", {"noise": noise, "deviation": dict(dev, noise=True)})):
        cfg = dict(base, training={"epochs": 4, "print_freq": 500, "seed": 3, "n_games": 2, "n_groups": 2, "groups": [0, 1],
                                   "group_stats": {"bins": 16}, "sampled_play": dict({"pi": True}, **extra)})
        (tmp_path / (key + ".json")).write_text(json.dumps(cfg))
        train_one(str(tmp_path / key), str(tmp_path / (key + ".json")))
        runs[key] = str(tmp_path / key)
    files = sorted(os.listdir(runs["dev"]))
    for f in ("sampled_deviation_noise.json", "sdevn_epsilon.npy", "sdevn_solved.npy", "sdevn_stat_iters.npy", "sdevn_noise_prob.npy",
              "sdevn_max_jump.npy", "sdevn0_games.npy", "sdevn0_steps.npy", "sdevn0_base.npy", "sdevn0_gamma.npy", "sdevn1_games.npy",
              "sdevn0_mean.npy", "sdevn1_quantiles.npy"):
        assert f in files, (f, files)
    # the noise-free files are absent with the key, and without it they are what they were: the run without "noise" writes
    # them and none of the new ones; the run under noise without the sub-key writes neither
    noise_free = lambda f: (f.startswith("sdev") and not f.startswith("sdevn")) or f == "sampled_deviation.json"
    under_noise = lambda f: f.startswith("sdevn") or f == "sampled_deviation_noise.json"
    assert not any(noise_free(f) for f in files)
    assert not any(noise_free(f) or under_noise(f) for f in os.listdir(runs["plain"]))
    assert any(noise_free(f) for f in os.listdir(runs["free"])) and not any(under_noise(f) for f in os.listdir(runs["free"]))
    for f in sorted(os.listdir(runs["plain"])):
        if f.startswith("splay_"):
            assert open(os.path.join(runs["plain"], f), "rb").read() == open(os.path.join(runs["dev"], f), "rb").read(), f
    desc = json.load(open(os.path.join(runs["dev"], "sampled_deviation_noise.json")))
    assert desc["options"] == {"agents": [0, 1], "steps": 6, "dev_len": 2, "action": "best_response", "ret_tol": 1e-3, "noise": True}
    assert desc["resolution"] == 16 and desc["n_nodes"] > 2
    assert "deviation" not in json.load(open(os.path.join(runs["dev"], "sampled_play.json")))["options"]
    summary = utils.sampled_deviation_noise_summary(runs["dev"])
    assert len(summary) == 4 and set(summary["deviator"]) == {0, 1} and (summary["solved"] == 1).all()
    assert "max_jump_max" in summary.columns and (summary["n_nodes"] == desc["n_nodes"]).all()
    play = utils.sampled_play_games(runs["dev"])
    for d in (0, 1):
        games = utils.sampled_deviation_noise_games(runs["dev"], deviator=d)
        assert len(games) == 2 and games["solved"].all() and np.isfinite(games["gain"]).all()
        assert np.array_equal(games["stat_iters"], play["iters"]) and (games["noise_prob"] == 0.05).all()
        _bits_equal(games["base_reward_%d" % d].to_numpy(), play["reward_%d" % d].to_numpy(), "base against sampled_play.json")
        curve = utils.group_quantiles(runs["dev"], 0, "total", prefix="sdevn%d" % d)
        assert len(curve) == 6
    with pytest.raises(KeyError):
        utils.sampled_deviation_summary(runs["dev"])
