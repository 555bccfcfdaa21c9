"""The deviation test of sampled play on the device (thrl_sampled_deviation, MixedGameBatch.sampled_deviation,
training.sampled_play.deviation): every output and row bit-equal to the numpy mirror (tests/sampled_deviation_mirror.py) on
every shape, deviator, length and action mode, with the rows in chunks, in halves and at the edge of the working-set plan;
an unsolved game beside solved neighbours; the cross-checks through sampled_play, sampled_response and the group
statistics; the trainer's artefacts.  A handful of games per case."""
import json
import os

import numpy as np
import pytest

import sampled_deviation_mirror as SDM
import sampled_mirror as SPM
import sampled_response_mirror as SRM
from sampled_mirror import AG, ENV, QQ, QR, QRA, RF, RR, SHIP

pytestmark = pytest.mark.gpu

OUT = SDM.AGENT + SDM.FLOAT + SDM.INT
ROWS = SDM.ROWS_AGENT + SDM.ROWS_GAME
# (config, games, seed)
CASES = {"QQ": (QQ, 5, 21), "QR": (QR, 4, 22), "QRA": (QRA, 3, 23), "RR": (RR, 1, 24), "SHIP": (SHIP, 3, 25)}


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


def _inputs(config, n_games, seed):
    """(batch, tabs, probs on the device, probs as numpy, dpolicy, eps [N, G], x0 [G, T]): random networks evaluated by
    thrl_price_probs, the networks' dpolicy entries their rows' first maxima, the QTable entries random with some at or
    above the action count, x0 a random distribution per game."""
    from th_rl_amd import sampled_play as sp
    tabs = sp.tables(config)
    mb = _mixed(config, n_games)
    rs = np.random.RandomState(seed)
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            mb.nn[i].set_params(SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, tabs["price"].min(), tabs["price"].max()))
    probs = sp.price_probs(mb, tabs["dprice"])
    host = {i: p.cpu().numpy() for i, p in probs.items()}
    pol = SPM.greedy_of(host, tabs, rs, n_games)
    eps = rs.uniform(0.0, 0.2, (len(tabs["kinds"]), n_games))
    x0 = rs.dirichlet(np.ones(int(tabs["n_tuples"])), n_games)
    return mb, tabs, probs, host, pol, eps, x0


def _case(name):
    config, n_games, seed = CASES[name]
    return SPM.cached(("deviation case", name), lambda: _inputs(config, n_games, seed))


def _run(case, sl=slice(None), **kw):
    mb, tabs, probs, host, pol, eps, x0 = case
    n = len(range(*sl.indices(pol.shape[0])))
    kw.setdefault("weights", x0[sl])
    return mb.sampled_deviation(n_games=n, probs={i: p[sl].contiguous() for i, p in probs.items()}, dpolicy=_dev(mb, pol[sl]),
                                tabs=tabs, **kw)


def _same(out, ref, fields, what):
    for f in fields:
        _bits_equal(out[f], ref[f], "%s %s" % (what, f))


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", ["QQ", "QR", "QRA", "RR", "SHIP"])
def test_the_device_equals_the_mirror(name):
    case = _case(name)
    mb, tabs, probs, host, pol, eps, x0 = case
    config, G, seed = CASES[name]
    N, D = mb.N, int(tabs["n_prices"])
    rs = np.random.RandomState(seed + 100)
    gam_g = rs.uniform(0.0, 1.0, (N, G))
    own = SRM.own_gammas(config)
    for dv in range(N):
        A = int(tabs["n_actions"][dv])
        given = rs.randint(0, A + 2, (G, D)).astype(np.uint16)         # entries at and above A: clamped
        # L = 1 of K = 12, the one-period best response, per-game epsilon and gamma
        out = _run(case, deviator=dv, steps=12, dev_len=1, epsilon=eps, gamma=gam_g, rows=True)
        ref = SDM.analyse(tabs, host, pol, eps, x0, deviator=dv, steps=12, dev_len=1, action=-1, gamma=gam_g[dv])
        _same(out, ref, OUT + ROWS, "%s deviator %d best response" % (name, dv))
        _bits_equal(out["gamma"], gam_g[dv], "gamma")
        _bits_equal(out["epsilon"], eps, "epsilon")
        assert out["solved"].all() and np.abs(out["mass"] - 1.0).max() < 1e-12 and out["lds_bytes"] > 0
        # the rows in tau-chunks of five periods (row_begin > 0) are the rows of one chunk
        chunked = _run(case, deviator=dv, steps=12, dev_len=1, epsilon=eps, gamma=gam_g, rows=True, budget=8 * N * G * 5)
        _same(chunked, out, OUT + ROWS, "%s deviator %d chunked" % (name, dv))
        # L = 3 of K = 12, a fixed action, scalar epsilon and gamma; without rows
        fixed = _run(case, deviator=dv, steps=12, dev_len=3, action=1, epsilon=0.125, gamma=0.9)
        ref = SDM.analyse(tabs, host, pol, 0.125, x0, deviator=dv, steps=12, dev_len=3, action=1, gamma=0.9)
        _same(fixed, ref, OUT, "%s deviator %d fixed action" % (name, dv))
        assert not any(f in fixed for f in ROWS)
        # L = K = 5, a given strategy, the deviator's own gamma
        lasting = _run(case, deviator=dv, steps=5, dev_len=5, action=given, epsilon=eps, rows=True)
        ref = SDM.analyse(tabs, host, pol, eps, x0, deviator=dv, steps=5, dev_len=5, dev_policy=given, gamma=own[dv])
        _same(lasting, ref, OUT + ROWS, "%s deviator %d given strategy" % (name, dv))
        assert (lasting["low_step"] == -1).all() and (lasting["ret_step"] == -1).all() and not lasting["low"].any()
        _bits_equal(lasting["dev_policy"], given, "dev_policy")
        # K = 1
        single = _run(case, deviator=dv, steps=1, dev_len=1, epsilon=eps, gamma=gam_g, rows=True)
        ref = SDM.analyse(tabs, host, pol, eps, x0, deviator=dv, steps=1, dev_len=1, action=-1, gamma=gam_g[dv])
        _same(single, ref, OUT + ROWS, "%s deviator %d one step" % (name, dv))
    print("%s: dev_share %.3g..%.3g, gain %.3g..%.3g, LDS %d bytes"
          % (name, out["dev_share"].min(), out["dev_share"].max(), out["gain"].min(), out["gain"].max(), out["lds_bytes"]))


@pytest.mark.parametrize("name", ["QQ", "QRA"])
def test_one_game_and_the_batch_in_halves(name):
    case = _case(name)
    mb, tabs, probs, host, pol, eps, x0 = case
    G = pol.shape[0]
    gam_g = np.random.RandomState(8).uniform(0.3, 0.9, (mb.N, G))
    kw = dict(deviator=mb.N - 1, steps=8, dev_len=2, rows=True)
    whole = _run(case, epsilon=eps, gamma=gam_g, **kw)
    h = G // 2
    for sl in (slice(0, h), slice(h, G), slice(G - 1, G)):
        part = _run(case, sl, epsilon=eps[:, sl], gamma=gam_g[:, sl], **kw)
        for f in OUT + ROWS:
            _bits_equal(part[f], whole[f][..., sl], "%s %s %s" % (name, sl, f))


# ------------------------------------------------------------------------------------------------ unsolved games
def test_an_unsolved_game_gets_zeros_and_leaves_its_neighbours_alone():
    case = _case("QR")
    mb, tabs, probs, host, pol, eps, x0 = case
    kw = dict(deviator=1, steps=8, dev_len=2, gamma=0.9, rows=True)
    clean = _run(case, epsilon=eps, **kw)
    bad = eps.copy()
    bad[0, 1] = 1.5                                      # the QTable agent's epsilon of game 1: device data
    out = _run(case, epsilon=bad, **kw)
    _same(out, SDM.analyse(tabs, host, pol, bad, x0, deviator=1, steps=8, dev_len=2, action=-1, gamma=0.9), OUT + ROWS, "unsolved")
    assert out["low_step"][1] == -1 and out["ret_step"][1] == -1 and not out["solved"][1] and out["solved"][[0, 2, 3]].all()
    for f in SDM.AGENT + SDM.FLOAT + ROWS:
        assert not out[f][..., 1].any(), f
    ok = np.array([True, False, True, True])
    for f in OUT + ROWS:
        _bits_equal(out[f][..., ok], clean[f][..., ok], "neighbours " + f)
    bad[0, 1] = np.nan
    assert not _run(case, epsilon=bad, **kw)["gain"][1]


# ------------------------------------------------------------------------------------------------ through existing code
def test_the_baseline_is_sampled_plays_long_run_profit():
    """weights = "stationary": x_0 is sampled_play's pi on the same rows, so base_* are its samp_* bit for bit, and the
    call returns its step counts; a start from the step limit is taken all the same."""
    case = _case("QR")
    mb, tabs, probs, host, pol, eps, _ = case
    for max_iters in (8192, 3):
        st = mb.sampled_play(epsilon=eps, pi=True, max_iters=max_iters, probs=probs, dpolicy=_dev(mb, pol), tabs=tabs)
        out = _run(case, deviator=0, steps=4, epsilon=eps, weights="stationary", max_iters=max_iters)
        _bits_equal(out["base_reward"], st["samp_reward"], "base_reward")
        _bits_equal(out["base_action"], st["samp_action"], "base_action")
        _bits_equal(out["base_price"], st["samp_price"], "base_price")
        assert np.array_equal(out["stat_iters"], st["iters"]) and (st["iters"] == 3).all() == (max_iters == 3)
        _same(out, SDM.analyse(tabs, host, pol, eps, st["pi"], deviator=0, steps=4, gamma=SRM.own_gammas(QR)[0]), OUT, "stationary")


def test_best_reply_deviates_to_sampled_responses_policy():
    case = _case("QRA")
    mb, tabs, probs, host, pol, eps, x0 = case
    G = pol.shape[0]
    dv = 1
    br = mb.sampled_response(agents=[dv], epsilon=eps, gamma=0.6, policies=True, pi=False, probs=probs, dpolicy=_dev(mb, pol), tabs=tabs)
    assert (br["iters"][dv] >= 0).all()
    out = _run(case, deviator=dv, steps=8, dev_len=8, action="best_reply", epsilon=eps, gamma=0.6, rows=True)
    _bits_equal(out["dev_policy"], br["br_policy"][dv], "dev_policy")
    _same(out, _run(case, deviator=dv, steps=8, dev_len=8, action=br["br_policy"][dv], epsilon=eps, gamma=0.6, rows=True),
          OUT + ROWS, "best_reply")
    assert out["solved"].all()
    # a game sampled_response leaves unsolved (its gamma is 1.0) is not solved here; its neighbours are
    gam = np.full((mb.N, G), 0.6)
    gam[dv, 2] = 1.0
    part = _run(case, deviator=dv, steps=8, dev_len=8, action="best_reply", epsilon=eps, gamma=gam, rows=True)
    assert not part["solved"][2] and part["low_step"][2] == -1 and part["ret_step"][2] == -1
    for f in SDM.AGENT + SDM.FLOAT + ROWS:
        assert not part[f][..., 2].any(), f
        _bits_equal(part[f][..., :2], out[f][..., :2], "neighbours " + f)


def test_group_stats_curves_are_the_rows_reduced_on_the_host():
    from th_rl_amd.group_stats import GroupSpec, reduce_host, resolve_ranges
    case = _case("QQ")
    mb, tabs, probs, host, pol, eps, x0 = case
    G = pol.shape[0]
    ids = np.arange(G) % 2
    spec = GroupSpec(2, ids, 2, resolve_ranges(QQ), bins=64)
    one = _run(case, deviator=0, steps=9, dev_len=2, epsilon=eps, gamma=0.9, rows=True)
    st = _run(case, deviator=0, steps=9, dev_len=2, epsilon=eps, gamma=0.9, group_stats=spec, budget=8 * 2 * G * 4)
    assert "reward_rows" not in st
    _same(st, one, OUT, "with group_stats")
    raw = reduce_host(one["reward_rows"], one["action_rows"], ids, 2, spec.describe())
    for k in ("hist", "sums", "minmax"):
        assert np.array_equal(np.asarray(st["group_stats"][k]).view(np.uint8), np.asarray(raw[k]).view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ the working set
def test_the_largest_accepted_working_set_and_the_first_refused_shape():
    """Of QTable A x Reinforce B for A in 20..39 and B in 21 / 24 / 28 / 32 the heaviest shape the plan accepts is 28 x 32
    (T = D = 896: 161,552 of 163,840 bytes), run here for one game and equal to the mirror; the lightest it refuses is
    35 x 32 (T = 1120, D = 936: 171,904 bytes), THRL_ERR_UNSUPPORTED without a launch."""
    from th_rl_amd import _lib
    from th_rl_amd import sampled_deviation as sd
    from th_rl_amd import sampled_play as sp
    from th_rl_amd._lib import ThrlError

    def cfg(A, B):
        return {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}
    ws, over = sd.working_set(cfg(28, 32)), sd.working_set(cfg(35, 32))
    assert ws == dict(bytes=161552, T=896, D=896, fits=True) and ws["bytes"] <= sd.MAX_LDS
    assert over == dict(bytes=171904, T=1120, D=936, fits=False)
    case = _inputs(cfg(28, 32), 1, 31)
    mb, tabs, probs, host, pol, eps, x0 = case
    out = _run(case, deviator=1, steps=3, dev_len=1, epsilon=eps, gamma=0.9, rows=True)
    assert out["lds_bytes"] == ws["bytes"]
    _same(out, SDM.analyse(tabs, host, pol, eps, x0, deviator=1, steps=3, dev_len=1, action=-1, gamma=0.9), OUT + ROWS, "largest")
    # the next shape: refused by the library from the shape alone (no tensor is valid, none is touched)
    mb2 = _mixed(cfg(35, 32), 1)
    tabs2 = sp.tables(cfg(35, 32))
    with pytest.raises(ThrlError) as e:
        mb2.sampled_deviation(tabs=tabs2, weights=np.zeros((1, 1120)))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a = _lib.SampledDeviationArgs()
    a.n_games, a.n_tuples, a.n_prices, a.dev_len, a.n_steps, a.dev_action = 1, 1120, 936, 1, 4, -1
    a.kind[1] = 1
    assert mb2.L.thrl_sampled_deviation(mb2.cfg, a, None) == _lib.ERR_UNSUPPORTED
    assert b"171904 bytes of LDS per game" in mb2.L.thrl_last_error()


# ------------------------------------------------------------------------------------------------ the trainer
def test_train_one_writes_the_deviation_test_beside_sampled_play(tmp_path):
    from th_rl_amd import utils
    from th_rl_amd.trainer import train_one
    base = {"agents": [dict(AG, actions=3, states=10), dict(RF, actions=3)], "environment": dict(ENV, max_steps=10)}
    runs = {}
    for key, extra in (("plain", {}), ("dev", {"deviation": {"steps": 6, "dev_len": 2, "ret_tol": 1e-3}})):
        cfg = dict(base, training={"epochs": 4, "print_freq": 500, "seed": 3, "n_games": 2, "n_groups": 2, "groups": [0, 1],
                                   "group_stats": {"bins": 16}, "sampled_play": dict({"pi": True}, **extra)})
        (tmp_path / (key + ".json")).write_text(json.dumps(cfg))
        train_one(str(tmp_path / key), str(tmp_path / (key + ".json")))
        runs[key] = str(tmp_path / key)
    files = sorted(os.listdir(runs["dev"]))
    for f in ("sampled_deviation.json", "sdev_epsilon.npy", "sdev_solved.npy", "sdev_stat_iters.npy", "sdev0_games.npy",
              "sdev0_steps.npy", "sdev0_base.npy", "sdev0_gamma.npy", "sdev1_games.npy", "sdev0_mean.npy", "sdev1_quantiles.npy"):
        assert f in files, (f, files)
    assert not any(f.startswith("sdev") or f == "sampled_deviation.json" for f in os.listdir(runs["plain"]))
    for f in sorted(os.listdir(runs["plain"])):
        if f.startswith("splay_"):
            assert open(os.path.join(runs["plain"], f), "rb").read() == open(os.path.join(runs["dev"], f), "rb").read(), f
    desc = json.load(open(os.path.join(runs["dev"], "sampled_deviation.json")))
    assert desc["options"] == {"agents": [0, 1], "steps": 6, "dev_len": 2, "action": "best_response", "ret_tol": 1e-3}
    assert "deviation" not in json.load(open(os.path.join(runs["dev"], "sampled_play.json")))["options"]
    summary = utils.sampled_deviation_summary(runs["dev"])
    assert len(summary) == 4 and set(summary["deviator"]) == {0, 1} and (summary["solved"] == 1).all()
    play = utils.sampled_play_games(runs["dev"])
    for d in (0, 1):
        games = utils.sampled_deviation_games(runs["dev"], deviator=d)
        assert len(games) == 2 and games["solved"].all() and np.isfinite(games["gain"]).all()
        assert np.array_equal(games["stat_iters"], play["iters"])
        _bits_equal(games["base_reward_%d" % d].to_numpy(), play["reward_%d" % d].to_numpy(), "base against sampled_play.json")
        curve = utils.group_quantiles(runs["dev"], 0, "total", prefix="sdev%d" % d)
        assert len(curve) == 6
