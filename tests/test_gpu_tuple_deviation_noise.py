"""The deviation test under demand noise in tuple form on the device (thrl_tuple_deviation_noise,
greedy_deviation_noise(), the option "noise" of training.greedy_deviation): every output and every row bit-equal to the
numpy mirror (tests/tuple_deviation_noise_mirror.py) on random strategies and random start distributions for a QTable
against a Reinforce agent (T = 25, 24 cells, 70 games), 9 x 9 actions at resolution 100 (T = 81, past one 64-lane
chunk), 5 x 5 at resolution 600 (J > 512: a thread's second pair of cells), 21 x 21 (T = 441 > 256 threads), three agents
with deviator 2, and 64 x 32 actions whose working set is above the 64 KB a block gets by default; on the smallest shape a
fixed action, dev_len 1, 3 and = steps, row slices, per-game noise with bad entries, p = 1, ret_tol = 0, band rows that
stick out of the cells, every kind of weights, extracted strategies, a prefix of the games, more games than the grid; the
batch method on a briefly trained example pairing and the trainer's artefacts.

The random inputs carry the coverage: tests/test_tuple_deviation_noise_host.py asserts on the mirror that the deviation
changes play and the response in most games and that the gain has both signs."""
import json

import numpy as np
import pytest

import tuple_deviation_noise_mirror as TD
import tuple_stationary_mirror as SM
from test_gpu_analysis_geometry import CONFIG as GEO, K as KB, _batch as _geo_batch, _bytes, _per_game, base  # noqa: F401
from test_gpu_tuple_attractors import ENV, _bits_equal, _device, _mixed
from test_tuple_deviation_noise_host import DCASES, QR, gammas, inputs, reference

pytestmark = pytest.mark.gpu

FIELDS = TD.AGENT_FIELDS + TD.FLOAT_FIELDS + TD.INT_FIELDS
_MB = {}


def _batch_of(name):
    """The batch of a case, made once (its tables are not read: every strategy is given)."""
    if name not in _MB:
        config, _, G = DCASES[name][:3]
        _MB[name] = _mixed(config, n_games=G)
    return _MB[name]


def _check(mb, config, tabs, tpol, cpol, weights, noise_prob=0.05, ref=None, gamma=None, **kw):
    """greedy_deviation_noise(rows=True, ...) on the given strategies against the mirror: (device, mirror)."""
    n = kw.get("n_games") or tpol.shape[0]
    w = weights if isinstance(weights, str) else np.ascontiguousarray(weights[:n])
    out = mb.greedy_deviation_noise(noise_prob=noise_prob, rows=True, weights=w, tuple_policy=_device(mb, tpol),
                                    cell_policy=_device(mb, cpol[:n]), tabs=tabs, **kw)
    if ref is None:
        m0 = w
        if isinstance(w, str):
            m0 = SM.analyse(tabs, tpol[:n], cpol[:n], noise_prob, tol=kw.get("tol", 1e-12), max_iters=kw.get("max_iters", 8192))["pi"]
        act = kw.get("action", "best_response")
        ref = TD.analyse(tabs, tpol, cpol, noise_prob if np.ndim(noise_prob) == 0 else np.asarray(noise_prob)[:n], m0,
                         deviator=kw.get("deviator", 0), steps=kw.get("steps", 32), dev_len=kw.get("dev_len", 1),
                         dev_action=-1 if act == "best_response" else act, ret_tol=kw.get("ret_tol", 1e-6),
                         gamma=gammas(config) if gamma is None else gamma, n_games=kw.get("n_games"))
    for f in FIELDS + TD.ROW_FIELDS:
        _bits_equal(out[f], ref[f], f)
    assert out["n_cells"] == tabs["n_cells"] and out["T"] == tabs["n_tuples"]
    return out, ref


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", ["QR", "NINE", "FINE", "W21", "TRIO", "BIG"])
def test_random_strategies_equal_mirror(name):
    config, tabs, tpol, cpol, w, d, K, L = inputs(name)
    out, ref = _check(_batch_of(name), config, tabs, tpol, cpol, w, ref=reference(name), deviator=d, steps=K, dev_len=L)
    assert out["reward_rows"].shape == (K, len(config["agents"]), tpol.shape[0]) and out["dist_rows"].shape == (K, tpol.shape[0])
    assert (out["dev_share"] > 0.1).any() and (out["gain"] > 0).any() and (out["gain"] < 0).any()
    assert np.abs(out["mass"] - 1.0).max() <= 1e-12 and (out["dist_rows"][0] == 0.0).all()
    need = 28 * out["T"] + 10 * out["n_cells"] + 512 * (2 * len(config["agents"]) + 2) + 6
    assert (need > 64 * 1024) == (name == "BIG")
    print("%s: T %d, J %d, %d bytes of LDS, gain %.3g..%.3g" % (name, out["T"], out["n_cells"], need, out["gain"].min(),
                                                               out["gain"].max()))


def test_a_fixed_action_the_length_of_the_deviation_and_ret_tol():
    config, tabs, tpol, cpol, w, d, K, L = inputs("QR")
    mb = _batch_of("QR")
    fixed, _ = _check(mb, config, tabs, tpol, cpol, w, steps=6, action=2, n_games=24)
    best, _ = _check(mb, config, tabs, tpol, cpol, w, steps=6, n_games=24)
    assert not np.array_equal(fixed["gain"], best["gain"]) and (best["gain_dev"] >= fixed["gain_dev"]).all()
    one, _ = _check(mb, config, tabs, tpol, cpol, w, steps=5, dev_len=1, deviator=1, n_games=24)
    three, _ = _check(mb, config, tabs, tpol, cpol, w, steps=5, dev_len=3, deviator=1, n_games=24)
    full, _ = _check(mb, config, tabs, tpol, cpol, w, steps=5, dev_len=5, deviator=1, n_games=24)
    _bits_equal(one["reward_rows"][0], three["reward_rows"][0])
    assert not np.array_equal(one["reward_rows"][1], three["reward_rows"][1])
    assert (full["low"] == 0.0).all() and (full["low_step"] == -1).all() and np.array_equal(full["gain"], full["gain_dev"])
    assert (three["low_step"] >= 3).all()
    zero, ref = _check(mb, config, tabs, tpol, cpol, w, steps=5, ret_tol=0.0, n_games=24)
    wide, _ = _check(mb, config, tabs, tpol, cpol, w, steps=5, ret_tol=1.0, n_games=24)
    assert (wide["ret_step"] == 1).all() and (zero["ret_step"] <= 5).all() and (zero["ret_step"] == -1).any()


def test_row_slices_and_no_rows():
    config, tabs, tpol, cpol, w, d, K, L = inputs("QR")
    mb = _batch_of("QR")
    ref = reference("QR")
    dt, dc = _device(mb, tpol), _device(mb, cpol)
    kw = dict(noise_prob=0.05, weights=w, tuple_policy=dt, cell_policy=dc, tabs=tabs, deviator=d, steps=K, dev_len=L)
    none = mb.greedy_deviation_noise(**kw)
    assert not any(f in none for f in TD.ROW_FIELDS)
    for f in FIELDS:
        _bits_equal(none[f], ref[f], f)
    # a budget of three periods per chunk: row_begin = 0, 3, 6, 9
    G, N = tpol.shape[0], 2
    sliced = mb.greedy_deviation_noise(rows=True, budget=3 * 8 * N * G, **kw)
    for f in FIELDS + TD.ROW_FIELDS:
        _bits_equal(sliced[f], ref[f], f)


def test_bad_noise_entries_p_one_and_per_game_gammas():
    from th_rl_amd.mixed import MixedGameBatch
    config, tabs, tpol, cpol, w, d, K, L = inputs("QR")
    G = tpol.shape[0]
    p = np.random.RandomState(1).uniform(0.02, 0.9, G)
    p[5], p[6], p[7], p[9] = np.nan, 0.0, 1.5, 1.0
    gam = np.repeat(gammas(config)[:, None], G, axis=1) * np.random.RandomState(2).uniform(0.5, 1.0, (2, G))
    mb = MixedGameBatch(config, n_games=G, sweep={"gamma": gam}).init_tables()
    out, ref = _check(mb, config, tabs, tpol, cpol, w, noise_prob=p, gamma=gam, steps=6, dev_len=2)
    bad = [5, 6, 7]
    for f in TD.AGENT_FIELDS + TD.FLOAT_FIELDS + TD.ROW_FIELDS:
        assert (np.asarray(out[f])[..., bad] == 0.0).all(), f
    assert (out["low_step"][bad] == -1).all() and (out["ret_step"][bad] == -1).all()
    assert out["mass"][9] > 0.99 and out["mass"][8] > 0.99 and np.isnan(out["noise_prob"][5])
    one, _ = _check(_batch_of("QR"), config, tabs, tpol, cpol, w, noise_prob=1.0, steps=4, n_games=16)
    assert (one["mass"] > 0.99).all()


def test_band_rows_that_stick_out_of_the_cells():
    """Tables of the caller's: a band wider than the axis, rows that begin before cell 0 and end past cell J - 1."""
    config, tabs, tpol, cpol, w, d, K, L = inputs("QR")
    T, J, W = tabs["n_tuples"], tabs["n_cells"], tabs["band_w"]
    rs = np.random.RandomState(8)
    wide = dict(tabs, band_w=J + 5, band=np.zeros((T, J + 5)), band_lo=np.asarray(tabs["band_lo"]).copy())
    wide["band"][:, :W] = tabs["band"]
    for t, lo in ((0, -2), (7, -J), (13, J - 3), (24, J - 1)):
        wide["band_lo"][t] = lo
        row = rs.uniform(0.0, 1.0, J + 5)
        wide["band"][t] = row / row.sum()
    out, _ = _check(_batch_of("QR"), config, wide, tpol, cpol, w, steps=5, dev_len=2, n_games=16)
    assert (out["mass"] < 1.0 - 1e-6).any()              # mass that a row puts outside [0, J) is lost, as in the mirror


def test_the_weights_a_prefix_of_the_games_and_the_stationary_baseline():
    config, tabs, tpol, cpol, w, d, K, L = inputs("QR")
    mb = _batch_of("QR")
    G, T = tpol.shape[0], tabs["n_tuples"]
    full, _ = _check(mb, config, tabs, tpol, cpol, w, steps=5)
    head, _ = _check(mb, config, tabs, tpol, cpol, w, steps=5, n_games=5)
    for f in FIELDS + TD.ROW_FIELDS:
        _bits_equal(head[f], np.asarray(full[f])[..., :5], f)
    unit = np.zeros((G, T))
    unit[np.arange(G), np.arange(G) % T] = 1.0
    one, ref = _check(mb, config, tabs, tpol, cpol, unit, steps=3)
    R = TD.expected_rewards(tabs, np.full(G, 0.05))
    for g in (0, 11, 69):
        _bits_equal(one["reward_rows"][0, :, g], R[:, g, ref["Dv"][g, g % T]])
    # "stationary": m_0 is thrl_tuple_stationary's pi on the same tables and strategies, and base_reward its stat_reward
    stat, _ = _check(mb, config, tabs, tpol, cpol, "stationary", steps=5)
    want = mb.greedy_stationary(noise_prob=0.05, pi=True, tuple_policy=_device(mb, tpol), cell_policy=_device(mb, cpol), tabs=tabs)
    _bits_equal(stat["base_reward"], want["stat_reward"], "base_reward against stat_reward")
    _bits_equal(stat["base_action"], want["stat_action"], "base_action against stat_action")
    assert np.array_equal(stat["stat_iters"], want["iters"]) and np.array_equal(stat["n_switch"], want["n_switch"])
    _bits_equal(stat["unresolved"], want["unresolved"], "unresolved")
    given, _ = _check(mb, config, tabs, tpol, cpol, want["pi"], steps=5)
    for f in FIELDS + TD.ROW_FIELDS:
        _bits_equal(given[f], stat[f], f)
    assert np.array_equal(given["n_switch"], want["n_switch"])          # the host's count of the same switches
    _bits_equal(given["unresolved"], want["unresolved"], "unresolved on the host")
    # a step limit: the last iterate is the start all the same
    capped, _ = _check(mb, config, tabs, tpol, cpol, "stationary", steps=3, max_iters=3, n_games=8)
    assert (capped["stat_iters"] == 3).all()
    from th_rl_amd._lib import ThrlError
    for bad in ("uniform", None, np.zeros((G, T + 1))):
        with pytest.raises(ThrlError, match="weights"):
            mb.greedy_deviation_noise(noise_prob=0.05, weights=bad, tabs=tabs)


def test_extracted_strategies_equal_the_ones_passed_in():
    from th_rl_amd import tuple_play as tp, tuple_stationary as ts
    config, tabs = inputs("QR")[:2]
    mb = _mixed(config, n_games=32, seed=9, weights_seed=4)
    mb.run(3, per_game_logs=False)
    own = mb.greedy_deviation_noise(noise_prob=0.05, resolution=16, rows=True, steps=6, deviator=1)
    tpol, cpol = tp.extract(mb, tabs), ts.extract_cells(mb, tabs)
    given = mb.greedy_deviation_noise(noise_prob=0.05, rows=True, steps=6, deviator=1, tuple_policy=tpol, cell_policy=cpol,
                                      tabs=tabs)
    for f in FIELDS + TD.ROW_FIELDS + ("stat_iters", "n_switch", "unresolved"):
        _bits_equal(own[f], given[f], f)
    tn, cn = tpol.cpu().numpy().view(np.uint16), cpol.cpu().numpy().view(np.uint16)
    ref = TD.analyse(tabs, tn, cn, 0.05, SM.analyse(tabs, tn, cn, 0.05)["pi"], deviator=1, steps=6, gamma=gammas(config))
    for f in FIELDS + TD.ROW_FIELDS:
        _bits_equal(own[f], ref[f], f)
    assert own["resolution"] == 16 and own["T"] == 25


# ------------------------------------------------------------------------------------------------ geometry
def test_more_games_than_the_grid(base):
    """Game g is a copy of base game g % 5: every output of g equals that of g % 5 byte for byte, with more games than
    one pass of the grid (test_gpu_analysis_geometry's scheme: 8,195 games on 256 CUs), and with one game."""
    import torch
    call = lambda gb: gb.greedy_deviation_noise(noise_prob=0.05, resolution=64, rows=True, steps=6, dev_len=2)
    G = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    ref = call(_geo_batch(base, KB))
    fields = _per_game(call(_geo_batch(base, G)), ref, G, KB)
    assert len(fields) >= 14 and {"gain", "low_step", "reward_rows", "dist_rows", "base_reward"} <= set(fields), sorted(fields)
    for f, (a, b) in sorted(fields.items()):
        a, b = _bytes(a), _bytes(b)
        bad = np.flatnonzero((a != b[np.arange(G) % KB]).any(axis=1))
        assert bad.size == 0, (f, bad[:8])
    one = _per_game(call(_geo_batch(base, 1)), ref, 1, KB)
    assert sorted(one) == sorted(fields)
    for f, (a, b) in one.items():
        assert np.array_equal(_bytes(a)[0], _bytes(b)[0]), f


# ------------------------------------------------------------------------------------------------ the example pairing
def test_example_pairing_after_a_brief_training():
    """QTable against Reinforce in NoisyPriceState(noise_prob=0.05): the batch's own noise, its own strategies, the
    stationary start; the device against the mirror on the extracted strategies."""
    from th_rl_amd import tuple_play as tp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    noisy = dict(QR, environment=dict(ENV, noise_prob=0.05, max_steps=20))
    mb = MixedGameBatch(noisy, n_games=12, seed=5).init_tables()
    mb.run(10, per_game_logs=False)
    out = mb.greedy_deviation_noise(resolution=32, rows=True, steps=8)
    tabs = ts.tables(noisy, 32)
    tn = tp.extract(mb, tabs).cpu().numpy().view(np.uint16)
    cn = ts.extract_cells(mb, tabs).cpu().numpy().view(np.uint16)
    ref = TD.analyse(tabs, tn, cn, 0.05, SM.analyse(tabs, tn, cn, 0.05)["pi"], steps=8, gamma=gammas(noisy))
    for f in FIELDS + TD.ROW_FIELDS:
        _bits_equal(out[f], ref[f], f)
    assert (out["noise_prob"] == 0.05).all() and (out["stat_iters"] > 0).all() and out["n_cells"] == tabs["n_cells"]
    _bits_equal(out["base_reward"], mb.greedy_stationary(resolution=32)["stat_reward"], "base_reward")


# ------------------------------------------------------------------------------------------------ trainer
def test_train_one_noise_artefacts_beside_untouched_noise_free_ones(tmp_path):
    from th_rl_amd import trainer, tuple_analysis as ta, utils
    from th_rl_amd.mixed import MixedGameBatch
    n = 12
    mixed = dict(QR, environment=dict(ENV, max_steps=20))
    runs = {}
    for name, opt in (("plain", {"steps": 8, "dev_len": 2}),
                      ("noise", {"steps": 8, "dev_len": 2, "noise": {"noise_prob": 0.05, "resolution": 32}})):
        cfg = dict(mixed, training={"epochs": 20, "print_freq": 500, "seed": 19, "n_games": n, "n_groups": 2,
                                    "groups": [g % 2 for g in range(n)], "group_stats": {"bins": 64, "histograms": True},
                                    "greedy_deviation": opt})
        (tmp_path / (name + ".json")).write_text(json.dumps(cfg))
        runs[name] = tmp_path / name
        trainer.train_one(str(runs[name]), str(tmp_path / (name + ".json")))
    names = sorted(f.name for f in runs["plain"].iterdir() if f.name.startswith(("gdev", "greedy_deviation")))
    assert "greedy_deviation.json" in names and "gdev_cycle.npy" in names and "gdev1_gain.npy" in names
    assert not any(x.startswith("gdevn") or x == "greedy_deviation_noise.json" for x in names)
    for x in names:        # the noise-free artefacts are byte for byte those of a run without the option
        assert (runs["plain"] / x).read_bytes() == (runs["noise"] / x).read_bytes(), x
    exp = runs["noise"]
    desc = json.load(open(exp / "greedy_deviation_noise.json"))
    T, J = desc["T"], desc["n_cells"]
    assert T == 25 and 32 <= J <= 42
    assert desc["options"]["noise"] == dict(noise_prob=0.05, ret_tol=1e-6, tol=1e-12, max_iters=8192, resolution=32)
    assert [(r["group"], r["deviator"]) for r in desc["summary"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert all(r["games"] == n // 2 == r["solved"] for r in desc["summary"])
    shapes = {"gdevn_prob.npy": ((n,), np.float64), "gdevn_stat.npy": ((2, n), np.int32), "gdevn_unresolved.npy": ((n,), np.float64)}
    for d in (0, 1):
        shapes.update({"gdevn%d_games.npy" % d: ((6, n), np.float64), "gdevn%d_steps.npy" % d: ((2, n), np.int32),
                       "gdevn%d_base.npy" % d: ((2, 2, n), np.float64)})
    have = sorted(f.name for f in exp.iterdir() if f.name.startswith("gdevn"))
    assert set(shapes) <= set(have) and np.load(exp / "gdevn1_mean.npy").shape == (8, 2, 5)     # the response curves
    for x, (shape, dtype) in shapes.items():
        a = np.load(exp / x)
        assert a.shape == shape and a.dtype == dtype, x
    mb = MixedGameBatch(mixed, n_games=n).load(str(exp / "batch.pt"))
    for d in (0, 1):
        g = ta.load_deviation_noise_games(str(exp), d)
        direct = mb.greedy_deviation_noise(deviator=d, steps=8, dev_len=2, noise_prob=0.05, resolution=32)
        for f in FIELDS + ("noise_prob", "stat_iters", "n_switch", "unresolved"):
            _bits_equal(g[f], direct[f], f)
    games = {d: ta.load_deviation_noise_games(str(exp), d) for d in (0, 1)}
    again = ta.summarize_deviation_noise(games, np.arange(n) % 2, 2, [0, 1])
    assert desc["summary"] == json.loads(json.dumps(again))
    df = utils.greedy_deviation_noise_summary(str(exp))
    assert len(df) == 4 and df.loc[0, "n_cells"] == J and df.loc[0, "T"] == 25 and "n_switch_max" in df.columns
    gm = utils.greedy_deviation_noise_games(str(exp), deviator=1)
    assert gm.index.tolist() == list(range(n)) and gm["solved"].all()
    _bits_equal(gm["gain"].to_numpy(), games[1]["gain"])
    curve = utils.group_quantiles(str(exp), 0, "total", prefix="gdevn0")
    assert len(curve) == 8
    with pytest.raises(KeyError, match="training.greedy_deviation.noise"):
        utils.greedy_deviation_noise_summary(str(runs["plain"]))
