"""The equilibrium check under demand noise in tuple form on the device (thrl_tuple_equilibrium_noise,
greedy_equilibrium_noise(), the option "noise" of training.greedy_equilibrium): every output, the per-state arrays
included, bit-equal to the numpy mirror (tests/tuple_equilibrium_noise_mirror.py) on random strategies for a QTable
against a Reinforce agent (T = 25, 24 cells: most lanes idle, 70 games), 9 x 9 actions at resolution 100 (T = 81 and
J both past one 64-lane chunk and no multiple of it), three agents with an ActorCritic among them, and a working set
above the 64 KB a block gets by default; per-game noise
probabilities and discount factors with bad entries, the sweep cap, a zero tolerance, band rows that stick out of the
cells, one agent alone, a game count below the batch's, every kind of weights, extracted strategies, more games than the
grid, and the trainer's artefacts.

The random strategies carry the coverage: tests/test_tuple_equilibrium_noise_host.py asserts on the mirror, and the
first test here again, that policy iteration runs for two rounds or more and changes actions in the cells."""
import json

import numpy as np
import pytest

import tuple_equilibrium_noise_mirror as TM
import tuple_stationary_mirror as SM
from test_gpu_analysis_geometry import CONFIG as GEO, K, _batch as _geo_batch, _bytes, _per_game, base  # noqa: F401
from test_gpu_tuple_attractors import ENV, _bits_equal, _device, _mixed
from test_tuple_equilibrium_noise_host import CASES, QR, gammas, strategies

pytestmark = pytest.mark.gpu

INT, FLOAT, WEIGHTED, STATE = TM.INT_FIELDS, TM.FLOAT_FIELDS, TM.W_FIELDS, TM.STATE_FIELDS
_CASE = {}


def _case(name):
    """(config, batch, tabs, tuple_policy, cell_policy, pi) of a case, made once: pi [G, T] are random distributions."""
    from th_rl_amd import tuple_stationary as ts
    if name not in _CASE:
        config, T, res, G, seed = CASES[name]
        tabs = ts.tables(config, res)
        tpol, cpol = strategies(tabs, G, seed)
        pi = np.random.RandomState(seed).uniform(0.0, 1.0, (G, T))
        _CASE[name] = (config, _mixed(config, n_games=G), tabs, tpol, cpol, pi / pi.sum(axis=1, keepdims=True))
    return _CASE[name]


def _check(mb, config, tabs, tpol, cpol, noise_prob=0.05, weights=None, gamma=None, **kw):
    """greedy_equilibrium_noise(policies=True, ...) on the given strategies against the mirror: (device, mirror)."""
    n = kw.get("n_games") or tpol.shape[0]
    if weights is not None and not isinstance(weights, str):
        weights = np.ascontiguousarray(weights[:n])
    out = mb.greedy_equilibrium_noise(noise_prob=noise_prob, policies=True, weights=weights, tuple_policy=_device(mb, tpol),
                                      cell_policy=_device(mb, cpol[:n]), tabs=tabs, **kw)
    pi = out["pi"] if isinstance(weights, str) else weights
    ref = TM.analyse(tabs, tpol, cpol, noise_prob if np.ndim(noise_prob) == 0 else np.asarray(noise_prob)[:n],
                     agents=kw.get("agents"), gamma=gammas(config) if gamma is None else gamma, pi=pi,
                     eval_tol=kw.get("eval_tol", 1e-12), max_sweeps=kw.get("max_sweeps", 8192), n_games=kw.get("n_games"))
    sel = out["agents"]
    for f in INT + FLOAT + STATE + (WEIGHTED if pi is not None else ()):
        _bits_equal(np.asarray(out[f])[sel], np.asarray(ref[f])[sel], f)
    assert (pi is not None) == ("loss_w" in out)
    assert out["n_cells"] == tabs["n_cells"] and out["T"] == tabs["n_tuples"] and out["n_states"] == out["T"] + out["n_cells"]
    return out, ref


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", ["QR", "NINE", "TRIO"])
def test_random_strategies_equal_mirror(name):
    config, mb, tabs, tpol, cpol, pi = _case(name)
    out, ref = _check(mb, config, tabs, tpol, cpol, weights=pi)
    # policy iteration really runs, and no (agent, game) is capped: held on the mirror
    assert (ref["iters"] >= 0).all() and (ref["iters"] >= 2).any() and (ref["n_diff_cells"] > 0).any()
    assert out["br_policy"].dtype == np.uint16 and out["br_policy"].shape == (mb.N, mb.G, out["n_states"])
    assert np.array_equal(out["br_all"], out["loss_all"] <= 0.0) and out["perfect"].shape == (mb.G,)
    print("%s: T %d, J %d, rounds %d..%d, sweeps <= %d" % (name, out["T"], out["n_cells"], ref["iters"].min(),
                                                           ref["iters"].max(), ref["sweeps"].max()))


def test_bad_noise_entries_p_one_and_a_discount_factor_of_one():
    from th_rl_amd.mixed import MixedGameBatch
    config, _, tabs, tpol, cpol, pi = _case("QR")
    G = tpol.shape[0]
    p = np.random.RandomState(1).uniform(0.02, 0.9, G)
    p[5], p[6], p[7], p[9] = np.nan, 0.0, 1.5, 1.0
    gam = np.repeat(gammas(config)[:, None], G, axis=1)
    gam[0, 11], gam[1, 12], gam[1, 13] = 1.0, -0.25, np.nan
    mb = MixedGameBatch(config, n_games=G, sweep={"gamma": gam}).init_tables()
    out, ref = _check(mb, config, tabs, tpol, cpol, noise_prob=p, weights=pi, gamma=gam)
    bad = np.zeros(G, bool)
    bad[[5, 6, 7]] = True
    for f in INT + FLOAT + WEIGHTED + STATE:                 # zeros with iters = -1, the neighbours untouched
        assert (np.asarray(out[f])[:, bad] == (-1 if f == "iters" else 0)).all(), f
    ok = np.ones((2, G), bool)
    ok[:, bad] = False
    ok[0, 11] = ok[1, 12] = ok[1, 13] = False
    assert (out["iters"][ok] >= 0).all() and (out["iters"][~ok] == -1).all() and out["iters"][:, 9].min() >= 0
    for i, g in ((0, 11), (1, 12), (1, 13)):                 # the NaN rule: nothing swept, br_policy = pi_i
        assert np.isnan(out["loss_all"][i, g]) and np.isnan(out["v_w"][i, g]) and np.isnan(out["v_opt"][i, g]).all()
        assert out["sweeps"][i, g] == 0 and out["n_diff_tuples"][i, g] == 0 and out["iters"][1 - i, g] >= 0
        assert np.array_equal(out["br_policy"][i, g], ref["br_policy"][i, g])


def test_sweep_cap_and_zero_tolerance():
    config, mb, tabs, tpol, cpol, pi = _case("QR")
    out, _ = _check(mb, config, tabs, tpol, cpol, weights=pi, eval_tol=0.0, max_sweeps=1)
    assert (out["iters"] == -1).all() and (out["sweeps"] == 1).all() and np.isnan(out["loss_cells_mean"]).all()
    # eval_tol = 0: the margin is 0 and an evaluation ends at an iterate that reproduces itself bit for bit
    out, ref = _check(mb, config, tabs, tpol, cpol, weights=pi, eval_tol=0.0, max_sweeps=4096, n_games=24)
    assert float(TM.margin_of(0.9, 0.0)) == 0.0 and (ref["iters"] >= 0).any() and (ref["sweeps"][ref["iters"] >= 0] < 4096 * 65).all()
    print("eval_tol 0: solved %d of %d, sweeps <= %d" % ((ref["iters"] >= 0).sum(), ref["iters"].size, ref["sweeps"].max()))


def test_band_rows_that_stick_out_of_the_cells():
    """Tables of the caller's: a band wider than the axis, rows that begin before cell 0 and end past cell J - 1."""
    config, mb, tabs, tpol, cpol, pi = _case("QR")
    T, J, W = tabs["n_tuples"], tabs["n_cells"], tabs["band_w"]
    rs = np.random.RandomState(8)
    wide = dict(tabs, band_w=J + 5, band=np.zeros((T, J + 5)), band_lo=np.asarray(tabs["band_lo"]).copy())
    wide["band"][:, :W] = tabs["band"]
    for t, lo in ((0, -2), (7, -J), (13, J - 3), (24, J - 1)):
        wide["band_lo"][t] = lo
        row = rs.uniform(0.0, 1.0, J + 5)
        wide["band"][t] = row / row.sum()
    out, ref = _check(mb, config, wide, tpol, cpol, weights=pi, n_games=16)
    assert (ref["iters"] >= 0).all()


def test_working_set_above_64_kb():
    """21 x 21 actions at resolution 1500: more LDS than a block gets by default, so the launch raises the kernel's limit
    first.  gamma = 0.5 keeps an evaluation at some 40 sweeps."""
    from th_rl_amd import tuple_stationary as ts
    half = {"agents": [dict(QR["agents"][0], actions=21, states=100, gamma=0.5), dict(QR["agents"][1], actions=21, gamma=0.5)],
            "environment": dict(ENV)}
    tabs = ts.tables(half, 1500)
    T, J = tabs["n_tuples"], tabs["n_cells"]
    assert T == 441 and 64 * 1024 < 44 * T + 28 * J + 2048 <= 160 * 1024
    tpol, cpol = strategies(tabs, 2, 61)
    pi = np.full((2, T), 1.0 / T)
    out, ref = _check(_mixed(half, n_games=2), half, tabs, tpol, cpol, weights=pi)
    assert (ref["iters"] >= 1).all() and ref["sweeps"].max() < 1000


def test_one_agent_a_prefix_of_the_games_and_the_weights():
    from th_rl_amd import tuple_stationary as ts
    config, mb, tabs, tpol, cpol, pi = _case("TRIO")
    G, N = tpol.shape[0], 3
    full, _ = _check(mb, config, tabs, tpol, cpol, weights=pi)
    last, _ = _check(mb, config, tabs, tpol, cpol, weights=pi, agents=[N - 1])
    for f in INT + FLOAT + WEIGHTED + STATE:
        _bits_equal(last[f][N - 1], full[f][N - 1], f)
        assert not np.asarray(last[f])[:N - 1].any(), f        # rows of agents not solved are not written
    head, _ = _check(mb, config, tabs, tpol, cpol, weights=pi[:5], n_games=5)
    for f in INT + FLOAT + WEIGHTED + STATE:
        _bits_equal(head[f], np.asarray(full[f])[:, :5], f)
    none, _ = _check(mb, config, tabs, tpol, cpol, weights=None)
    for f in INT + FLOAT + STATE:
        _bits_equal(none[f], full[f], f)
    assert "br_w" not in none and "pi" not in none
    # "stationary": the long-run distribution of thrl_tuple_stationary on the same tables and strategies
    stat, _ = _check(mb, config, tabs, tpol, cpol, weights="stationary")
    want = mb.greedy_stationary(noise_prob=0.05, pi=True, tuple_policy=_device(mb, tpol), cell_policy=_device(mb, cpol),
                                tabs=tabs)["pi"]
    _bits_equal(stat["pi"], want, "pi")
    _bits_equal(stat["pi"], SM.analyse(tabs, tpol, cpol, 0.05)["pi"], "pi against its mirror")
    assert (np.abs(stat["diff_w"]) <= 1.0 + 1e-12).all() and "br_w" in stat


def test_extracted_strategies_equal_the_ones_passed_in():
    from th_rl_amd import tuple_play as tp, tuple_stationary as ts
    config, _, tabs, _, _, _ = _case("QR")
    mb = _mixed(config, n_games=32, seed=9, weights_seed=4)
    mb.run(3, per_game_logs=False)
    own = mb.greedy_equilibrium_noise(noise_prob=0.05, resolution=16, policies=True)
    tpol, cpol = tp.extract(mb, tabs), ts.extract_cells(mb, tabs)
    given = mb.greedy_equilibrium_noise(noise_prob=0.05, policies=True, tuple_policy=tpol, cell_policy=cpol, tabs=tabs)
    for f in INT + FLOAT + WEIGHTED + STATE + ("pi",):
        _bits_equal(own[f], given[f], f)
    ref = TM.analyse(tabs, tpol.cpu().numpy().view(np.uint16), cpol.cpu().numpy().view(np.uint16), 0.05,
                     gamma=gammas(config), pi=own["pi"])
    for f in INT + FLOAT + WEIGHTED + STATE:
        _bits_equal(own[f], ref[f], f)
    assert own["resolution"] == 16 and (own["iters"] >= 0).all()


# ------------------------------------------------------------------------------------------------ geometry
def test_more_games_than_the_grid(base):
    """Game g is a copy of base game g % K: every output of g equals that of g % K byte for byte, with more games than
    one pass of the grid (test_gpu_analysis_geometry's scheme), and with one game."""
    import torch
    call = lambda gb: gb.greedy_equilibrium_noise(noise_prob=0.05, resolution=64, policies=True)
    G = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    ref = call(_geo_batch(base, K))
    fields = _per_game(call(_geo_batch(base, G)), ref, G, K)
    assert len(fields) >= 12 and {"iters", "loss_w", "v_opt", "br_policy", "pi"} <= set(fields), sorted(fields)
    for f, (a, b) in sorted(fields.items()):
        a, b = _bytes(a), _bytes(b)
        bad = np.flatnonzero((a != b[np.arange(G) % K]).any(axis=1))
        assert bad.size == 0, (f, bad[:8])
    one = _per_game(call(_geo_batch(base, 1)), ref, 1, K)
    assert sorted(one) == sorted(fields)
    for f, (a, b) in one.items():
        assert np.array_equal(_bytes(a)[0], _bytes(b)[0]), f


# ------------------------------------------------------------------------------------------------ trainer
def test_train_one_noise_artefacts_beside_untouched_noise_free_ones(tmp_path):
    from th_rl_amd import trainer, tuple_analysis as ta, utils
    from th_rl_amd.mixed import MixedGameBatch
    n = 12
    mixed = dict(QR, environment=dict(ENV, max_steps=20))
    runs = {}
    for name, opt in (("plain", {"policies": True}),
                      ("noise", {"noise": {"noise_prob": 0.05, "resolution": 32}, "policies": True})):
        cfg = dict(mixed, training={"epochs": 20, "print_freq": 500, "seed": 19, "n_games": n, "n_groups": 2,
                                    "groups": [g % 2 for g in range(n)], "greedy_equilibrium": opt})
        (tmp_path / (name + ".json")).write_text(json.dumps(cfg))
        runs[name] = tmp_path / name
        trainer.train_one(str(runs[name]), str(tmp_path / (name + ".json")))
    names = sorted(f.name for f in runs["plain"].iterdir() if f.name.startswith(("geq", "greedy_equilibrium")))
    assert "greedy_equilibrium.json" in names and "geq_policy.npy" in names
    assert not any(x.startswith("geqn_") or x == "greedy_equilibrium_noise.json" for x in names)
    for x in names:        # the noise-free artefacts are byte for byte those of a run without the option
        assert (runs["plain"] / x).read_bytes() == (runs["noise"] / x).read_bytes(), x
    exp = runs["noise"]
    desc = json.load(open(exp / "greedy_equilibrium_noise.json"))
    T, J = desc["T"], desc["n_cells"]
    assert T == 25 and 32 <= J <= 42 and desc["options"]["noise"] == dict(noise_prob=0.05, eval_tol=1e-12, max_sweeps=8192,
                                                                           resolution=32)
    assert [(r["group"], r["agent"]) for r in desc["summary"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [(r["group"], r["agent"]) for r in desc["perfect"]] == [(0, None), (1, None)]
    assert all(r["games"] == n // 2 for r in desc["summary"] + desc["perfect"]) and all(r["capped"] == 0 for r in desc["summary"])
    shapes = {"geqn_iters.npy": ((4, 2, n), np.int32), "geqn_loss.npy": ((3, 2, n), np.float64),
              "geqn_prob.npy": ((n,), np.float64), "geqn_weighted.npy": ((3, 2, n), np.float64),
              "geqn_policy.npy": ((2, n, T + J), np.uint16), "geqn_v_opt.npy": ((2, n, T + J), np.float64),
              "geqn_v_pi.npy": ((2, n, T + J), np.float64)}
    assert sorted(f.name for f in exp.iterdir() if f.name.startswith("geqn_")) == sorted(shapes)
    for x, (shape, dtype) in shapes.items():
        a = np.load(exp / x)
        assert a.shape == shape and a.dtype == dtype, x
    g = ta.load_equilibrium_noise_games(str(exp))
    mb = MixedGameBatch(mixed, n_games=n).load(str(exp / "batch.pt"))
    direct = mb.greedy_equilibrium_noise(noise_prob=0.05, resolution=32, policies=True)
    for f in INT + FLOAT + WEIGHTED + STATE + ("noise_prob",):
        _bits_equal(g[f], direct[f], f)
    again = ta.summarize_equilibrium_noise(g, np.arange(n) % 2, 2, [0, 1], 0.0)
    assert desc["summary"] + desc["perfect"] == json.loads(json.dumps([r for r in again if r["agent"] is not None]
                                                                      + [r for r in again if r["agent"] is None]))
    df = utils.greedy_equilibrium_noise_summary(str(exp))
    assert len(df) == 6 and df.loc[0, "n_cells"] == J and df.loc[0, "T"] == 25
    gm = utils.greedy_equilibrium_noise_games(str(exp), agent=1)
    assert gm.index.tolist() == list(range(n)) and gm["n_diff_cells"].tolist() == direct["n_diff_cells"][1].tolist()
    _bits_equal(gm["loss_w"].to_numpy(), g["loss_w"][1])
