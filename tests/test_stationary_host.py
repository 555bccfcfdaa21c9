"""Host side of the stationary analysis (thrl_stationary, th_rl_amd/stationary.py), no GPU: the mirror's iteration
against its direct solve, the per-config tables against the CPU oracle's env step, a periodic chain, the entry point's
validation through the library, the args struct against the header, option parsing, the summary, shards and readers."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import deviation_mirror as M
import stationary_mirror as S
from oracle import oracle as O
from th_rl_amd import stationary as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
SMALL = {"agents": [dict(AG, states=20), dict(AG, states=20)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
CLIPPED = {"agents": [dict(AG, actions=6, states=30, action_range=[0.0, 0.5], max_state=8),
                      dict(AG, actions=7, states=25, action_range=[0.0, 0.45], max_state=8),
                      dict(AG, actions=5, states=40, action_range=[0.0, 0.4], max_state=8)],
           "environment": dict(ENV, nplayers=3, max_steps=40)}
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}
# measured on the 64 tables of test_iteration_against_the_direct_solve: 3.66e-10 and 4.62e-10; the bounds are 10 x
# that, for tables other than these
REWARD_BOUND, PI_BOUND = 3.66e-9, 4.62e-9


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the mirror itself
def test_iteration_against_the_direct_solve():
    tabs = sn.tables(CFG)
    pol = S.policies(CFG, S.fresh_tables(CFG, 64, 1))
    it = S.iterate(CFG, tabs, pol, 0.05)
    so = S.solve(CFG, tabs, pol, 0.05)
    dr = np.abs(it["stat_reward"] - so["stat_reward"]).max()
    dp = np.abs(it["pi"] - so["pi"]).sum(axis=1).max()
    print("iters %d .. %d (median %g); max |stat_reward - direct| = %.3e, max L1 |pi - direct| = %.3e; closed classes <= %d"
          % (it["iters"].min(), it["iters"].max(), np.median(it["iters"]), dr, dp, so["classes"].max()))
    assert dr <= REWARD_BOUND and dp <= PI_BOUND
    # what the device tests rest on: every game stops before max_iters
    assert (it["iters"] > 0).all() and (it["iters"] < 8192).all() and (it["change"] <= 1e-12).all()
    assert np.abs(it["mass"] - 1.0).max() <= it["iters"].max() * 103 * 2.0 ** -52


def test_periodic_chain_needs_the_lazy_iteration():
    """p = 1 and a band that sends cell 7 to cell 8 and cell 8 to cell 7: mu P^m alternates for ever, the lazy
    iteration converges to (1/2, 1/2)."""
    tabs = dict(sn.tables(SMALL))
    J, T, W = tabs["n_cells"], tabs["n_tuples"], tabs["band_w"]
    pol = np.zeros((1, 42), np.uint16)
    pol[0, tabs["cell_rows"][0, 8]] = 1                     # cell 8 plays another tuple than cell 7
    tup = S.cell_tuples(SMALL, pol, tabs, 1)[0]
    ta, tb = tup[7], tup[8]
    assert ta != tb
    band, blo = np.zeros((T, W)), np.zeros(T, np.int32)
    band[:, 0] = 1.0
    blo[:] = 7                                              # every other tuple feeds cell 7
    blo[ta] = 8
    tabs.update(band=band, band_lo=blo)
    s0 = np.array([7 * 10.0 / 20])                          # the centre of cell 7 = [3.25, 3.75)
    assert S.start_cells(SMALL, tabs, s0)[0] == 7
    P = S.chain(tabs, tup, 1.0)
    mu = np.eye(J)[7]
    assert (mu @ P)[8] == 1.0 and (mu @ P @ P)[7] == 1.0    # the plain iteration has period 2
    out = S.iterate(SMALL, tabs, pol, 1.0, state0=s0)
    assert 0 < out["iters"][0] < 100
    assert abs(out["pi"][0, 7] - 0.5) <= 1e-12 and abs(out["pi"][0, 8] - 0.5) <= 1e-12 and out["mass"][0] == 1.0
    so = S.solve(SMALL, tabs, pol, 1.0, state0=s0)
    assert so["classes"][0] == 1 and np.abs(so["pi"][0] - out["pi"][0]).sum() <= 1e-12


def test_solve_splits_mass_between_closed_classes():
    P = np.array([[1.0, 0, 0, 0], [0, 0.5, 0.5, 0], [0, 0.25, 0.75, 0], [0.2, 0.3, 0.0, 0.5]])
    classes, trans = S.closed_classes(P)
    assert [c.tolist() for c in classes] == [[0], [1, 2]] and trans.tolist() == [3]
    mu, n = S.limit(P, np.array([0.1, 0.2, 0.3, 0.4]))
    # cell 3 leaves to class {0} with 0.4 and to {1, 2} with 0.6; the stationary vector of {1, 2} is (1/3, 2/3)
    assert n == 2 and np.allclose(mu, [0.1 + 0.16, (0.5 + 0.24) / 3, 2 * (0.5 + 0.24) / 3, 0.0], atol=1e-15)


# ------------------------------------------------------------------------------------------------ tables()
@pytest.mark.parametrize("name", ["CFG", "THREE", "CLIPPED", "BIG"])
def test_tables_rows_and_det_cell(name):
    config = globals()[name]
    tabs = sn.tables(config)
    J, T, W = tabs["n_cells"], tabs["n_tuples"], tabs["band_w"]
    assert tabs["band"].shape == (T, W) and tabs["noise_reward"].shape == (len(config["agents"]), T)
    err = np.abs(tabs["band"].sum(axis=1) - 1.0).max()
    print("%s: J = %d, T = %d, W = %d, max |row sum - 1| = %.3e" % (name, J, T, W, err))
    assert err <= W * 2.0 ** -52 and (tabs["band"] >= 0).all()
    assert (tabs["band_lo"] >= 0).all() and (tabs["band_lo"] < J).all()
    # det_cell against encode64 of the noise-free price
    ag, a, b = M.params(config)
    idx = np.unravel_index(np.arange(T), [p["actions"] for p in ag])
    price, _ = M.env_step([M.scale(idx[i], ag[i]) for i in range(len(ag))], a, b)
    for i, p in enumerate(ag):
        assert tabs["cell_rows"][i][tabs["det_cell"]].tolist() == M.encode(price, p).tolist()
    # the intervals hold the prices that lie on no breakpoint; the point cells follow the intervals, carry no reset
    # weight and no band entry
    c = sn.cuts(config)
    Ji = tabs["n_intervals"]
    inside = (price < a) & ~np.isin(price, c)
    d = np.minimum(tabs["det_cell"], Ji - 1)
    assert (tabs["det_cell"][inside] < Ji).all() and ((c[d] <= price) & (price < c[d + 1]))[inside].all()
    assert (tabs["cell_w"][Ji:] == 0).all() and (S.full_band(tabs)[:, Ji:] == 0).all()
    assert len({tuple(r) for r in tabs["cell_rows"].T.tolist()}) == J
    print("%s: %d point cells" % (name, J - Ji))
    assert (J - Ji > 0) == (name == "THREE")


@pytest.mark.parametrize("name", ["CFG", "CLIPPED"])
def test_band_and_noise_price_against_the_oracle_env_step(name):
    """The oracle's noisy env step at 1,000 equally spaced intercepts (the midpoints of 1,000 equal parts of
    [0.7 a, a)) per tuple.  Shares per cell: a cell's share of the samples differs from its share of the interval by
    less than one sample per end, 2 / 1000.  Mean price: the price is max(0, a' - u), linear in a' but for one kink,
    so the midpoint rule is exact on every part except the one with the kink, where it errs by at most h^2 / 8 with
    h = width / 1000 (the area of the triangle between the chord and the kink); as a mean over the interval that is
    h^2 / (8 width) = width / 8e6, plus 1e-12 for the rounding of 1,000 adds."""
    config = globals()[name]
    tabs = sn.tables(config)
    J, T = tabs["n_cells"], tabs["n_tuples"]
    cfg, _ = O.cfg_from_config(config, 1, 1)
    ag, a, b = M.params(config)
    N = len(ag)
    idx = np.unravel_index(np.arange(T), [p["actions"] for p in ag])
    sc = np.stack([M.scale(idx[i], ag[i]) for i in range(N)], axis=1).copy()        # [T, N]
    width = a - a * 0.7
    inter = a * 0.7 + (np.arange(1000) + 0.5) / 1000.0 * width
    c = sn.cuts(config)
    n = S.full_band(tabs)
    step = O.lib().oracle_env_step
    price, rew = ctypes.c_double(), np.zeros(N)
    pr, pp = rew.ctypes.data_as(ctypes.c_void_p), ctypes.byref(price)
    cref = ctypes.byref(cfg)
    prices = np.zeros((T, 1000))
    clipped = 0
    for t in range(T):
        ps = sc[t].ctypes.data_as(ctypes.c_void_p)
        for m in range(1000):
            step(cref, ps, ctypes.c_int(1), ctypes.c_double(inter[m]), pp, pr)
            prices[t, m] = price.value
    clipped = int((prices == 0.0).sum())
    cells = np.clip(np.searchsorted(c, prices, side="right") - 1, 0, tabs["n_intervals"] - 1)
    share = np.stack([np.bincount(cells[t], minlength=J) for t in range(T)]) / 1000.0
    err = np.abs(share - n).max()
    perr = np.abs(prices.mean(axis=1) - tabs["noise_price"]).max()
    print("%s: max |share - band| = %.4f, max |mean price - noise_price| = %.3e, clipped samples %d"
          % (name, err, perr, clipped))
    assert err <= 2.0 / 1000.0
    assert perr <= width / 8e6 + 1e-12
    assert clipped > 0 or name != "CLIPPED"                 # the clipped prices the second config is there for
    # noise_reward is that price times the agent's quantity
    quantity, u, _, _ = sn.tuple_steps(config)
    assert np.array_equal(tabs["noise_reward"], tabs["noise_price"][None, :] * quantity)


def test_tables_point_cells_and_neural_agents():
    with pytest.raises(ValueError, match="QTable agents only"):
        sn.tables(MIXED)
    # the tuple (0, 0) has the price 10 - 2.5 - 3 = 4.5: agent 0's breakpoint between rows 4 and 5 (4.5 rounds half-even
    # to 4) and agent 1's between rows 13 and 14 (13.5 rounds to 14): the interval below has rows (4, 13), the one above
    # (5, 14), and the price's (4, 14) become a point cell, where the noise-free map goes
    tie = {"agents": [dict(AG, actions=2, states=10, action_range=[0.25, 0.35]),
                      dict(AG, actions=2, states=30, action_range=[0.3, 0.35])], "environment": dict(ENV)}
    tabs = sn.tables(tie)
    k = tabs["det_cell"][0]
    assert k >= tabs["n_intervals"] and tabs["cell_rows"][:, k].tolist() == [4, 14] and tabs["cell_w"][k] == 0.0
    # with agent 1 on 50 states 4.5 is no breakpoint of its grid, and an interval is found
    fine = sn.tables({"agents": [tie["agents"][0], dict(tie["agents"][1], states=50)], "environment": dict(ENV)})
    assert fine["n_cells"] == fine["n_intervals"]


# ------------------------------------------------------------------------------------------------ the entry point
TABLES = ("cell_rows", "cell_w", "det_cell", "band_lo", "band", "noise_reward", "noise_price")
OUTPUTS = ("iters", "change", "mass", "stat_reward", "stat_action", "stat_price")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.StationaryArgs()
    a.n_games, a.n_cells, a.band_w, a.max_iters, a.tol, a.noise_prob = 64, 101, 31, 8192, 1e-12, 0.05
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("policy",) + TABLES + OUTPUTS:
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(n_games=65), dict(flags=4), dict(flags=-1), dict(n_cells=0),
                                 dict(band_w=0), dict(max_iters=0), dict(max_iters=65537), dict(tol=-1e-12),
                                 dict(tol=float("nan")), dict(noise_prob=0.0), dict(noise_prob=1.5),
                                 dict(noise_prob=float("nan")), dict(noise_prob=-0.05)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_stationary(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", ("q", "args", "policy", "state0") + TABLES + OUTPUTS)
def test_missing_pointers_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    kw = dict(flags=_lib.STAT_START_STATE) if null == "state0" else ({} if null in ("q", "args") else {null: None})
    a = None if null == "args" else ctypes.byref(_args(**kw))
    assert lib.thrl_stationary(ctypes.byref(cfg), q, a, None) == -2


def test_flags_limits_and_n_tuples(lib):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    call = lambda a, q=None: lib.thrl_stationary(ctypes.byref(cfg), q, ctypes.byref(a), None)
    t = ctypes.c_int32(-1)
    assert call(_args(n_tuples=ctypes.pointer(t))) == -2 and b"q is NULL" in lib.thrl_last_error() and t.value == 441
    given = _args(flags=_lib.STAT_POLICY_GIVEN, mass=None)
    assert call(given) == -2 and b"q is NULL" not in lib.thrl_last_error() and b"mass" in lib.thrl_last_error()
    # a per-game array replaces the scalar, which is then not read
    assert call(_args(noise_prob=0.0, noise_prob_g=4096)) == -2 and b"q is NULL" in lib.thrl_last_error()
    # the limits: cells, and LDS (18 J + 512 (2 N + 2) bytes against 64 KB: J = 3,001 fits, 3,500 does not)
    q = ctypes.c_void_p(4096)
    assert call(_args(n_cells=4097), q) == _lib.ERR_UNSUPPORTED and b"4096" in lib.thrl_last_error()
    assert call(_args(n_cells=3500), q) == _lib.ERR_UNSUPPORTED and b"LDS" in lib.thrl_last_error()
    # J = 3,001 passes the limits: the call gets as far as the NULL check that follows them (nothing is launched)
    assert call(_args(n_cells=3001, mass=None), q) == -2 and b"mass" in lib.thrl_last_error()
    assert call(_args(n_cells=3500, mass=None), q) == _lib.ERR_UNSUPPORTED
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}       # 4,160 tuples
    wcfg, _ = _lib.cfg_from_config(wide, 64, 0)
    assert lib.thrl_stationary(ctypes.byref(wcfg), q, ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    fields = ("noise_prob", "tol", "noise_prob_g", "policy", "band", "n_tuples", "iters", "pi")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %d %d %d %d %d"'
           + "".join(' " %zu"' for _ in fields) + ',sizeof(thrl_stationary_args),THRL_STAT_POLICY_GIVEN,THRL_STAT_START_STATE,'
           'THRL_STAT_MAX_CELLS,THRL_STAT_MAX_ITERS,THRL_ABI_VERSION' + "".join(",offsetof(thrl_stationary_args,%s)" % f for f in fields)
           + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    want = [ctypes.sizeof(_lib.StationaryArgs), _lib.STAT_POLICY_GIVEN, _lib.STAT_START_STATE, _lib.STAT_MAX_CELLS,
            _lib.STAT_MAX_ITERS, 4]
    assert got == want + [getattr(_lib.StationaryArgs, f).offset for f in fields]
    assert "thrl_stationary" in _lib.SYMBOLS


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_and_refusals():
    noisy = dict(CFG, environment=dict(ENV, noise_prob=0.05))
    assert sn.parse_options(True, noisy) == sn.DEFAULTS
    got = sn.parse_options({"noise_prob": 0.01, "start": "state", "tol": 0, "max_iters": 100, "pi": True,
                            "tables": "converged"}, CFG)
    assert got == dict(noise_prob=0.01, start="state", tol=0.0, max_iters=100, pi=True, tables="converged")
    with pytest.raises(ValueError, match="noise_prob = 0"):
        sn.parse_options(True, CFG)                       # a noise-free run must say which noise to analyse
    assert sn.parse_options(True, dict(CFG, training={"sweep": {"noise_prob": [0.1]}}))["noise_prob"] is None
    for bad in ({"noise_prob": 0}, {"noise_prob": 1.5}, {"noise_prob": "x"}, {"noise_prob": True}, {"start": "x0"},
                {"tol": -1}, {"tol": "a"}, {"max_iters": 0}, {"max_iters": 65537}, {"max_iters": 1.5}, {"pi": 1},
                {"tables": "best"}, {"policies": True}, 5, "yes"):
        with pytest.raises(ValueError):
            sn.parse_options(bad, noisy)
    with pytest.raises(ValueError, match="QTable agents only"):
        sn.parse_options(True, MIXED)


# ------------------------------------------------------------------------------------------------ summary, shards
def _games(G=10):
    rs = np.random.RandomState(4)
    g = dict(iters=rs.randint(50, 900, G).astype(np.int32), change=rs.uniform(0, 1e-12, G), mass=np.ones(G),
             stat_price=rs.uniform(3, 5, G), stat_reward=rs.uniform(10, 12.5, (2, G)), stat_action=rs.uniform(0.2, 0.4, (2, G)),
             noise_prob=np.full(G, 0.05))
    g["iters"][3] = 8192
    g["iters"][4] = -1
    return g


def test_summary_arithmetic():
    g = _games()
    ids = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1])
    nash, cartel = sn.optimal(CFG)
    rr = np.random.RandomState(5).uniform(10, 12.5, (2, 10))
    rows = sn.summarize(g, ids, 3, nash, cartel, 8192, reset_reward=rr)
    assert [r["games"] for r in rows] == [5, 5, 0]
    assert rows[0]["converged"] == 3 / 5 and rows[1]["converged"] == 1.0 and rows[2]["converged"] is None
    delta = (g["stat_reward"][0] + g["stat_reward"][1] - nash) / (cartel - nash)
    solved0 = [0, 1, 2, 3]
    assert rows[0]["delta_noise_mean"] == float(delta[solved0].mean())
    assert rows[0]["delta_noise_q50"] == float(np.quantile(delta[solved0], 0.5))
    assert rows[0]["iters_max"] == 8192 and rows[0]["iters_q50"] == float(np.quantile(g["iters"][solved0], 0.5))
    assert rows[0]["price_mean"] == float(g["stat_price"][solved0].mean())
    dreset = (rr[0] + rr[1] - nash) / (cartel - nash)
    assert rows[1]["delta_reset_mean"] == float(dreset[5:].mean())
    assert rows[1]["noise_cost_mean"] == float((dreset[5:] - delta[5:]).mean())
    assert rows[2]["delta_noise_mean"] is None and rows[2]["iters_max"] is None
    assert "noise_cost_mean" not in sn.summarize(g, ids, 3, nash, cartel, 8192)[0]
    json.dumps(rows)


def test_shards_combine_to_the_unsharded_run_and_readers(tmp_path):
    from th_rl_amd import utils
    g = dict(_games(), pi=np.random.RandomState(6).uniform(0, 1, (10, 7)))
    ids = np.arange(10) % 2
    nash, cartel = sn.optimal(CFG)
    rr = np.random.RandomState(5).uniform(10, 12.5, (2, 10))
    cut = lambda x, lo, hi, f: x[lo:hi] if f == "pi" else x[..., lo:hi]
    for r, (lo, hi) in enumerate(((0, 4), (4, 10))):
        d = tmp_path / ("shard%d" % r)
        d.mkdir()
        part = {f: cut(np.asarray(v), lo, hi, f) for f, v in g.items()}
        sn.save_games(str(d), part)
        np.save(d / "attr_reset_reward.npy", rr[:, lo:hi])
        (d / "shard_config.json").write_text(json.dumps({"training": {"game_offset": lo}}))
        summ = sn.summarize(part, ids[lo:hi], 2, nash, cartel, 8192, reset_reward=rr[:, lo:hi])
        sn.save_json(str(d / "stationary.json"), sn.describe(dict(sn.DEFAULTS), 7, nash, cartel, summ))
    both = sn.combine(sn.load_games(str(tmp_path / ("shard%d" % r))) for r in range(2))
    assert set(both) == set(g)
    for f in g:
        assert np.array_equal(both[f], g[f]), f
    assert sn.summarize(both, ids, 2, nash, cartel, 8192) == sn.summarize(g, ids, 2, nash, cartel, 8192)
    # the readers: per game from the shards, the summary from a merged directory
    gm = utils.stationary_games(str(tmp_path))
    assert gm.index.tolist() == list(range(10)) and gm["iters"].tolist() == g["iters"].tolist()
    assert np.array_equal(gm["delta_noise"].to_numpy(), sn.profit_gain(g["stat_reward"], nash, cartel))
    assert np.array_equal(gm["delta_reset"].to_numpy(), sn.profit_gain(rr, nash, cartel))
    sn.save_games(str(tmp_path), both)
    sn.save_json(str(tmp_path / "stationary.json"),
                 sn.describe(dict(sn.DEFAULTS), 7, nash, cartel, sn.summarize(both, ids, 2, nash, cartel, 8192)))
    df = utils.stationary_summary(str(tmp_path))
    assert df["games"].tolist() == [5, 5] and df["n_cells"].tolist() == [7, 7] and df.loc[0, "Nash"] == nash
    assert utils.stationary_games(str(tmp_path)).index.tolist() == list(range(10))
    with pytest.raises(KeyError):
        utils.stationary_games(str(tmp_path / "shard0" / "none"))
