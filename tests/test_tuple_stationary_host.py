"""Host side of the stationary analysis in tuple form (th_rl_amd.tuple_stationary, thrl_price_policy,
thrl_tuple_stationary): the per-config tables, the numpy mirror's hand answers, that the random strategies of the device
tests are no degenerate input for it, option parsing and refusals, the summary rows and artefacts, the ctypes mirrors of
the args structs against the header and both entry points' validation through the library loaded without a GPU.
No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tuple_stationary_mirror as SM
from th_rl_amd import stationary as sn, tuple_stationary as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
RF = dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])
MIXED = {"agents": [dict(AG), dict(RF)], "environment": dict(ENV)}
AC = {"agents": [dict(AG), dict(RF, name="ActorCritic", actions=5)], "environment": dict(ENV)}
NN2 = {"agents": [dict(RF, actions=32), dict(RF, name="ActorCritic", actions=21)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.3]),
                    dict(RF, actions=11, action_range=[0.05, 0.25]),
                    dict(RF, name="ActorCritic", actions=5, action_range=[0.0, 0.3])],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
CAC = {"agents": [dict(AG), dict(name="CAC", gamma=0.99, states=1, action_range=[0.2, 0.4])], "environment": dict(ENV)}
FOUR = {"agents": [dict(AG, actions=2), dict(AG, actions=2)], "environment": dict(ENV)}            # T = 4
WIDE = {"agents": [dict(AG, actions=129), dict(RF, actions=32)], "environment": dict(ENV)}         # 4128 tuples
# a market with rewards below 1.3, so that a residual mass of tol moves a reward by less than tol (test_constant_...)
SMALL = {"agents": [dict(AG, actions=2), dict(RF, actions=5)], "environment": dict(ENV, a=2)}
# the configs of the device tests, with the resolution each is run at there: the QTable agents' breakpoints alone
# (about 100 cells), or a coarse uniform grid; (config, T, resolution, seed of the random strategies)
CASES = {"FOUR": (FOUR, 4, 0, 41), "AC": (AC, 105, 0, 42), "THREE": (THREE, 385, 16, 43), "MIXED": (MIXED, 441, 0, 44),
         "NN2": (NN2, 672, 40, 45)}
G = 203


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def random_strategies(tabs, n_games, seed):
    """(tuple_policy uint16 [G, N, T], cell_policy uint16 [G, N, J]) for the device tests: uniform entries over the
    tuples; over the cells a few random runs of one action per agent, as a strategy that is piecewise constant in the
    price has; 2 % of all entries at or above the agent's action count (clamped by the analysis) and game 3's agent 0 at
    65535 throughout."""
    rs = np.random.RandomState(seed)
    T, J, acts = int(tabs["n_tuples"]), int(tabs["n_cells"]), [int(x) for x in tabs["n_actions"]]
    tpol = np.stack([rs.randint(0, A, (n_games, T)) for A in acts], axis=1).astype(np.uint16)
    cpol = np.zeros((n_games, len(acts), J), np.uint16)
    for i, A in enumerate(acts):
        runs = rs.randint(0, A, (n_games, 8))
        edge = np.sort(rs.randint(0, J, (n_games, 7)), axis=1)
        which = (np.arange(J)[None, None, :] >= edge[:, :, None]).sum(axis=1)
        cpol[:, i] = np.take_along_axis(runs, which, axis=1)
    for i, A in enumerate(acts):
        tpol[:, i][rs.rand(n_games, T) < 0.02] += np.uint16(A)
        cpol[:, i][rs.rand(n_games, J) < 0.02] += np.uint16(A)
    if n_games > 3:
        tpol[3, 0, :] = 65535
        cpol[3, 0, :] = 65535
    return tpol, cpol


def _constant(tabs, action):
    T, J, N = tabs["n_tuples"], tabs["n_cells"], len(tabs["n_actions"])
    return np.full((1, N, T), action, np.uint16), np.full((1, N, J), action, np.uint16)


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", sorted(CASES) + ["MIXED-1024"])
def test_tables_are_distributions(name):
    config, T, res, _ = CASES[name] if name in CASES else (MIXED, 441, 1024, 0)
    t = ts.tables(config, res)
    J, W = t["n_cells"], t["band_w"]
    assert t["n_tuples"] == T and t["cuts"].size == J + 1 and t["cuts"][0] == 0.0 and t["cuts"][-1] == 10.0
    assert t["cell_w"].shape == t["cell_x"].shape == (J,) and t["band"].shape == (T, W) and t["band_lo"].shape == (T,)
    assert t["noise_reward"].shape == (len(config["agents"]), T) and t["noise_price"].shape == (T,)
    assert (t["cell_w"] > 0).all() and abs(t["cell_w"].sum() - 1.0) <= J * 2.0 ** -53
    assert ((t["cuts"][:-1] < t["cell_x"]) & (t["cell_x"] < t["cuts"][1:])).all()
    # every redrawn price, those clipped to 0 included, lands in exactly one cell
    assert (t["band"] >= 0).all() and (np.abs(t["band"].sum(axis=1) - 1.0) <= (W + 2) * 2.0 ** -52).all()
    assert (t["band_lo"] >= 0).all() and (t["band_lo"] + 1 <= J).all() and (t["band"][:, 0] > 0).all()
    if name == "MIXED-1024":
        assert J > 1024 and t["resolution"] == 1024


def test_cuts_without_a_grid_are_the_qtable_cuts():
    assert np.array_equal(ts.cuts(TWO, 0), sn.cuts(TWO)) and np.array_equal(ts.tables(TWO, 0)["cuts"], sn.cuts(TWO))
    assert np.array_equal(ts.tables(TWO, 0)["cell_w"], sn.tables(TWO)["cell_w"][:sn.tables(TWO)["n_intervals"]])
    assert np.array_equal(ts.cuts(NN2, 0), [0.0, 10.0]) and np.array_equal(ts.cuts(NN2, 4), [0.0, 2.5, 5.0, 7.5, 10.0])
    # a network has no breakpoints of its own: MIXED's are its QTable agent's
    one = {"agents": [dict(AG)], "environment": dict(ENV, nplayers=1)}
    assert np.array_equal(ts.cuts(MIXED, 0), sn.cuts(one))


def test_too_many_cells_name_the_resolution():
    with pytest.raises(ValueError, match="resolution=4096 gives .* cells, at most 4096"):
        ts.tables(MIXED, 4096)
    assert ts.tables(NN2, 4096)["n_cells"] == 4096
    for bad in (-1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="resolution"):
            ts.cuts(MIXED, bad)


def test_noise_tables_follow_the_formulas():
    t = ts.tables(FOUR, 0)
    # tuple 0: both agents sell 2, u = 4, the redrawn price is uniform on [3, 6]; tuple 3: u = 8, on [-1, 2] clipped at 0
    assert t["price"].tolist() == [6.0, 4.0, 4.0, 2.0]
    assert abs(t["noise_price"][0] - 4.5) < 1e-15 and abs(t["noise_price"][3] - 2.0 * 2.0 / 6.0) < 1e-15
    assert np.allclose(t["noise_reward"][:, 0], [9.0, 9.0]) and np.allclose(t["noise_reward"][:, 3], [8.0 / 3.0] * 2)
    n = np.zeros((4, t["n_cells"]))
    for k in range(4):
        n[k, t["band_lo"][k]:t["band_lo"][k] + t["band_w"]] = t["band"][k][:t["n_cells"] - t["band_lo"][k]]
    c = t["cuts"]
    assert n[0, c[1:] <= 3.0].sum() == 0 and n[0, c[:-1] >= 6.0].sum() == 0 and n[3, c[:-1] >= 2.0].sum() == 0
    assert abs(n[3, 0] - (1.0 + 0.05) / 3.0) < 1e-15                      # the clipped third and the cell [0, 0.05)


# ------------------------------------------------------------------------------------------------ mirror, hand answers
@pytest.mark.parametrize("action", [0, 1, 4])
def test_constant_strategies_under_pure_noise(action):
    """Every agent always plays `action` and every step redraws the price (p = 1): the chain sits on that one tuple.  From
    a unit start elsewhere the lazy step halves the mass outside it, so the run stops with at most tol left there, and
    SMALL's rewards lie within 1.3 of each other: stat_reward is within 2 tol of the tuple's noise reward."""
    t = ts.tables(SMALL, 32)
    tc = min(action, 1) * 5 + min(action, 4)
    assert np.abs(t["noise_reward"]).max() < 1.3
    tpol, cpol = _constant(t, action)
    tol = 1e-12
    for start in (None, [0], [9], [tc], [3]):
        r = SM.analyse(t, tpol, cpol, 1.0, start=start, tol=tol)
        assert 1 <= r["iters"][0] < 64 and r["change"][0] <= tol
        assert abs(r["pi"][0, tc] - 1.0) <= 2 * tol and np.delete(r["pi"][0], tc).sum() <= 2 * tol
        assert (np.abs(r["stat_reward"][:, 0] - t["noise_reward"][:, tc]) <= 2 * tol).all()
        assert abs(r["stat_price"][0] - t["noise_price"][tc]) <= 2 * tol
        assert (np.abs(r["stat_action"][:, 0] - t["scaled"][:, tc]) <= 2 * tol).all()
    assert r["n_switch"][0] == 0 and r["unresolved"][0] == 0.0


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_a_two_cycle_gets_half_and_half(p):
    """F swaps tuples 0 and 3 of FOUR, and the agents play at every price a shock from 0 (3) can reach what they play at
    0's (3's) own price: the chain is the 2-cycle itself, which only the lazy form brings to its Cesaro limit."""
    t = ts.tables(FOUR, 0)
    tpol = np.array([[[1, 0, 1, 0], [1, 0, 1, 0]]], np.uint16)            # F = [3, 0, 3, 0]
    low = t["cell_x"] < 2.5                                               # [0, 2] is reached from 3, [3, 6] from 0
    cpol = np.where(low, 0, 1).astype(np.uint16)[None, None, :].repeat(2, axis=1)
    for start in ([0], [3], [1], None):
        r = SM.analyse(t, tpol, cpol, p, start=start, tol=1e-12, max_iters=500)
        assert r["iters"][0] < 500 and np.abs(r["pi"][0] - [0.5, 0.0, 0.0, 0.5]).max() < 1e-9, (start, r["pi"], r["iters"])
        expect = 0.5 * ((1 - p) * t["reward"][:, 0] + p * t["noise_reward"][:, 0]) \
            + 0.5 * ((1 - p) * t["reward"][:, 3] + p * t["noise_reward"][:, 3])
        assert np.abs(r["stat_reward"][:, 0] - expect).max() < 1e-8
    # the plain iteration m' = s would flip between the two tuples for ever
    F, tau = SM.tuple_of(t, tpol), SM.tuple_of(t, cpol)
    m = np.array([[1.0, 0.0, 0.0, 0.0]])
    new, _ = SM.step(t, F, tau, np.array([p]), np.array([1 - p]), m)
    assert abs((2 * new - m)[0, 3] - 1.0) < 1e-12


def test_one_step_and_refused_games():
    t = ts.tables(FOUR, 0)
    tpol, cpol = random_strategies(t, 6, 3)
    r = SM.analyse(t, tpol, cpol, 0.05, max_iters=1)
    assert r["iters"].tolist() == [1] * 6 and (r["change"] > 0).all()
    r = SM.analyse(t, tpol, cpol, [0.05, np.nan, 0.0, 1.0, 1.5, 0.3], start=[0, 1, 2, 4, 3, -1], max_iters=7)
    assert r["iters"].tolist() == [7, -1, -1, -1, -1, -1]
    assert not r["pi"][1:].any() and not r["stat_reward"][:, 1:].any() and not r["mass"][1:].any()
    assert abs(r["mass"][0] - 1.0) < 1e-15
    # the diagnostics count the neural agents' switches only: FOUR has none, the same arrays read as MIXED's kinds do
    assert not r["n_switch"].any()
    sw, un = SM.switches(t, np.array([[[0] * 50 + [1] * 51, [0] * 101]], np.uint16), kinds=["QTable", "Reinforce"])
    assert sw.tolist() == [0] and un.tolist() == [0.0]
    sw, un = SM.switches(t, np.array([[[0] * 101, [0] * 50 + [1] * 51]], np.uint16), kinds=["QTable", "Reinforce"])
    assert sw.tolist() == [1] and un[0] == 0.5 * (t["cell_w"][49] + t["cell_w"][50])
    sw, un = SM.switches(t, np.array([[[0] * 101, [1] * 50 + [7] * 51]], np.uint16), kinds=["QTable", "Reinforce"])
    assert sw.tolist() == [0]                                             # 7 is clamped to the last action, 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_strategies_carry_the_coverage(name):
    """The inputs the device is compared on are no degenerate chains: in at least half of the games the distribution is
    spread over two tuples or more and some network's sampled action switches."""
    config, T, res, seed = CASES[name]
    t = ts.tables(config, res)
    tpol, cpol = random_strategies(t, G, seed)
    acts = [int(x) for x in t["n_actions"]]
    assert all((tpol[:, i] >= A).any() and (cpol[:, i] >= A).any() for i, A in enumerate(acts))
    r = SM.analyse(t, tpol, cpol, 0.05, max_iters=12)
    assert (r["iters"] == 12).all() and (np.abs(r["mass"] - 1.0) < 1e-12).all()
    assert np.mean((r["pi"] > 1e-6).sum(axis=1) >= 2) >= 0.5
    if name == "FOUR":                                                    # no network: nothing is sampled
        assert not r["n_switch"].any() and not r["unresolved"].any()
    else:
        assert np.mean(r["n_switch"] > 0) >= 0.5 and np.mean(r["unresolved"] > 0) >= 0.5


# ------------------------------------------------------------------------------------------------ options, refusals
def test_parse_options():
    assert ts.parse_options({"noise_prob": 0.05}, MIXED) == dict(ts.DEFAULTS, noise_prob=0.05)
    noisy = dict(MIXED, environment=dict(ENV, noise_prob=0.05))
    assert ts.parse_options(True, noisy) == ts.DEFAULTS
    got = ts.parse_options({"start": "state", "tol": 0, "max_iters": 5, "pi": True, "resolution": 0, "noise_prob": 1}, MIXED)
    assert got == dict(noise_prob=1.0, start="state", tol=0.0, max_iters=5, pi=True, resolution=0)
    swept = dict(MIXED, training={"sweep": {"noise_prob": [0.1, 0.2]}})
    assert ts.parse_options(True, swept)["noise_prob"] is None
    with pytest.raises(ValueError, match="noise_prob = 0: give the noise_prob"):
        ts.parse_options(True, MIXED)
    with pytest.raises(ValueError, match=r"unknown keys \['tables'\]"):
        ts.parse_options({"tables": "final", "noise_prob": 0.05}, MIXED)
    for bad in ({"noise_prob": 0}, {"noise_prob": 1.5}, {"noise_prob": True}, {"start": "tuple"}, {"tol": -1}, {"tol": "x"},
                {"max_iters": 0}, {"max_iters": 1 << 17}, {"max_iters": 2.0}, {"pi": 1}, {"resolution": -1},
                {"resolution": 1.5}, {"resolution": 4096}, 7, "yes"):
        with pytest.raises(ValueError, match="greedy_stationary"):
            ts.parse_options(dict({"noise_prob": 0.05}, **bad) if isinstance(bad, dict) else bad, MIXED)
    with pytest.raises(ValueError, match="continuous"):
        ts.parse_options({"noise_prob": 0.05}, CAC)
    with pytest.raises(ValueError, match="4096"):
        ts.parse_options({"noise_prob": 0.05}, WIDE)


def test_refused_under_launch_and_the_old_check_stands():
    from th_rl_amd import launch
    with pytest.raises(ValueError, match="greedy_stationary is not available under th_rl_amd.launch"):
        launch.check_launch_config(dict(MIXED, training={"n_games": 8, "greedy_stationary": {"noise_prob": 0.05}}))
    launch.check_launch_config(dict(MIXED, training={"n_games": 8, "greedy_stationary": False}))
    with pytest.raises(ValueError, match="follow-up on the mixed path's policy tables"):
        sn.check_config(MIXED)


def test_summary_rows_and_artefacts(tmp_path):
    rs = np.random.RandomState(5)
    n = 6
    g = {"iters": np.array([3, 9, -1, 10, 10, 4], np.int32), "n_switch": np.array([0, 4, 2, 9, 1, 0], np.int32),
         "change": rs.rand(n), "mass": np.ones(n), "stat_price": rs.rand(n), "unresolved": np.array([0, .1, .2, .3, .4, 0]),
         "noise_prob": np.full(n, 0.05), "stat_reward": rs.rand(2, n) + 2.0, "stat_action": rs.rand(2, n)}
    rows = ts.summarize(g, [0, 0, 0, 1, 1, 1], 2, 2.0, 4.0, 10)
    base = sn.summarize(g, [0, 0, 0, 1, 1, 1], 2, 2.0, 4.0, 10)
    for r, b in zip(rows, base):
        assert {k: r[k] for k in b} == b
    assert [(r["n_switch_max"], r["unresolved_max"]) for r in rows] == [(4, 0.2), (9, 0.4)]
    assert abs(rows[0]["unresolved_mean"] - 0.1) < 1e-15 and rows[0]["converged"] == 2.0 / 3.0
    json.dumps(rows)
    ts.save_games(str(tmp_path), g)
    assert sorted(os.listdir(tmp_path)) == ["gstat_action.npy", "gstat_games.npy", "gstat_iters.npy", "gstat_reward.npy"]
    back = ts.load_games(str(tmp_path))
    assert sorted(back) == sorted(g) and all(np.array_equal(back[f], g[f]) for f in g)
    full = dict(g, pi=rs.rand(n, 4), start=np.arange(n, dtype=np.int32))
    ts.save_games(str(tmp_path), full)
    back = ts.load_games(str(tmp_path))
    assert sorted(back) == sorted(full) and all(np.array_equal(back[f], full[f]) for f in full)
    both = ts.combine([{f: (v[:2] if f == "pi" else v[..., :2]) for f, v in full.items()},
                       {f: (v[2:] if f == "pi" else v[..., 2:]) for f, v in full.items()}])
    assert all(np.array_equal(both[f], full[f]) for f in full)
    ts.save_games(str(tmp_path), g)                                       # an earlier run's pi and start do not stay
    assert sorted(ts.load_games(str(tmp_path))) == sorted(g)
    d = ts.describe(dict(ts.DEFAULTS), 101, 441, 2.0, 4.0, rows)
    assert json.loads(json.dumps(d))["T"] == 441 and d["n_cells"] == 101


# ------------------------------------------------------------------------------------------------ the entry points
def _offsets(struct, cname, extra):
    fields = [n for n, _ in struct._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%%zu %s",sizeof(%s),%s);\n' \
          % (" ".join(["%d"] * len(extra)), cname, ",".join(extra))
    for f in fields:
        src += 'printf(" %%zu",offsetof(%s,%s));\n' % (cname, f)
    src += 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    return got, [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_args_structs_match_the_header():
    from th_rl_amd import _lib
    got, mine = _offsets(_lib.PricePolicyArgs, "thrl_price_policy_args", ["THRL_PP_PER_GAME", "THRL_STAT_MAX_CELLS"])
    assert got == mine[:1] + [_lib.PP_PER_GAME, ts.MAX_CELLS] + mine[1:] and ts.MAX_CELLS == 4096
    got, mine = _offsets(_lib.TupleStationaryArgs, "thrl_tuple_stationary_args",
                         ["THRL_TS_START_TUPLE", "THRL_STAT_MAX_ITERS", "THRL_TP_MAX_TUPLES", "THRL_ABI_VERSION"])
    assert got == mine[:1] + [_lib.TS_START_TUPLE, _lib.STAT_MAX_ITERS, 4096, _lib.ABI_VERSION] + mine[1:]
    assert "thrl_price_policy" in _lib.SYMBOLS and "thrl_tuple_stationary" in _lib.SYMBOLS


FAKE = 4096                           # never dereferenced: validation fails before any launch
TS_REQUIRED = ("tuple_policy", "cell_policy", "cell_w", "reward", "scaled", "price", "band_lo", "band", "noise_reward",
               "noise_price", "iters", "change", "mass", "stat_reward", "stat_action", "stat_price")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    return _lib.cfg_from_config(config or TWO, n_games, 0)[0]


def ts_args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleStationaryArgs()
    a.n_games, a.n_tuples, a.n_cells, a.band_w, a.max_iters, a.noise_prob, a.tol = 64, 441, 101, 31, 100, 0.05, 1e-12
    for f in TS_REQUIRED:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k == "kind":
            for i, x in enumerate(v):
                a.kind[i] = x
        else:
            setattr(a, k, v)
    return a


def pp_args(**kw):
    from th_rl_amd import _lib
    a = _lib.PricePolicyArgs()
    a.n_games, a.n_prices, a.price, a.price_policy = 64, 101, FAKE, FAKE
    for k, v in kw.items():
        if k == "kind":
            for i, x in enumerate(v):
                a.kind[i] = x
        else:
            setattr(a, k, v)
    return a


TS_BAD = [dict(n_games=0), dict(n_games=-3), dict(flags=2), dict(flags=-1), dict(n_tuples=0), dict(n_tuples=440),
          dict(n_cells=0), dict(band_w=0), dict(max_iters=0), dict(max_iters=65537), dict(tol=-1e-9), dict(tol=float("nan")),
          dict(noise_prob=0.0), dict(noise_prob=1.5), dict(noise_prob=float("nan")), dict(kind=[0, 4]), dict(kind=[-1, 0]),
          dict(kind=[0, 1], n_tuples=21 * 40)]
PP_BAD = [dict(n_games=0), dict(n_games=65), dict(flags=2), dict(reserved=1), dict(n_prices=0), dict(n_prices=-1),
          dict(kind=[0, 4]), dict(kind=[0, 1])]


def check_validation(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path of both entry points; none of them touches a device."""
    cfg = _cfg()
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})       # a network has at most 32
    for bad in TS_BAD:
        c = forty if bad.get("n_tuples") == 21 * 40 else cfg
        assert lib.thrl_tuple_stationary(ctypes.byref(c), ctypes.byref(ts_args(**bad)), None) == -1, bad
        assert lib.thrl_last_error()
    for bad in PP_BAD:
        c = forty if bad.get("kind") == [0, 1] else cfg
        assert lib.thrl_price_policy(ctypes.byref(c), FAKE, ctypes.byref(pp_args(**bad)), None) == -1, bad
    # a per-game noise array takes the place of the scalar, which is then not read
    assert lib.thrl_tuple_stationary(ctypes.byref(cfg), ctypes.byref(ts_args(noise_prob=0.0, noise_prob_g=FAKE, iters=None)), None) == -2
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097), dict(n_cells=4097)):
        assert lib.thrl_tuple_stationary(ctypes.byref(cfg), ctypes.byref(ts_args(**unsupported)), None) == -3, unsupported
    wide = _cfg({"agents": [dict(AG, actions=129), dict(AG, actions=32)], "environment": dict(ENV)})
    assert lib.thrl_tuple_stationary(ctypes.byref(wide), ctypes.byref(ts_args(n_tuples=4128)), None) == -3
    for unsupported in (dict(kind=[3, 0]), dict(n_prices=4097)):
        assert lib.thrl_price_policy(ctypes.byref(cfg), FAKE, ctypes.byref(pp_args(**unsupported)), None) == -3, unsupported
    # the limits themselves pass the checks: the next refusal is a missing pointer
    big = _cfg({"agents": [dict(AG, actions=128), dict(AG, actions=32)], "environment": dict(ENV)})
    assert lib.thrl_tuple_stationary(ctypes.byref(big), ctypes.byref(ts_args(n_tuples=4096, n_cells=4096, mass=None)), None) == -2
    assert lib.thrl_price_policy(ctypes.byref(cfg), FAKE, ctypes.byref(pp_args(n_prices=4096, price=None)), None) == -2
    for null in TS_REQUIRED:
        assert lib.thrl_tuple_stationary(ctypes.byref(cfg), ctypes.byref(ts_args(**{null: None})), None) == -2, null
    assert lib.thrl_tuple_stationary(ctypes.byref(cfg), ctypes.byref(ts_args(flags=1)), None) == -2
    assert b"start" in lib.thrl_last_error()
    assert lib.thrl_tuple_stationary(ctypes.byref(cfg), None, None) == -2
    assert lib.thrl_tuple_stationary(None, ctypes.byref(ts_args()), None) == -2
    for null in ("price", "price_policy"):
        assert lib.thrl_price_policy(ctypes.byref(cfg), FAKE, ctypes.byref(pp_args(**{null: None})), None) == -2, null
    assert lib.thrl_price_policy(ctypes.byref(cfg), FAKE, None, None) == -2
    assert lib.thrl_price_policy(None, FAKE, ctypes.byref(pp_args()), None) == -2
    assert lib.thrl_price_policy(ctypes.byref(cfg), None, ctypes.byref(pp_args()), None) == -2           # q with a QTable agent
    assert lib.thrl_price_policy(ctypes.byref(cfg), FAKE, ctypes.byref(pp_args(kind=[0, 2])), None) == -2  # its nn_params
    assert b"nn_params[1]" in lib.thrl_last_error()


def test_entry_points_validate_before_any_launch(lib):
    check_validation(lib)
