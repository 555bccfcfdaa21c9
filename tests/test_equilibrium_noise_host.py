"""Host side of the equilibrium check under demand noise (thrl_equilibrium_noise, th_rl_amd/equilibrium.py), no GPU:
the mirror against independent solves (the dense chain with numpy.linalg.solve, plain value iteration), the known
answers through hand-written policies, the cap as a condition on the mirror, the entry point's validation through the
library, the args struct against the header, option parsing, the summary, shards, the merge and the readers."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import equilibrium_mirror as E
import equilibrium_noise_mirror as EN
import stationary_mirror as S
from th_rl_amd import equilibrium as eq
from th_rl_amd import stationary as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
NOISY = dict(CFG, environment=dict(ENV, noise_prob=0.05))
SMALL = {"agents": [dict(AG, states=20), dict(AG, states=20, gamma=0.9)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}
SHAPES = {"SMALL": SMALL, "TWO": CFG, "THREE": THREE}
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the mirror itself
@pytest.mark.parametrize("gamma,eval_tol", [(0.9, 1e-12), (0.95, 1e-12), (0.95, 1e-9), (0.99, 1e-9)])
@pytest.mark.parametrize("shape", ["SMALL", "TWO", "THREE"])
def test_mirror_against_independent_solves(shape, gamma, eval_tol):
    """Random strategies, 12 (agent, game) solves per shape (6 at gamma = 0.99).  V_pi against (I - gamma P)^-1 R on the
    dense chain, V* against value iteration run far past convergence.

    Bounds.  e = EN.error_bound: gamma / (1 - gamma) * eval_tol of truncation plus (W + 3) u max|V| / (1 - gamma) of
    rounding (derived there).  V_pi: e.  V*: the iteration stops when no action's Q exceeds the incumbent's by more than
    margin, both Q within gamma e of the true ones, so the last strategy's Bellman residual is at most d = margin +
    2 gamma e and its value within d / (1 - gamma) of the optimum: e + d / (1 - gamma)."""
    config = SHAPES[shape]
    tabs = sn.tables(config)
    pl = E.plan(config)
    N, W = pl["N"], tabs["band_w"]
    G = (12 if gamma < 0.99 else 6) // N                   # gamma = 0.99 takes five times the sweeps
    pol = S.policies(config, S.fresh_tables(config, G, 3))
    gam = np.full((N, G), gamma)
    out = EN.analyse(config, tabs, pol, 0.05, gamma=gam, eval_tol=eval_tol)
    # the cap is a condition of every test that follows, not a measurement
    assert (out["iters"] >= 0).all() and out["iters"].max() <= 8
    tup = S.cell_tuples(config, pol, tabs, G)
    worst_pi = worst_opt = 0.0
    for g in range(G):
        for i in range(N):
            R, P, pk = EN.dense(pl, tabs, tup[g], i, 0.05)
            vd = EN.direct_value(R, P, pk, gamma)
            vi = EN.value_iteration(R, P, gamma)
            vmax = np.abs(vi).max()
            e = EN.error_bound(gamma, eval_tol, W, vmax)
            d = float(EN.margin_of(gamma, eval_tol)) + 2.0 * gamma * e
            err_pi = np.abs(out["v_pi"][i, g] - vd).max()
            err_opt = np.abs(out["v_opt"][i, g] - vi).max()
            worst_pi, worst_opt = max(worst_pi, err_pi / e), max(worst_opt, err_opt / (e + d / (1.0 - gamma)))
            assert err_pi <= e, (g, i, err_pi, e)
            assert err_opt <= e + d / (1.0 - gamma), (g, i, err_opt)
            # the best response found is one: value iteration's greedy strategy has the same value up to the bound
            assert (out["v_opt"][i, g] >= out["v_pi"][i, g] - 2 * e).all()
    print("%s gamma %g eval_tol %g: rounds <= %d, sweeps <= %d, max |V_pi - direct| / bound = %.3f, max |V* - VI| / bound = %.3f"
          % (shape, gamma, eval_tol, out["iters"].max(), out["sweeps"].max(), worst_pi, worst_opt))


def test_headline_defaults_observed_error():
    """The headline grid at the defaults (p = 0.05, gamma = 0.95, eval_tol = 1e-12), 8 games: the figure DESIGN.md
    records."""
    tabs, pl = sn.tables(CFG), E.plan(CFG)
    pol = S.policies(CFG, S.fresh_tables(CFG, 8, 1))
    out = EN.analyse(CFG, tabs, pol, 0.05)
    tup = S.cell_tuples(CFG, pol, tabs, 8)
    worst = bound = 0.0
    for g in range(8):
        for i in range(2):
            R, P, pk = EN.dense(pl, tabs, tup[g], i, 0.05)
            vd = EN.direct_value(R, P, pk, 0.95)
            worst = max(worst, np.abs(out["v_pi"][i, g] - vd).max())
            bound = max(bound, EN.error_bound(0.95, 1e-12, tabs["band_w"], np.abs(vd).max()))
    print("max |V_pi - direct| = %.3e: truncation term %.3e, with the rounding allowance %.3e; sweeps <= %d, rounds <= %d"
          % (worst, 0.95 / 0.05 * 1e-12, bound, out["sweeps"].max(), out["iters"].max()))
    assert worst <= bound and (out["iters"] >= 0).all()


def test_known_answers_constant_rival_and_gamma_zero():
    tabs, pl = sn.tables(SMALL), E.plan(SMALL)
    J, W = tabs["n_cells"], tabs["band_w"]
    rival = 12
    Rv = 0.95 * pl["rew"][0].reshape(21, 21)[:, rival] + 0.05 * tabs["noise_reward"][0].reshape(21, 21)[:, rival]
    best = int(np.argmax(Rv))
    # a rival that plays one action in every row makes agent 0's problem static
    pol = S.policies(SMALL, np.concatenate([E.strategy_tables(SMALL, [a0, rival]) for a0 in (3, 20, best)]))
    w = np.tile(tabs["cell_w"], (3, 1))
    out = EN.analyse(SMALL, tabs, pol, 0.05, agents=[0], weights=w)
    assert (out["br_policy"][0] == best).all() and out["iters"][0].tolist() == [1, 1, 0]
    e = EN.error_bound(0.95, 1e-12, W, Rv.max() / 0.05)
    err = np.abs(out["v_opt"][0] - Rv.max() / 0.05).max()
    print("max |V* - max R / (1 - gamma)| = %.3e (bound %.3e)" % (err, e))
    assert err <= e
    assert out["n_diff_all"][0].tolist() == [J, J, 0]
    for f in ("loss_all", "loss_all_mean", "loss_w", "diff_w"):
        assert out[f][0, 2] == 0.0 and (out[f][0, :2] > 0).all(), f
    assert np.array_equal(out["v_opt"][0, 2], out["v_pi"][0, 2])
    assert abs(out["diff_w"][0, 0] - 1.0) <= J * 2 * U                   # every cell differs: the weights' sum
    # gamma = 0: V = R exactly after 2 sweeps, sigma* the one-period best response under noise
    pol = S.policies(SMALL, S.fresh_tables(SMALL, 4, 2))
    out = EN.analyse(SMALL, tabs, pol, 0.05, gamma=np.zeros((2, 4)))
    tup = S.cell_tuples(SMALL, pol, tabs, 4)
    for g in range(4):
        for i in range(2):
            R, _, pk = EN.dense(pl, tabs, tup[g], i, 0.05)
            assert out["sweeps"][i, g] == 2 * (out["iters"][i, g] + 1) and out["iters"][i, g] <= 1
            assert np.array_equal(out["v_opt"][i, g], R.max(axis=1))
            keep = R.max(axis=1) == R[np.arange(J), pk]
            assert np.array_equal(out["br_policy"][i, g], np.where(keep, pk, R.argmax(axis=1)))


def test_cap_bad_gamma_and_bad_noise_on_the_mirror():
    tabs = sn.tables(SMALL)
    pol = S.policies(SMALL, S.fresh_tables(SMALL, 5, 4))
    w = np.tile(tabs["cell_w"], (5, 1))
    out = EN.analyse(SMALL, tabs, pol, 0.05, max_sweeps=16, weights=w)
    assert (out["iters"] == -1).all() and (out["sweeps"] == 16).all() and (out["n_diff_all"] == 0).all()
    assert np.isnan(out["loss_all"]).all() and np.isnan(out["v_w"]).all() and np.isnan(out["v_opt"]).all()
    gam = np.full((2, 5), 0.9)
    gam[0, 1], gam[1, 2] = 1.0, -0.1
    p = np.array([0.05, 0.05, 0.05, 0.0, np.nan])
    out = EN.analyse(SMALL, tabs, pol, p, gamma=gam, weights=w)
    assert out["iters"][0, 1] == -1 and out["iters"][1, 2] == -1 and np.isnan(out["loss_w"][0, 1]) and out["sweeps"][0, 1] == 0
    assert out["iters"][1, 1] >= 0 and out["iters"][0, 2] >= 0 and (out["iters"][:, 0] >= 0).all()
    for f in EN.INT_FIELDS + EN.FLOAT_FIELDS + EN.W_FIELDS + EN.CELL_FIELDS:
        assert (np.asarray(out[f])[:, 3:] == (-1 if f == "iters" else 0)).all(), f


def test_margin_stops_cycling_on_evaluation_error():
    """With a loose evaluation (eval_tol = 1e-3) the rounds still end well inside the cap, and the strategy found loses
    at most the bound of test_mirror_against_independent_solves against the optimum."""
    tabs, pl = sn.tables(SMALL), E.plan(SMALL)
    pol = S.policies(SMALL, S.fresh_tables(SMALL, 6, 5))
    out = EN.analyse(SMALL, tabs, pol, 0.05, eval_tol=1e-3)
    assert (out["iters"] >= 0).all() and out["iters"].max() <= 8
    tup = S.cell_tuples(SMALL, pol, tabs, 6)
    for g in range(6):
        for i, gamma in enumerate((0.95, 0.9)):
            R, P, _ = EN.dense(pl, tabs, tup[g], i, 0.05)
            vi = EN.value_iteration(R, P, gamma)
            e = EN.error_bound(gamma, 1e-3, tabs["band_w"], np.abs(vi).max())
            d = float(EN.margin_of(gamma, 1e-3)) + 2.0 * gamma * e
            assert np.abs(out["v_opt"][i, g] - vi).max() <= e + d / (1.0 - gamma)
    assert float(EN.margin_of(0.95, 0.0)) == 0.0 and float(EN.margin_of(0.5, 1e-6)) == 2 * 0.5 * 0.5 * 1e-6 / 0.5


# ------------------------------------------------------------------------------------------------ the entry point
TABLES = ("cell_rows", "det_cell", "band_lo", "band", "noise_reward")
OUTPUTS = ("iters", "sweeps", "n_diff_all", "loss_all", "loss_all_mean")
WEIGHTED = ("loss_w", "diff_w", "v_w")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.EquilibriumNoiseArgs()
    a.n_games, a.agents, a.n_cells, a.band_w, a.max_sweeps, a.eval_tol, a.noise_prob = 64, 3, 101, 31, 8192, 1e-12, 0.05
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("policy",) + TABLES + OUTPUTS:
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(n_games=65), dict(agents=0), dict(agents=4), dict(flags=2),
                                 dict(flags=-1), dict(n_cells=0), dict(band_w=0), dict(max_sweeps=0),
                                 dict(max_sweeps=65537), dict(eval_tol=-1e-12), dict(eval_tol=float("nan")),
                                 dict(noise_prob=0.0), dict(noise_prob=1.5), dict(noise_prob=float("nan")),
                                 dict(noise_prob=-0.05)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_equilibrium_noise(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


def test_gamma_of_the_config_is_checked_without_sweep_gamma(lib):
    from th_rl_amd import _lib
    over = {"agents": [dict(AG, gamma=1.5), dict(AG)], "environment": dict(ENV)}
    cfg, _ = _lib.cfg_from_config(over, 64, 0)
    call = lambda a: lib.thrl_equilibrium_noise(ctypes.byref(cfg), None, ctypes.byref(a), None)
    assert call(_args()) == -1 and b"gamma" in lib.thrl_last_error()
    assert call(_args(agents=2)) == -2 and b"q is NULL" in lib.thrl_last_error()         # agent 0 is not solved
    assert call(_args(sweep_gamma=4096)) == -2 and b"q is NULL" in lib.thrl_last_error()  # the device array decides


@pytest.mark.parametrize("null", ("q", "args", "policy") + TABLES + OUTPUTS + WEIGHTED)
def test_missing_pointers_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    kw = {} if null in ("q", "args") else {null: None}
    if null in WEIGHTED:
        kw = dict({f: 4096 for f in WEIGHTED}, weights=4096, **kw)
    a = None if null == "args" else ctypes.byref(_args(**kw))
    assert lib.thrl_equilibrium_noise(ctypes.byref(cfg), q, a, None) == -2


def test_flags_limits_and_n_tuples(lib):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    call = lambda a, q=None: lib.thrl_equilibrium_noise(ctypes.byref(cfg), q, ctypes.byref(a), None)
    t = ctypes.c_int32(-1)
    assert call(_args(n_tuples=ctypes.pointer(t))) == -2 and b"q is NULL" in lib.thrl_last_error() and t.value == 441
    given = _args(flags=_lib.EQN_POLICY_GIVEN, sweeps=None)
    assert call(given) == -2 and b"q is NULL" not in lib.thrl_last_error() and b"sweeps" in lib.thrl_last_error()
    # without weights the three weighted outputs may be NULL: the call gets as far as q
    assert call(_args(loss_w=None, diff_w=None, v_w=None)) == -2 and b"q is NULL" in lib.thrl_last_error()
    # a per-game array replaces the scalar, which is then not read
    assert call(_args(noise_prob=0.0, noise_prob_g=4096)) == -2 and b"q is NULL" in lib.thrl_last_error()
    # the limits: cells, and LDS (50 J + 2064 bytes against 64 KB: J = 1,269 fits, 1,270 does not)
    q = ctypes.c_void_p(4096)
    assert call(_args(n_cells=4097), q) == _lib.ERR_UNSUPPORTED and b"4096" in lib.thrl_last_error()
    assert call(_args(n_cells=1270), q) == _lib.ERR_UNSUPPORTED and b"LDS" in lib.thrl_last_error()
    assert 50 * 1269 + 2064 <= 65536 < 50 * 1270 + 2064
    assert call(_args(n_cells=1269, sweeps=None), q) == -2 and b"sweeps" in lib.thrl_last_error()
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}       # 4,160 tuples
    wcfg, _ = _lib.cfg_from_config(wide, 64, 0)
    assert lib.thrl_equilibrium_noise(ctypes.byref(wcfg), q, ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    fields = [f for f, _ in _lib.EquilibriumNoiseArgs._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %d %d %d %d %d"'
           + "".join(' " %zu"' for _ in fields) + ',sizeof(thrl_equilibrium_noise_args),THRL_EQN_POLICY_GIVEN,'
           'THRL_STAT_MAX_CELLS,THRL_STAT_MAX_ITERS,THRL_EQ_MAX_ITERS,THRL_ABI_VERSION'
           + "".join(",offsetof(thrl_equilibrium_noise_args,%s)" % f for f in fields) + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    want = [ctypes.sizeof(_lib.EquilibriumNoiseArgs), _lib.EQN_POLICY_GIVEN, _lib.STAT_MAX_CELLS, _lib.STAT_MAX_ITERS,
            _lib.EQ_MAX_ITERS, 4]
    assert got == want + [getattr(_lib.EquilibriumNoiseArgs, f).offset for f in fields]
    assert "thrl_equilibrium_noise" in _lib.SYMBOLS and EN.MAX_ITERS == _lib.EQ_MAX_ITERS and _lib.ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_with_noise():
    old = [True, {"agents": [1], "tol": 1e-9, "policies": True, "tables": "converged"}, {"tol": 0.5}, {"policies": True}]
    want = [dict(agents=[0, 1], tol=0.0, policies=False), dict(agents=[1], tol=1e-9, policies=True, tables="converged"),
            dict(agents=[0, 1], tol=0.5, policies=False), dict(agents=[0, 1], tol=0.0, policies=True)]
    for o, w in zip(old, want):         # every option dict valid before parses to what it did
        assert eq.parse_options(o, CFG) == w and eq.parse_options(o, NOISY) == w
    assert eq.parse_options({"noise": None}, CFG) == want[0] and eq.parse_options({"noise": False}, CFG) == want[0]
    assert eq.parse_options({"noise": True}, NOISY) == dict(want[0], noise=eq.NOISE_DEFAULTS)
    assert eq.NOISE_DEFAULTS == dict(noise_prob=None, eval_tol=1e-12, max_sweeps=8192)
    got = eq.parse_options({"agents": [1], "noise": {"noise_prob": 0.2, "eval_tol": 0, "max_sweeps": 100}}, CFG)
    assert got == dict(agents=[1], tol=0.0, policies=False, noise=dict(noise_prob=0.2, eval_tol=0.0, max_sweeps=100))
    swept = dict(CFG, training={"sweep": {"noise_prob": [0.1]}})
    assert eq.parse_options({"noise": True}, swept)["noise"]["noise_prob"] is None
    # the refusal on a noise-free run, with stationary's wording
    with pytest.raises(ValueError, match="the environment has noise_prob = 0: give the noise_prob to analyse"):
        eq.parse_options({"noise": True}, CFG)
    with pytest.raises(ValueError, match="the environment has noise_prob = 0: give the noise_prob to analyse"):
        sn.parse_options(True, CFG)
    for bad in ({"resolution": 8}, {"noise_prob": 0}, {"noise_prob": 1.5}, {"noise_prob": "x"}, {"noise_prob": True},
                {"eval_tol": -1}, {"eval_tol": "a"}, {"eval_tol": True}, {"eval_tol": float("nan")}, {"max_sweeps": 0},
                {"max_sweeps": 65537}, {"max_sweeps": 1.5}, {"max_sweeps": True}, 5, "yes"):
        with pytest.raises(ValueError):
            eq.parse_options({"noise": bad}, NOISY)
    with pytest.raises(ValueError, match="follow-up"):
        eq.parse_options({"noise": True}, MIXED)
    # train_one refuses before it builds a batch (no GPU is touched)
    from th_rl_amd import trainer
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "c.json"), "w").write(json.dumps(dict(CFG, training={"epochs": 1, "n_games": 4,
                                                                                    "equilibrium": {"noise": True}})))
        with pytest.raises(ValueError, match="noise_prob = 0"):
            trainer.train_one(os.path.join(d, "run"), os.path.join(d, "c.json"))


# ------------------------------------------------------------------------------------------------ summary, shards
def _games(G=10, weights=True):
    rs = np.random.RandomState(4)
    g = dict(iters=rs.randint(0, 4, (2, G)).astype(np.int32), sweeps=rs.randint(500, 3000, (2, G)).astype(np.int32),
             n_diff_all=rs.randint(0, 21, (2, G)).astype(np.int32), loss_all=rs.uniform(0, 0.4, (2, G)),
             loss_all_mean=rs.uniform(0, 0.1, (2, G)), noise_prob=np.full(G, 0.05))
    if weights:
        g.update(loss_w=rs.uniform(0, 0.2, (2, G)), diff_w=rs.uniform(0, 1, (2, G)), v_w=rs.uniform(200, 250, (2, G)))
    for f in ("loss_all", "loss_all_mean") + (("loss_w", "diff_w") if weights else ()):
        g[f][:, [0, 5]] = 0.0
        g[f][0, 3] = np.nan
    g["iters"][:, [0, 5]] = 0
    g["iters"][0, 3] = -1                       # capped
    g["loss_all"][1, 1], g["iters"][1, 1] = 1e-12, 1
    return g


def test_flags_and_summary_arithmetic():
    g = _games()
    ids = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1])
    fl = eq.flags_noise(g, [0, 1])
    assert fl["br_all"][0].tolist() == [True] + [False] * 4 + [True] + [False] * 4 and not fl["br_all"][0, 3]
    assert fl["br_w"][1].tolist() == fl["br_all"][0].tolist() and fl["perfect"].tolist() == fl["br_all"][0].tolist()
    assert eq.flags_noise(g, [0, 1], tol=1e-9)["br_all"][1, 1] and not fl["br_all"][1, 1]
    assert not eq.flags_noise(g, [1])["br_all"][0].any() and eq.flags_noise(g, [1])["perfect"][0]
    rows = eq.summarize_noise(g, ids, 3, [0, 1], 0.0)
    assert [(r["group"], r["agent"]) for r in rows] == [(0, 0), (0, 1), (0, None), (1, 0), (1, 1), (1, None), (2, 0), (2, 1), (2, None)]
    a00, a01, g0 = rows[:3]
    assert a00["games"] == 5 and a00["capped"] == 1 and a00["br_all"] == 1 / 5 and a00["br_w"] == 1 / 5
    pos = g["loss_all"][0][[1, 2, 4]]
    assert a00["loss_all_q50"] == float(np.quantile(pos, 0.5)) and a00["loss_all_q25"] == float(np.quantile(pos, 0.25))
    assert a00["loss_w_q75"] == float(np.quantile(g["loss_w"][0][[1, 2, 4]], 0.75))
    assert a00["diff_w_mean"] == float(g["diff_w"][0][[0, 1, 2, 4]].mean()) and a00["sweeps_max"] == int(g["sweeps"][0][:5].max())
    assert a01["capped"] == 0 and a01["loss_all_q50"] == float(np.quantile(g["loss_all"][1][1:5], 0.5))
    assert g0 == {"group": 0, "agent": None, "games": 5, "perfect": 1 / 5}
    assert rows[6]["games"] == 0 and rows[6]["br_all"] is None and rows[6]["sweeps_max"] is None and rows[8]["perfect"] is None
    bare = eq.summarize_noise(_games(weights=False), ids, 2, [0, 1])
    assert bare[0]["br_w"] is None and bare[0]["loss_w_q50"] is None and bare[0]["diff_w_mean"] is None
    assert bare[0]["br_all"] == 1 / 5
    json.dumps(rows)


def test_shards_merge_to_the_unsharded_run_and_readers(tmp_path):
    from th_rl_amd import utils
    G = 10
    rs = np.random.RandomState(6)
    g = dict(_games(G), br_policy=rs.randint(0, 21, (2, G, 7)).astype(np.uint16), v_opt=rs.uniform(200, 250, (2, G, 7)),
             v_pi=rs.uniform(200, 250, (2, G, 7)))
    g = {f: np.nan_to_num(v) for f, v in g.items()}
    ids = np.arange(G) % 2
    config = dict(NOISY, training={"n_games": G, "n_groups": 2, "groups": ids.tolist(),
                                   "equilibrium": {"policies": True, "noise": True}})
    opt = eq.parse_options(config["training"]["equilibrium"], config)
    # save / load
    one = tmp_path / "one"
    one.mkdir()
    eq.save_noise_games(str(one), g)
    back = eq.load_noise_games(str(one))
    assert set(back) == set(g)
    for f in g:
        assert np.array_equal(back[f], g[f]) and back[f].dtype == g[f].dtype, f
    assert sorted(f.name for f in one.iterdir()) == ["eqn_iters.npy", "eqn_loss.npy", "eqn_policy.npy", "eqn_prob.npy",
                                                     "eqn_v_opt.npy", "eqn_v_pi.npy", "eqn_weighted.npy"]
    # two fabricated shards (the noise-free arrays of the same games beside them) against the unsharded arrays
    q = rs.rand(G, 2 * 101 * 21)
    s0 = rs.uniform(0, 10, G)
    two = tmp_path / "two"
    shards = []
    for r, (lo, hi) in enumerate(((0, 4), (4, G))):
        d = two / ("shard%d" % r)
        d.mkdir(parents=True)
        shards.append(str(d))
        part = E.analyse(CFG, q[lo:hi], s0[lo:hi])
        part.pop("n_states")
        eq.save_games(str(d), part)
        eq.save_json(str(d / "equilibrium.json"), eq.describe(opt, 41, eq.summarize(part, ids[lo:hi], 2, [0, 1])))
        cut = {f: (v[lo:hi] if v.ndim == 1 else v[:, lo:hi]) for f, v in g.items()}
        eq.save_noise_games(str(d), cut)
        eq.save_json(str(d / "equilibrium_noise.json"),
                     eq.describe_noise(opt, 7, eq.summarize_noise(cut, ids[lo:hi], 2, [0, 1])))
        (d / "shard_config.json").write_text(json.dumps(dict(config, training=dict(config["training"], n_games=hi - lo,
                                                                                     game_offset=lo))))
    first = json.load(open(os.path.join(shards[0], "equilibrium.json")))
    assert "noise" not in first["options"]                  # equilibrium.json is what it is without the option
    desc = eq.merged(shards, str(two), config, opt, ids, 2, first)
    assert "noise" not in desc["options"] and len(desc["summary"]) == 6
    both = eq.load_noise_games(str(two))
    for f in g:
        assert np.array_equal(both[f], g[f]), f
    nd = json.load(open(two / "equilibrium_noise.json"))
    assert nd["options"]["noise"] == eq.NOISE_DEFAULTS and nd["n_cells"] == 7
    assert nd["summary"] == json.loads(json.dumps(eq.summarize_noise(g, ids, 2, [0, 1])))
    # without the option the merge writes nothing of it
    three = tmp_path / "three"
    three.mkdir()
    eq.merged(shards, str(three), config, eq.parse_options({"policies": True}, config), ids, 2, first)
    assert not any(f.name.startswith("eqn_") or f.name == "equilibrium_noise.json" for f in three.iterdir())
    # the readers: per game from the shards (before and after the merge), the summary from the merged directory
    eq.save_json(str(one / "equilibrium_noise.json"), eq.describe_noise(opt, 7, eq.summarize_noise(g, ids, 2, [0, 1])))
    (one / "config.json").write_text(json.dumps(config))
    a, b = utils.equilibrium_noise_games(str(one), 1), utils.equilibrium_noise_games(str(two), 1)
    for f in ("eqn_iters.npy",):
        os.remove(two / f)                                  # back to the shards alone
    c = utils.equilibrium_noise_games(str(two), 1)
    assert a.index.tolist() == b.index.tolist() == c.index.tolist() == list(range(G))
    for col in a.columns:
        assert np.array_equal(a[col].to_numpy(), b[col].to_numpy()) and np.array_equal(a[col].to_numpy(), c[col].to_numpy()), col
    assert a["loss_w"].tolist() == g["loss_w"][1].tolist() and a["perfect"].tolist() == eq.flags_noise(g, [0, 1])["perfect"].tolist()
    df = utils.equilibrium_noise_summary(str(two))
    assert len(df) == 6 and df["n_cells"].tolist() == [7] * 6 and df["tol"].tolist() == [0.0] * 6
    with pytest.raises(KeyError, match=r"no equilibrium check under noise \(eqn_iters.npy\) under .* \(training.equilibrium.noise\)"):
        utils.equilibrium_noise_games(str(tmp_path / "none"), 0)
    with pytest.raises(KeyError, match=r"no equilibrium check under noise \(equilibrium_noise.json\)"):
        utils.equilibrium_noise_summary(str(tmp_path / "none"))


def test_batch_method_is_shared_and_documented():
    from th_rl_amd import analysis
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    fn = analysis.AnalysisMethods.equilibrium_noise
    assert GameBatch.equilibrium_noise is fn and MixedGameBatch.equilibrium_noise is fn and "thrl_equilibrium_noise" in fn.__doc__
    assert [a.key for a in analysis.REGISTRY].count("equilibrium") == 1 and len(analysis.REGISTRY) == 12
