"""Host side of the equilibrium check (thrl_equilibrium, th_rl_amd.equilibrium): the numpy mirror against an
independent solver and against known answers on the headline grid, the entry point's validation through the library
loaded without a GPU, the ctypes mirror of the args struct, option parsing, the flags and the summary on hand-made
games, the shard combination and the utils readers.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import deviation_mirror as M
import equilibrium_mirror as E
from th_rl_amd import equilibrium as eq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the state set
def test_state_sets():
    pl = E.plan(CFG)
    assert (pl["T"], pl["S"]) == (441, 41)
    assert sorted(pl["srow"][0].tolist()) == list(range(20, 61)) and np.array_equal(pl["srow"][0], pl["srow"][1])
    assert pl["sid"][0] == 0 and pl["tstride"] == [21, 1]
    p3 = E.plan(THREE)
    assert (p3["T"], p3["S"]) == (385, 87) and p3["tstride"] == [55, 5, 1]
    # numbered in order of first occurrence in tuple order
    first = [int(np.flatnonzero(p3["sid"] == s)[0]) for s in range(p3["S"])]
    assert first == sorted(first)


def test_doublings():
    assert [E.doublings(g) for g in (0.0, 0.3, 0.9, 0.95, 0.99)] == [0, 6, 9, 10, 13]
    assert E.doublings(np.nextafter(1.0, 0.0)) <= 59


# ------------------------------------------------------------------------------------------------ the scheme
@pytest.mark.parametrize("gamma", [0.9, 0.95, 0.99])
@pytest.mark.parametrize("name", ["headline", "three"])
def test_mirror_against_value_iteration(name, gamma):
    """max |V* - W| <= 4 (2 D + 2 / (1 - gamma)) 2^-53 max W: two roundings per doubling round, two per sweep of the
    value iteration accumulating to 2 u / (1 - gamma), and a factor 4."""
    config = CFG if name == "headline" else THREE
    pl = E.plan(config)
    rs = np.random.RandomState(7)
    worst = 0.0
    for trial in range(6):
        pol = [rs.randint(0, pl["n_actions"][i], pl["S"]) for i in range(pl["N"])]
        for i in range(pl["N"]):
            it, sig, v_opt, v_pi = E.solve(pl, pol, i, gamma)
            R, nxt = E.problem(pl, pol, i)
            W = E.value_iteration(R, nxt, gamma)
            bound = 4 * (2 * E.doublings(gamma) + 2 / (1 - gamma)) * 2.0 ** -53 * W.max()
            err = np.abs(v_opt - W).max()
            print("%s gamma=%g agent %d: iters %d, max|V*-W| %.3e, bound %.3e" % (name, gamma, i, it, err, bound))
            assert 0 <= it <= 8
            assert err <= bound
            assert (v_opt >= v_pi - bound).all()
            worst = max(worst, err / bound)
    assert worst <= 1.0


def test_best_response_keeps_the_incumbent_bit_for_bit():
    pl = E.plan(CFG)
    rs = np.random.RandomState(3)
    pol = [rs.randint(0, 21, 41), rs.randint(0, 21, 41)]
    _, sig, v_opt, _ = E.solve(pl, pol, 0, 0.95)
    it, sig2, v2, v_pi2 = E.solve(pl, [sig, pol[1]], 0, 0.95)
    assert it == 0 and np.array_equal(sig2, sig)
    assert np.array_equal(v2.view(np.uint64), v_pi2.view(np.uint64))
    assert np.array_equal(v2.view(np.uint64), v_opt.view(np.uint64))


# ------------------------------------------------------------------------------------------------ known answers
def test_known_static_nash_pairs():
    pl = E.plan(CFG)
    pairs = E.static_best_responses(pl)
    assert pairs == [(13, 14), (14, 13)]
    for a0, a1 in pairs:
        r = E.analyse(CFG, E.strategy_tables(CFG, [a0, a1], 2), [3.0, 7.5])
        assert r["iters"].tolist() == [[0, 0]] * 2 and not r["n_diff_all"].any()
        for f in ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean"):
            assert (r[f] == 0.0).all() and not np.signbit(r[f]).any()
        assert r["lam"].tolist() == [1, 1]


def test_known_cartel_without_punishment():
    pl = E.plan(CFG)
    r = E.analyse(CFG, E.strategy_tables(CFG, [5, 5], 1), [3.0])
    assert r["n_diff_all"][:, 0].tolist() == [41, 41] and r["iters"][:, 0].tolist() == [1, 1]
    R = pl["rew"][0].reshape(21, 21)
    want = 1.0 - R[5, 5] / R[:, 5].max()
    assert abs(want - 0.110953) < 1e-6
    assert abs(r["loss_all"][0, 0] - want) <= 4 * 2 * E.doublings(0.95) * 2.0 ** -53 * want
    # every state gives up the same share: the rival plays 5 everywhere
    assert abs(r["loss_all_mean"][0, 0] - want) < 1e-12 and abs(r["loss_on"][0, 0] - want) < 1e-12


def _grim():
    pl = E.plan(CFG)
    row = int(M.encode(M.env_step([M.scale(5, pl["ag"][0]), M.scale(5, pl["ag"][1])], 10.0, 1.0)[0], pl["ag"][0]))
    s0, s1 = np.full(101, 13), np.full(101, 14)
    s0[row] = s1[row] = 5
    return row, [s0, s1]


def test_known_grim_trigger():
    row, strat = _grim()
    assert row == 50
    patient = {"agents": [dict(AG, gamma=0.95), dict(AG, gamma=0.95)], "environment": dict(ENV)}
    r = E.analyse(patient, E.strategy_tables(patient, strat, 1), [5.0])
    fl = eq.flags(r, [0, 1])
    assert (r["mu"][0], r["lam"][0]) == (0, 1) and fl["nash"].all() and fl["perfect"].all()
    assert r["iters"][:, 0].tolist() == [0, 0]
    hasty = {"agents": [dict(AG, gamma=0.3), dict(AG, gamma=0.3)], "environment": dict(ENV)}
    r = E.analyse(hasty, E.strategy_tables(hasty, strat, 1), [5.0])
    fl = eq.flags(r, [0, 1])
    assert r["n_diff_on"][:, 0].tolist() == [1, 1] and (r["loss_on"] > 0).all() and not fl["nash"].any()
    assert abs(r["loss_on"][0, 0] - 0.0465) < 1e-3
    # every off-path state is a best response: the only state whose action changes is the cartel state
    pl = E.plan(hasty)
    cartel_state = pl["ids"][(50, 50)]
    for i in (0, 1):
        changed = np.flatnonzero(r["br_policy"][i, 0] != strat[i][pl["srow"][i]])
        assert changed.tolist() == [cartel_state]


def test_mirror_cycle_equals_deviation_mirror():
    rs = np.random.RandomState(5)
    G = 40
    q = rs.rand(G, 2 * 101 * 21)
    s0 = rs.uniform(0, 10, G)
    e = E.analyse(CFG, q, s0, agents=[0])
    d = M.analyse(CFG, q, s0, steps=2)
    assert e["mu"].tolist() == d["mu"].tolist() and e["lam"].tolist() == d["lam"].tolist()
    assert e["lam"].max() > 1 and e["mu"].min() >= 0


# ------------------------------------------------------------------------------------------------ the entry point
def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.EquilibriumArgs()
    a.n_games, a.agents = 64, 3
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("state0", "mu", "lam", "iters", "n_diff_all", "n_diff_on", "loss_all", "loss_on", "loss_all_mean",
              "loss_on_mean", "v_on"):
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(n_games=65), dict(agents=0), dict(agents=4), dict(agents=-1)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_equilibrium(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("gamma", [1.0, 1.5, -0.1, float("nan")])
def test_gamma_outside_unit_interval_is_bad_config(lib, gamma):
    from th_rl_amd import _lib
    one = {"agents": [dict(AG, gamma=gamma), dict(AG)], "environment": dict(ENV)}
    cfg, _ = _lib.cfg_from_config(one, 64, 0)
    assert lib.thrl_equilibrium(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == -1
    assert b"gamma" in lib.thrl_last_error()
    # an agent that is not solved may have any gamma: validation passes on to the pointer checks
    assert lib.thrl_equilibrium(ctypes.byref(cfg), None, ctypes.byref(_args(agents=2)), None) == -2


@pytest.mark.parametrize("null", ["q", "state0", "mu", "lam", "iters", "n_diff_all", "n_diff_on", "loss_all", "loss_on",
                                  "loss_all_mean", "loss_on_mean", "v_on", "args"])
def test_missing_outputs_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    a = None if null == "args" else ctypes.byref(_args(**({} if null in ("q", "args") else {null: None})))
    assert lib.thrl_equilibrium(ctypes.byref(cfg), q, a, None) == -2


def test_limits_are_unsupported_and_n_states_is_reported(lib):
    from th_rl_amd import _lib
    s = ctypes.c_int32(-1)
    for config, want in ((CFG, 41), (THREE, 87)):
        cfg, _ = _lib.cfg_from_config(config, 64, 0)
        a = _args(n_states=ctypes.pointer(s))
        assert lib.thrl_equilibrium(ctypes.byref(cfg), None, ctypes.byref(a), None) == -2 and s.value == want
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}       # 4,160 tuples
    cfg, _ = _lib.cfg_from_config(wide, 64, 0)
    assert lib.thrl_equilibrium(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED
    # 64 x 64 tuples of incommensurable grids on a fine state grid: more than 1,024 distinct row tuples
    fine = {"agents": [dict(AG, actions=64, states=30000), dict(AG, actions=64, states=30000, action_range=[0.2, 0.4037])],
            "environment": dict(ENV)}
    assert E.plan(fine)["S"] > 1024
    cfg, _ = _lib.cfg_from_config(fine, 64, 0)
    assert lib.thrl_equilibrium(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED
    assert b"states" in lib.thrl_last_error()


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    src = ('#include <stdio.h>\n#include "thrl.h"\nint main(){printf("%zu %d %d %d %d\\n",sizeof(thrl_equilibrium_args),'
           'THRL_EQ_MAX_ITERS,THRL_EQ_MAX_TUPLES,THRL_EQ_MAX_STATES,THRL_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [ctypes.sizeof(_lib.EquilibriumArgs), _lib.EQ_MAX_ITERS, _lib.EQ_MAX_TUPLES, _lib.EQ_MAX_STATES, 4]
    assert E.MAX_ITERS == _lib.EQ_MAX_ITERS


# ------------------------------------------------------------------------------------------------ options
def test_parse_options():
    assert eq.parse_options(True, CFG) == dict(agents=[0, 1], tol=0.0, policies=False)
    o = eq.parse_options({"agents": [1], "tol": 1e-9, "policies": True, "tables": "converged"}, CFG)
    assert o == dict(agents=[1], tol=1e-9, policies=True, tables="converged")
    for bad in ({"agents": []}, {"agents": [2]}, {"tol": -1.0}, {"tables": "best"}, {"steps": 3}, 5):
        with pytest.raises(ValueError):
            eq.parse_options(bad, CFG)
    with pytest.raises(ValueError, match="follow-up"):
        eq.parse_options(True, MIXED)


def test_gamma_of_one_is_refused_before_training(tmp_path):
    one = {"agents": [dict(AG, gamma=1.0), dict(AG)], "environment": dict(ENV)}
    with pytest.raises(ValueError, match=r"gamma in \[0, 1\)"):
        eq.parse_options(True, one)
    assert eq.parse_options({"agents": [1]}, one)["agents"] == [1]
    swept = dict(CFG, training={"sweep": {"gamma": [0.5, 1.0, 0.9]}})
    with pytest.raises(ValueError, match="sweep.gamma"):
        eq.parse_options(True, swept)
    assert eq.parse_options(True, dict(CFG, training={"sweep": {"gamma": [0.5, 0.0, 0.9]}}))["agents"] == [0, 1]
    # train_one refuses both before it builds a batch (no GPU is touched); gamma = 1 itself never gets that far, the
    # QTable constructor divides by 1 - gamma
    from th_rl_amd import trainer
    over = {"agents": [dict(AG, gamma=1.5), dict(AG)], "environment": dict(ENV)}
    for cfg in (dict(over, training={"epochs": 1, "n_games": 4, "equilibrium": True}),
                dict(MIXED, training={"epochs": 1, "n_games": 4, "equilibrium": True}),
                dict(CFG, training={"epochs": 1, "n_games": 4, "equilibrium": {"tables": "converged"}})):
        (tmp_path / "c.json").write_text(json.dumps(cfg))
        with pytest.raises(ValueError):
            trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))


# ------------------------------------------------------------------------------------------------ flags, summary
def _games():
    """Six games, two agents, two groups (ids 0 0 0 1 1 1)."""
    lon = np.array([[0.0, 0.0, 0.2, 0.0, 1e-12, 0.0], [0.0, 0.1, 0.0, 0.0, 0.0, 0.0]])
    lall = np.array([[0.0, 0.3, 0.4, 0.0, 1e-12, 0.5], [0.0, 0.1, 0.0, 0.0, 0.0, 0.0]])
    g = {"mu": np.zeros(6, np.int32), "lam": np.ones(6, np.int32), "iters": np.array([[0, 1, 2, 0, 1, -1], [0, 1, 0, 0, 0, 0]]),
         "n_diff_all": (lall > 0).astype(np.int32), "n_diff_on": (lon > 0).astype(np.int32), "loss_on": lon,
         "loss_all": lall, "loss_on_mean": lon, "loss_all_mean": lall / 41, "v_on": np.ones((2, 6))}
    return g, np.array([0, 0, 0, 1, 1, 1])


def test_flags_and_tolerance():
    g, _ = _games()
    f = eq.flags(g, [0, 1])
    assert f["br_on"].tolist() == [[True, True, False, True, False, True], [True, False, True, True, True, True]]
    assert f["nash"].tolist() == [True, False, False, True, False, True]
    assert f["perfect"].tolist() == [True, False, False, True, False, False]
    f = eq.flags(g, [0, 1], tol=1e-9)
    assert f["nash"].tolist() == [True, False, False, True, True, True] and f["perfect"][4]
    f = eq.flags(g, [1])
    assert not f["br_on"][0].any() and f["nash"].tolist() == [True, False, True, True, True, True]


def test_summary_arithmetic():
    g, ids = _games()
    delta = np.array([0.9, 0.8, 0.1, 0.6, 0.7, 0.2])
    s = eq.summarize(g, ids, 2, [0, 1], 0.0, delta)
    assert [(r["group"], r["agent"]) for r in s] == [(0, 0), (0, 1), (0, None), (1, 0), (1, 1), (1, None)]
    a00, a01, g0, a10, a11, g1 = s
    assert a00["games"] == 3 and a00["br_on"] == 2 / 3 and a00["br_all"] == 1 / 3 and a00["capped"] == 0
    assert a00["loss_on_q50"] == 0.2 and a00["loss_all_q50"] == 0.35 and a00["loss_all_q25"] == 0.325
    assert a01["br_on"] == 2 / 3 and a01["loss_on_q50"] == 0.1
    assert a10["capped"] == 1 and a10["br_all"] == 1 / 3 and a11["loss_on_q50"] is None and a11["br_all"] == 1.0
    assert g0["nash"] == 1 / 3 and g0["perfect"] == 1 / 3 and g0["collusive"] == 2
    assert g0["nash_collusive"] == 0.5 and g0["perfect_collusive"] == 0.5
    assert g1["nash"] == 2 / 3 and g1["perfect"] == 1 / 3 and g1["collusive"] == 2 and g1["nash_collusive"] == 0.5
    none = eq.summarize(g, ids, 2, [0, 1], 0.0, None)
    assert none[2]["collusive"] is None and none[2]["nash_collusive"] is None and none[2]["nash"] == 1 / 3
    empty = eq.summarize(g, ids, 3, [0], 0.0, delta)
    assert empty[-1]["games"] == 0 and empty[-1]["nash"] is None and empty[-2]["br_on"] is None
    json.dumps(s)


def test_shards_combine_to_the_unsharded_run(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(1)
    G = 23
    q = rs.rand(G, 2 * 101 * 21)
    s0 = rs.uniform(0, 10, G)
    full = E.analyse(CFG, q, s0)
    parts = [E.analyse(CFG, q[lo:hi], s0[lo:hi]) for lo, hi in ((0, 9), (9, 16), (16, G))]
    fields = [f for f in full if f != "n_states"]
    for p in parts:
        p.pop("n_states")
    whole = eq.combine(parts)
    for f in fields:
        assert np.array_equal(np.asarray(whole[f]), np.asarray(full[f])), f
    ids = np.arange(G) % 2
    assert eq.summarize(whole, ids, 2, [0, 1]) == eq.summarize(full, ids, 2, [0, 1])
    # the artefact round trip and the readers, sharded and not
    opt = eq.parse_options(True, CFG)
    one = tmp_path / "one"
    one.mkdir()
    eq.save_games(str(one), full)
    eq.save_json(str(one / "equilibrium.json"), eq.describe(opt, 41, eq.summarize(full, ids, 2, [0, 1])))
    (one / "config.json").write_text(json.dumps(dict(CFG, training={"n_games": G})))
    back = eq.load_games(str(one))
    for f in fields:
        assert np.array_equal(back[f], np.asarray(full[f])), f
    two = tmp_path / "two"
    for r, (lo, hi) in enumerate(((0, 9), (9, 16), (16, G))):
        d = two / ("shard%d" % r)
        d.mkdir(parents=True)
        eq.save_games(str(d), parts[r])
        eq.save_json(str(d / "equilibrium.json"), eq.describe(opt, 41, []))
        (d / "shard_config.json").write_text(json.dumps(dict(CFG, training={"n_games": hi - lo, "game_offset": lo})))
    a, b = utils.equilibrium_games(str(one), 1), utils.equilibrium_games(str(two), 1)
    assert a.index.tolist() == b.index.tolist() == list(range(G))
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy()), c
    assert a["loss_on"].tolist() == full["loss_on"][1].tolist() and a["nash"].tolist() == eq.flags(full, [0, 1])["nash"].tolist()
    df = utils.equilibrium_summary(str(one))
    assert len(df) == 6 and df["n_states"].tolist() == [41] * 6
    with pytest.raises(KeyError):
        utils.equilibrium_games(str(tmp_path), 0)


def test_docstrings_state_that_the_cycles_agree():
    from th_rl_amd import utils
    for fn in (utils.deviation_summary, utils.equilibrium_summary):
        assert "mu and lam" in fn.__doc__ and "same run" in fn.__doc__
