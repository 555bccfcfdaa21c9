"""Host side of the deviation test and the equilibrium check in tuple form (th_rl_amd.tuple_analysis,
thrl_tuple_deviation / thrl_tuple_equilibrium): the numpy mirrors' known answers on hand-written strategies of the
3 x 3 game, option parsing and refusals, the summaries, the ctypes mirrors of the two args structs against the header
and the entry points' validation through the library loaded without a GPU.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tuple_deviation_mirror as DM
import tuple_equilibrium_mirror as EM
from th_rl_amd import tuple_analysis as ta, tuple_play as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
RF = dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])
MIXED = {"agents": [dict(AG), dict(RF)], "environment": dict(ENV)}
CAC = {"agents": [dict(AG), dict(name="CAC", gamma=0.99, states=1, action_range=[0.2, 0.4])], "environment": dict(ENV)}
SMALL = {"agents": [dict(AG, actions=3), dict(AG, actions=3)], "environment": dict(ENV)}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _strategy(nxt):
    """uint16 [1, 2, 9]: the two agents' entries that send tuple t of the 3 x 3 game to tuple nxt[t]."""
    nxt = np.asarray(nxt)
    return np.stack([nxt // 3, nxt % 3])[None].astype(np.uint16)


# ------------------------------------------------------------------------------------------------ deviation mirror
def test_a_punished_deviation_returns():
    t = tp.tables(SMALL)
    r0 = t["reward"][0]
    assert r0[6] > r0[3] > r0[0] and r0[0] > r0[8]                       # against action 0 the best reply is 2
    # the quiet tuple 0 is kept by a trigger: any other tuple is answered by one period of (2, 2), then back to 0
    pol = _strategy([0, 8, 8, 8, 8, 8, 8, 8, 0])
    g = 0.95
    r = DM.analyse(t, pol, [0], deviator=0, steps=4, dev_len=1, action=-1, gamma=g)
    assert (r["mu"][0], r["lam"][0], r["act_dev"][0]) == (0, 1, 2)
    assert r["cycle_reward"][:, 0].tolist() == t["reward"][:, 0].tolist()
    assert r["cycle_action"][:, 0].tolist() == t["scaled"][:, 0].tolist()
    assert r["reward_rows"][:, 0, 0].tolist() == [r0[6], r0[8], r0[0], r0[0]]
    assert r["action_rows"][:, 1, 0].tolist() == [t["scaled"][1, x] for x in (6, 8, 0, 0)]
    assert (r["mu_post"][0], r["lam_post"][0], r["ret_step"][0]) == (2, 1, 3)
    w1 = 1.0 * g
    w2 = w1 * g
    w3 = w2 * g
    want = (((0.0 + 1.0 * (r0[6] - r0[0])) + w1 * (r0[8] - r0[0])) + w2 * (r0[0] - r0[0])) + w3 * (r0[0] - r0[0])
    assert r["gain"][0] == want and 0 < want < r0[6] - r0[0]
    # a fixed deviation of the other agent for two periods: the punishment starts when it stops
    r = DM.analyse(t, pol, [0], deviator=1, steps=5, dev_len=2, action=1, gamma=g)
    assert r["act_dev"][0] == 1 and r["reward_rows"][:, 1, 0].tolist() == [t["reward"][1, x] for x in (1, 7, 8, 0, 0)]
    assert (r["mu_post"][0], r["lam_post"][0], r["ret_step"][0]) == (2, 1, 4)


def test_an_unpunished_deviation_stays_and_a_short_horizon_finds_no_cycle():
    t = tp.tables(SMALL)
    r0 = t["reward"][0]
    pol = _strategy([0, 1, 2, 3, 4, 5, 6, 7, 8])                         # everybody repeats what was played
    r = DM.analyse(t, pol, [0], deviator=0, steps=3, gamma=0.5)
    assert (r["lam"][0], r["act_dev"][0], r["mu_post"][0], r["lam_post"][0], r["ret_step"][0]) == (1, 2, 0, 1, -1)
    d = r0[6] - r0[0]
    assert r["gain"][0] == ((0.0 + d) + 0.5 * d) + 0.25 * d
    # 0 -> 1 -> 2 -> 3 -> 4 -> 3: mu + lam = 5
    pol = _strategy([1, 2, 3, 4, 3, 0, 0, 0, 0])
    r = DM.analyse(t, pol, [0], steps=2, horizon=5)
    assert (r["mu"][0], r["lam"][0]) == (3, 2)
    assert r["cycle_reward"][0, 0] == ((0.0 + r0[4]) + r0[3]) / 2.0
    r = DM.analyse(t, pol, [0], steps=2, horizon=4, action=0)
    assert (r["mu"][0], r["lam"][0], r["ret_step"][0]) == (4, 0, -1)     # s* = t_4 = 4; play goes on from there
    assert not r["cycle_reward"].any() and not r["cycle_action"].any()
    assert r["reward_rows"][:, 1, 0].tolist() == [t["reward"][1, x] for x in (0, 1)]     # F(4) = 3 with 0 in place 0
    assert (r["mu_post"][0], r["lam_post"][0]) == (4, 0)                 # from y_1 = 0 the same rule: 3 + 2 > 4


def test_a_refused_start_in_the_deviation_mirror():
    t = tp.tables(SMALL)
    pol = np.concatenate([_strategy([4] * 9)] * 3)
    r = DM.analyse(t, pol, [-1, 2, 9], steps=2)
    for f, v in (("mu", -1), ("lam", 0), ("mu_post", 0), ("lam_post", 0), ("ret_step", -1), ("act_dev", -1)):
        assert r[f][[0, 2]].tolist() == [v, v], f
    assert not r["gain"][[0, 2]].any() and not r["cycle_reward"][:, [0, 2]].any() and not r["reward_rows"][:, :, [0, 2]].any()
    assert (r["mu"][1], r["lam"][1]) == (1, 1) and r["reward_rows"][:, :, 1].any()


# ------------------------------------------------------------------------------------------------ equilibrium mirror
def test_a_best_response_in_place_and_one_improvable_state():
    t = tp.tables(SMALL)
    r0 = t["reward"][0]
    g = 0.9
    pol = _strategy([6] * 9)                                             # agent 1 always plays 0, agent 0 its best reply 2
    r = EM.analyse(t, pol, [3], agents=[0], gamma=g, policies=True)
    assert (r["mu"][0], r["lam"][0], r["iters"][0, 0], r["n_diff_all"][0, 0], r["n_diff_on"][0, 0]) == (1, 1, 0, 0, 0)
    assert np.array_equal(r["v_opt"].view(np.uint64), r["v_pi"].view(np.uint64))
    assert r["loss_all"][0, 0] == 0.0 and r["loss_on"][0, 0] == 0.0 and r["loss_all_mean"][0, 0] == 0.0
    assert r["br_policy"][0, 0].tolist() == [2] * 9 and r["iters"][1, 0] == 0 and r["v_on"][1, 0] == 0.0   # not solved
    assert r["v_on"][0, 0] == r["v_pi"][0, 0, 6] and abs(r["v_on"][0, 0] - r0[6] / (1 - g)) < 1e-9
    assert EM.doublings(0.9) == 9 and EM.doublings(0.95) == 10 and EM.doublings(0.99) == 13 and EM.doublings(0.0) == 0
    # agent 1 is not at a best reply: against 2 it should play 1
    r1 = EM.analyse(t, pol, [3], agents=[1], gamma=g, policies=True)
    assert r1["iters"][1, 0] == 1 and r1["n_diff_all"][1, 0] == 9 and r1["br_policy"][1, 0].tolist() == [1] * 9
    assert r1["loss_on"][1, 0] > 0 and r1["iters"][0, 0] == 0
    # one state where agent 0 plays 0 instead of 2
    nxt = [6] * 9
    nxt[4] = 0
    pol = _strategy(nxt)
    r = EM.analyse(t, np.concatenate([pol, pol]), [6, 4], agents=[0], gamma=g, policies=True)
    assert r["mu"].tolist() == [0, 2] and r["lam"].tolist() == [1, 1]
    for k in (0, 1):
        assert (r["iters"][0, k], r["n_diff_all"][0, k], r["n_diff_on"][0, k]) == (1, 1, 0)
        assert r["br_policy"][0, k].tolist() == [2] * 9
        vs, vp = r["v_opt"][0, k], r["v_pi"][0, k]
        assert vs[4] > vp[4] and np.array_equal(np.delete(vs, 4), np.delete(vp, 4))
        assert r["loss_all"][0, k] == (vs[4] - vp[4]) / vs[4] and r["loss_on"][0, k] == 0.0
        assert r["loss_all_mean"][0, k] == r["loss_all"][0, k] / 9.0 and r["v_on"][0, k] == vp[6]
    # gamma = 0: no doubling, one-period values
    r = EM.analyse(t, pol, [6], agents=[0], gamma=0.0, policies=True)
    assert r["iters"][0, 0] == 1 and r["v_opt"][0, 0].tolist() == [r0[6]] * 9 and r["v_pi"][0, 0, 4] == r0[0]
    assert r["loss_all"][0, 0] == (r0[6] - r0[0]) / r0[6] and r["v_on"][0, 0] == r0[6]


def test_a_refused_start_and_a_bad_gamma_in_the_equilibrium_mirror():
    t = tp.tables(SMALL)
    nxt = [6] * 9
    nxt[4] = 0
    pol = np.concatenate([_strategy(nxt)] * 3)
    gam = np.array([[0.9, 0.9, 1.0], [0.9, 0.9, 0.9]])
    r = EM.analyse(t, pol, [6, -1, 6], gamma=gam)
    assert r["mu"].tolist() == [0, -1, 0] and r["lam"].tolist() == [1, 0, 1]
    for f in ("iters", "n_diff_all", "loss_all", "loss_all_mean"):
        assert r[f][:, 1].tolist() == r[f][:, 0].tolist(), f
    assert r["n_diff_on"][:, 1].tolist() == [0, 0]
    for f in ("loss_on", "loss_on_mean", "v_on"):
        assert np.isnan(r[f][:, 1]).all() and not np.isnan(r[f][:, 0]).any()
    assert r["iters"][0, 2] == -1 and r["n_diff_all"][0, 2] == 0 and np.isnan(r["loss_all"][0, 2]) and np.isnan(r["v_on"][0, 2])
    assert r["iters"][1, 2] == r["iters"][1, 0] and r["v_on"][1, 2] == r["v_on"][1, 0]


# ------------------------------------------------------------------------------------------------ options, summaries
def test_option_parsing_and_refusals(tmp_path):
    o = ta.parse_deviation_options(True, MIXED)
    assert o == dict(steps=32, dev_len=1, action="best_response", horizon=None, agents=[0, 1])
    o = ta.parse_deviation_options({"agents": [1], "steps": 8, "dev_len": 2, "action": 20, "horizon": 50}, MIXED)
    assert o["agents"] == [1] and o["action"] == 20 and o["horizon"] == 50
    for bad in ({"tables": "final"}, {"agents": []}, {"agents": [2]}, {"steps": 0}, {"dev_len": 9, "steps": 8},
                {"action": 21}, {"action": "worst"}, {"horizon": 0}, {"steps": 2.5}, {"steps": True}):
        with pytest.raises(ValueError):
            ta.parse_deviation_options(bad, MIXED)
    with pytest.raises(ValueError):
        ta.parse_deviation_options(3, MIXED)
    e = ta.parse_equilibrium_options(True, MIXED)
    assert e == dict(tol=0.0, policies=False, agents=[0, 1])
    assert ta.parse_equilibrium_options({"agents": [1, 1], "tol": 1e-9, "policies": True}, MIXED)["agents"] == [1]
    for bad in ({"tables": "final"}, {"agents": [-1]}, {"tol": -1.0}, {"tol": "x"}, {"policies": 1}):
        with pytest.raises(ValueError):
            ta.parse_equilibrium_options(bad, MIXED)
    undiscounted = {"agents": [dict(AG), dict(RF, gamma=1.0)], "environment": dict(ENV)}
    with pytest.raises(ValueError, match="greedy_equilibrium.*gamma"):
        ta.parse_equilibrium_options(True, undiscounted)
    ta.parse_equilibrium_options({"agents": [0]}, undiscounted)
    with pytest.raises(ValueError, match="sweep.gamma"):
        ta.parse_equilibrium_options(True, dict(MIXED, training={"sweep": {"gamma": [0.5, 1.0]}}))
    wide = {"agents": [dict(AG, actions=129), dict(RF, actions=32)], "environment": dict(ENV)}     # 4128 tuples
    for parse in (ta.parse_deviation_options, ta.parse_equilibrium_options):
        with pytest.raises(ValueError, match="continuous"):
            parse(True, CAC)
        with pytest.raises(ValueError, match="4096"):
            parse(True, wide)
    # train_one refuses before it builds a batch, the launcher before it starts a shard (no GPU is touched)
    from th_rl_amd import launch, trainer
    for key in ("greedy_deviation", "greedy_equilibrium"):
        for cfg in (dict(CAC, training={"epochs": 1, "n_games": 4, key: True}),
                    dict(MIXED, training={"epochs": 1, "n_games": 4, key: {"tables": "converged"}})):
            (tmp_path / "c.json").write_text(json.dumps(cfg))
            with pytest.raises(ValueError):
                trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))
        (tmp_path / "l.json").write_text(json.dumps(dict(MIXED, training={"epochs": 1, "n_games": 4, key: True})))
        with pytest.raises(ValueError, match="%s is not available under th_rl_amd.launch" % key):
            launch.launch(str(tmp_path / "l.json"), str(tmp_path / "out"), gpus=2)
        assert not (tmp_path / "out").exists()


def test_summaries_count_the_games_without_a_start():
    games = {"lam": np.array([1, 2, 0, 0]), "ret_step": np.array([3, -1, -1, -1]), "gain": np.array([-1.0, 0.5, 0.0, 0.0]),
             "cycle_reward": np.array([[2.0, 1.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0]]), "start": np.array([3, 4, -1, 0])}
    s = ta.summarize_deviation(games, [0, 0, 1, 1], 2, 2.0, 4.0, 1)
    assert [(r["group"], r["deviator"], r["games"], r["cycles"], r["no_start"]) for r in s] == [(0, 1, 2, 2, 0), (1, 1, 2, 0, 1)]
    assert s[0]["returned"] == 1 and s[0]["unprofitable"] == 1 and s[0]["delta_mean"] == 0.75
    nan = np.nan
    eqg = {"iters": np.array([[0, 1, 0, 0]]), "loss_on": np.array([[0.0, 0.1, nan, 0.0]]),
           "loss_all": np.array([[0.0, 0.2, 0.0, 0.3]]), "start": games["start"]}
    s = ta.summarize_equilibrium(eqg, [0, 0, 1, 1], 2, [0], 0.0, np.array([0.9, 0.9, -np.inf, 0.1]))
    assert [(r["group"], r["agent"], r["no_start"]) for r in s] == [(0, 0, 0), (0, None, 0), (1, 0, 1), (1, None, 1)]
    assert s[0]["br_on"] == 0.5 and s[2]["br_on"] == 0.5 and s[1]["collusive"] == 2 and s[3]["collusive"] == 0
    json.dumps(s)


# ------------------------------------------------------------------------------------------------ the entry points
def test_args_structs_match_header():
    from th_rl_amd import _lib
    D, E = _lib.TupleDeviationArgs, _lib.TupleEquilibriumArgs
    dfields = [n for n, _ in D._fields_]
    efields = [n for n, _ in E._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %zu %d %d",' \
          'sizeof(thrl_tuple_deviation_args),sizeof(thrl_tuple_equilibrium_args),THRL_TP_MAX_TUPLES,THRL_ABI_VERSION);\n'
    for f in dfields:
        src += 'printf(" %%zu",offsetof(thrl_tuple_deviation_args,%s));\n' % f
    for f in efields:
        src += 'printf(" %%zu",offsetof(thrl_tuple_equilibrium_args,%s));\n' % f
    src += 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    want = [ctypes.sizeof(D), ctypes.sizeof(E), 4096, 4] + [getattr(D, f).offset for f in dfields] \
        + [getattr(E, f).offset for f in efields]
    assert got == want
    assert len(dfields) == 26 and len(efields) == 21
    assert "thrl_tuple_deviation" in _lib.SYMBOLS and "thrl_tuple_equilibrium" in _lib.SYMBOLS and _lib.ABI_VERSION == 4


FAKE = 4096                           # never dereferenced: validation fails before any launch
DEV_FIELDS = ("start", "tuple_policy", "reward", "scaled", "mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev",
              "cycle_reward", "cycle_action", "gain")
EQ_FIELDS = ("start", "tuple_policy", "reward", "mu", "lam", "iters", "n_diff_all", "n_diff_on", "loss_all", "loss_on",
             "loss_all_mean", "loss_on_mean", "v_on")


def _cfg(config=None, G=64):
    from th_rl_amd import _lib
    return _lib.cfg_from_config(config or CFG, G, 0)[0]


def _dev_args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleDeviationArgs()
    a.n_games, a.n_tuples, a.deviator, a.dev_len, a.n_steps, a.horizon, a.dev_action = 64, 441, 0, 1, 8, 442, -1
    for f in DEV_FIELDS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _eq_args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleEquilibriumArgs()
    a.n_games, a.n_tuples, a.agents = 64, 441, 3
    for f in EQ_FIELDS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(deviator=-1), dict(deviator=2), dict(dev_len=0), dict(n_steps=0),
                                 dict(dev_len=9), dict(n_steps=(1 << 20) + 1), dict(horizon=0), dict(horizon=(1 << 24) + 1),
                                 dict(dev_action=-2), dict(dev_action=21), dict(row_begin=-1), dict(row_count=-1),
                                 dict(row_begin=4, row_count=5), dict(reserved=1), dict(n_tuples=0), dict(n_tuples=440)])
def test_tuple_deviation_bad_arguments_are_bad_config(lib, bad):
    cfg = _cfg()
    assert lib.thrl_tuple_deviation(ctypes.byref(cfg), ctypes.byref(_dev_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", DEV_FIELDS + ("args", "cfg"))
def test_tuple_deviation_missing_pointers_are_null(lib, null):
    cfg = _cfg()
    a = None if null == "args" else ctypes.byref(_dev_args(**({null: None} if null in DEV_FIELDS else {})))
    assert lib.thrl_tuple_deviation(None if null == "cfg" else ctypes.byref(cfg), a, None) == -2


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(agents=0), dict(agents=4), dict(reserved=1), dict(n_tuples=0),
                                 dict(n_tuples=442)])
def test_tuple_equilibrium_bad_arguments_are_bad_config(lib, bad):
    cfg = _cfg()
    assert lib.thrl_tuple_equilibrium(ctypes.byref(cfg), ctypes.byref(_eq_args(**bad)), None) == -1
    assert lib.thrl_last_error()


def test_tuple_equilibrium_gamma_rule_and_limits(lib):
    one = _cfg({"agents": [dict(AG), dict(AG, gamma=1.0)], "environment": dict(ENV)})
    call = lambda c, a: lib.thrl_tuple_equilibrium(ctypes.byref(c), ctypes.byref(a), None)
    assert call(one, _eq_args()) == -1 and b"gamma" in lib.thrl_last_error()
    assert call(one, _eq_args(agents=2)) == -1
    # agent 0 alone, or a per-game gamma array, pass the gamma rule: the next refusal is the missing output
    assert call(one, _eq_args(agents=1, v_on=None)) == -2
    assert call(one, _eq_args(sweep_gamma=FAKE, v_on=None)) == -2
    cfg = _cfg()
    assert call(cfg, _eq_args(n_tuples=4097)) == -3
    assert lib.thrl_tuple_deviation(ctypes.byref(cfg), ctypes.byref(_dev_args(n_tuples=4097)), None) == -3
    wide = _cfg({"agents": [dict(AG, actions=129), dict(AG, actions=32)], "environment": dict(ENV)})
    assert call(wide, _eq_args(n_tuples=4128)) == -3
    assert lib.thrl_tuple_deviation(ctypes.byref(wide), ctypes.byref(_dev_args(n_tuples=4128)), None) == -3


@pytest.mark.parametrize("null", EQ_FIELDS + ("args", "cfg"))
def test_tuple_equilibrium_missing_pointers_are_null(lib, null):
    cfg = _cfg()
    a = None if null == "args" else ctypes.byref(_eq_args(**({null: None} if null in EQ_FIELDS else {})))
    assert lib.thrl_tuple_equilibrium(None if null == "cfg" else ctypes.byref(cfg), a, None) == -2
