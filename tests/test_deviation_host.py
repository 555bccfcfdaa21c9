"""Host side of the deviation analysis (thrl_deviation, th_rl_amd.deviation): the entry point's validation through the
library loaded without a GPU, the ctypes mirror of the args struct, the numpy mirror against hand-derived answers,
option parsing, the summary and profit-gain formulas, the shard combination and the utils readers.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import deviation_mirror as M
from th_rl_amd import deviation as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.DeviationArgs()
    a.n_games, a.deviator, a.dev_len, a.n_steps, a.horizon, a.dev_action = 64, 0, 1, 32, 442, -1
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("state0", "mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev", "cycle_reward", "cycle_action", "gain"):
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(deviator=-1), dict(deviator=2), dict(dev_len=0), dict(n_steps=0),
                                 dict(dev_len=5, n_steps=4), dict(n_steps=(1 << 20) + 1), dict(horizon=0),
                                 dict(horizon=(1 << 24) + 1), dict(dev_action=-2), dict(dev_action=21),
                                 dict(row_begin=-1), dict(row_count=-1), dict(row_begin=30, row_count=3),
                                 dict(n_games=0), dict(n_games=65)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_deviation(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", ["q", "state0", "mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev",
                                  "cycle_reward", "cycle_action", "gain", "args"])
def test_missing_outputs_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    a = None if null == "args" else ctypes.byref(_args(**({} if null in ("q", "args") else {null: None})))
    assert lib.thrl_deviation(ctypes.byref(cfg), q, a, None) == -2


def test_args_struct_matches_header():
    from th_rl_amd import _lib
    src = '#include <stdio.h>\n#include "thrl.h"\nint main(){printf("%zu\\n",sizeof(thrl_deviation_args));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size = int(subprocess.check_output([os.path.join(d, "s")]).split()[0])
    assert size == ctypes.sizeof(_lib.DeviationArgs)


# ------------------------------------------------------------------------------------------------ the mirror
def test_mirror_punishment_that_returns():
    r = M.analyse(M.KNOWN, M.one_hot_tables(M.PUNISH_2), [5.0], steps=5, dev_len=1, action=2)
    assert (r["mu"][0], r["lam"][0], r["mu_post"][0], r["lam_post"][0], r["ret_step"][0], r["act_dev"][0]) == (0, 1, 2, 1, 3, 2)
    assert r["gain"][0] == -6.25                                  # -12.5 * gamma: one period of punishment at 0
    assert r["cycle_reward"][:, 0].tolist() == [12.5, 12.5] and r["cycle_action"][:, 0].tolist() == [0.25, 0.25]
    assert r["reward_rows"][:, :, 0].tolist() == [[12.5, 6.25], [0, 0], [12.5, 12.5], [12.5, 12.5], [12.5, 12.5]]
    assert r["action_rows"][:, :, 0].tolist() == [[0.5, 0.25], [0.5, 0.5], [0.25, 0.25], [0.25, 0.25], [0.25, 0.25]]


def test_mirror_grim_trigger_never_returns():
    r = M.analyse(M.KNOWN, M.one_hot_tables(M.GRIM), [5.0], steps=5, dev_len=1, action=2)
    assert (r["lam"][0], r["mu_post"][0], r["lam_post"][0], r["ret_step"][0]) == (1, 1, 1, -1)
    assert r["gain"][0] == -12.5 * (0.5 + 0.25 + 0.125 + 0.0625)


def test_mirror_two_cycle_and_horizon():
    r = M.analyse(M.KNOWN, M.one_hot_tables(M.CYCLE_2, 2), [5.0, 10.0], steps=4, action=2)
    assert r["mu"].tolist() == [0, 1] and r["lam"].tolist() == [2, 2]
    assert r["cycle_reward"].tolist() == [[6.25, 6.25]] * 2 and r["cycle_action"].tolist() == [[0.375, 0.375]] * 2
    short = M.analyse(M.KNOWN, M.one_hot_tables(M.CYCLE_2), [10.0], steps=4, action=2, horizon=2)
    assert (short["mu"][0], short["lam"][0], short["ret_step"][0]) == (2, 0, -1)
    assert short["cycle_reward"][:, 0].tolist() == [0.0, 0.0]
    enough = M.analyse(M.KNOWN, M.one_hot_tables(M.CYCLE_2), [10.0], steps=4, action=2, horizon=3)
    assert (enough["mu"][0], enough["lam"][0]) == (1, 2)


def test_default_horizon():
    assert dv.default_horizon([21, 21]) == 442
    assert dv.default_horizon([3]) == 4
    assert dv.default_horizon([300, 300]) == 65536


# ------------------------------------------------------------------------------------------------ options
def test_parse_options():
    o = dv.parse_options(True, CFG)
    assert o == dict(agents=[0, 1], steps=32, dev_len=1, action="best_response", horizon=None)
    o = dv.parse_options({"agents": [1], "steps": 8, "dev_len": 3, "action": 4, "horizon": 100}, CFG)
    assert o == dict(agents=[1], steps=8, dev_len=3, action=4, horizon=100)
    for bad in ({"agents": [2]}, {"dev_len": 9, "steps": 8}, {"dev_len": 0}, {"action": 21}, {"action": "nash"},
                {"horizon": 0}, {"nope": 1}, "yes"):
        with pytest.raises(ValueError):
            dv.parse_options(bad, CFG)
    with pytest.raises(ValueError, match="follow-up"):
        dv.parse_options(True, MIXED)


def test_train_one_refuses_neural_config_before_training(tmp_path, monkeypatch):
    from th_rl_amd import trainer
    ran = []
    monkeypatch.setattr(trainer, "GameBatch", lambda *a, **k: ran.append(1))
    cfg = dict(MIXED, training={"epochs": 3, "n_games": 4, "seed": 1, "deviation": True})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="QTable"):
        trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))
    assert not ran and not os.path.exists(tmp_path / "run" / "log.csv")


# ------------------------------------------------------------------------------------------------ summary
def _games(G, rs):
    return {"mu": rs.randint(0, 5, G).astype(np.int32), "lam": rs.choice([0, 1, 2, 7, 70], G).astype(np.int32),
            "mu_post": rs.randint(0, 5, G).astype(np.int32), "lam_post": rs.randint(0, 3, G).astype(np.int32),
            "ret_step": rs.choice([-1, 1, 4], G).astype(np.int32), "act_dev": rs.randint(0, 21, G).astype(np.int32),
            "gain": rs.normal(size=G), "cycle_reward": rs.uniform(10, 14, (2, G)), "cycle_action": rs.uniform(size=(2, G))}


def test_profit_gain_and_optimal():
    nash, cartel = dv.optimal(CFG)
    assert abs(nash - 200 / 9) < 1e-12 and cartel == 25.0
    cr = np.array([[nash / 2, 12.5, 10.0], [nash / 2, 12.5, 10.0]])
    d = dv.profit_gain(cr, nash, cartel)
    assert d[1] == 1.0 and abs(d[0]) < 1e-15
    assert d[2] == (20.0 - nash) / (cartel - nash)


def test_summary_formulas():
    rs = np.random.RandomState(3)
    G = 500
    g = _games(G, rs)
    ids = rs.randint(0, 3, G)
    nash, cartel = dv.optimal(CFG)
    s = dv.summarize(g, ids, 3, nash, cartel, deviator=1)
    assert [r["group"] for r in s] == [0, 1, 2] and all(r["deviator"] == 1 for r in s)
    delta = (g["cycle_reward"][0] + g["cycle_reward"][1] - nash) / (cartel - nash)
    for k, r in enumerate(s):
        m = ids == k
        lam, ret, gain = g["lam"][m], g["ret_step"][m], g["gain"][m]
        assert r["games"] == m.sum() and r["cycles"] == np.sum(lam > 0) and r["fixed_points"] == np.sum(lam == 1)
        assert r["returned"] == np.sum(ret >= 0) and r["unprofitable"] == np.sum(gain < 0)
        assert r["lam_hist"] == [np.sum(lam == 0), np.sum(lam == 1), np.sum(lam == 2), 0, 0, np.sum(lam == 7), 0, 0,
                                 np.sum(lam == 70)]
        assert r["ret_step_mean"] == ret[ret >= 0].mean()
        dk = delta[m][lam > 0]
        assert r["delta_mean"] == dk.mean()
        assert [r["delta_q25"], r["delta_q50"], r["delta_q75"]] == np.quantile(dk, [0.25, 0.5, 0.75]).tolist()
        assert r["gain_mean"] == gain.mean()
    empty = dv.summarize(g, np.zeros(G, int), 2, nash, cartel, 0)[1]
    assert empty["games"] == 0 and empty["delta_mean"] is None and empty["ret_step_mean"] is None


def test_shard_combination_is_exact():
    rs = np.random.RandomState(5)
    g = _games(301, rs)
    ids = rs.randint(0, 4, 301)
    nash, cartel = dv.optimal(CFG)
    parts = [{f: v[..., lo:hi] for f, v in g.items()} for lo, hi in ((0, 100), (100, 250), (250, 301))]
    c = dv.combine(parts)
    for f in g:
        assert np.array_equal(c[f], g[f]), f
    assert dv.summarize(c, ids, 4, nash, cartel, 0) == dv.summarize(g, ids, 4, nash, cartel, 0)


# ------------------------------------------------------------------------------------------------ readers
def _write_run(d, g, config, opt, offset=0, shard=False):
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "dev_cycle.npy"), np.stack([g["mu"], g["lam"]]))
    np.save(os.path.join(d, "dev_cycle_reward.npy"), g["cycle_reward"])
    np.save(os.path.join(d, "dev_cycle_action.npy"), g["cycle_action"])
    for k in opt["agents"]:
        np.save(os.path.join(d, "dev%d_post.npy" % k), np.stack([g["mu_post"], g["lam_post"], g["ret_step"], g["act_dev"]]))
        np.save(os.path.join(d, "dev%d_gain.npy" % k), g["gain"])
    cfg = dict(config, training={"game_offset": offset})
    with open(os.path.join(d, "shard_config.json" if shard else "config.json"), "w") as f:
        json.dump(cfg, f)


def test_readers_on_synthetic_files(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(7)
    G = 40
    g = _games(G, rs)
    opt = dv.parse_options({"agents": [0, 1]}, CFG)
    nash, cartel = dv.optimal(CFG)
    one = tmp_path / "one"
    _write_run(str(one), g, CFG, opt)
    summary = dv.summarize(g, np.zeros(G, int), 1, nash, cartel, 0) + dv.summarize(g, np.zeros(G, int), 1, nash, cartel, 1)
    dv.save_json(str(one / "deviation.json"), dv.describe(dict(opt, horizon_used=442), nash, cartel, summary))
    df = utils.deviation_summary(str(one))
    assert len(df) == 2 and df["deviator"].tolist() == [0, 1] and df["games"].tolist() == [G, G]
    assert df["lam_0"].iloc[0] == np.sum(g["lam"] == 0) and df["lam_>64"].iloc[0] == np.sum(g["lam"] > 64)
    assert df["Cartel"].iloc[0] == 25.0
    games = utils.deviation_games(str(one), 1)
    assert games.index.tolist() == list(range(G))
    assert games["lam"].tolist() == g["lam"].tolist() and games["gain"].tolist() == g["gain"].tolist()
    assert games["cycle_reward_1"].tolist() == g["cycle_reward"][1].tolist()
    assert np.array_equal(games["delta"].to_numpy(), dv.profit_gain(g["cycle_reward"], nash, cartel))
    # a sharded run: per-game files in shard*/ with their global offsets
    two = tmp_path / "two"
    for r, (lo, hi) in enumerate(((0, 15), (15, 40))):
        _write_run(str(two / ("shard%d" % r)), {f: v[..., lo:hi] for f, v in g.items()}, CFG, opt, offset=lo, shard=True)
    g2 = utils.deviation_games(str(two), 1)
    assert g2.index.tolist() == list(range(G))
    assert g2.equals(games)
    with pytest.raises(KeyError):
        utils.deviation_games(str(tmp_path / "nothing"))
