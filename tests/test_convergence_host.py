"""Host side of convergence tracking (thrl_policy_track, th_rl_amd.convergence): the entry point's export and
validation through the library loaded without a GPU, the ctypes mirror of the args struct, the numpy mirror of the
definitions on hand-built table sequences, option parsing, the group summary, the shard combination, the readers and
the truncation of per-epoch artefacts after an early stop.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import convergence_mirror as M
from th_rl_amd import convergence as cv

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
    a = _lib.PolicyTrackArgs()
    a.n_games, a.flags, a.episode, a.window = 64, 0, 20, 1000
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("policy", "stable_since", "converged_at", "conv_since", "changes"):
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_library_exports_policy_track(lib):
    from th_rl_amd import _lib
    assert "thrl_policy_track" in _lib.SYMBOLS
    assert hasattr(lib, "thrl_policy_track")
    assert lib.thrl_version() == 4


def test_args_struct_matches_header():
    from th_rl_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %zu\\n",'
           'sizeof(thrl_policy_track_args),offsetof(thrl_policy_track_args,state_conv));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, off = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert size == ctypes.sizeof(_lib.PolicyTrackArgs)
    assert off == _lib.PolicyTrackArgs.state_conv.offset


@pytest.mark.parametrize("bad", [dict(window=0), dict(window=-5), dict(n_games=0), dict(n_games=65), dict(flags=2),
                                 dict(flags=-1), dict(q_conv=4096), dict(q_conv=4096, state=4096),
                                 dict(q_conv=4096, state_conv=4096)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_policy_track(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("actions", [32001, 65536, 65537, 70000])
def test_actions_beyond_a_16_bit_entry_are_bad_config(lib, actions):
    # the contract refuses more than 65,536 actions; the library's config check (at most 32,000 per agent) is what
    # refuses them, so every action index that reaches the kernel fits a 16-bit policy entry
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    cfg.n_actions[1] = actions
    assert lib.thrl_policy_track(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == -1
    assert b"actions" in lib.thrl_last_error()
    cfg.n_actions[1] = 32000          # the largest grid is accepted by validation (fails later only on the NULL q)
    assert lib.thrl_policy_track(ctypes.byref(cfg), None, ctypes.byref(_args()), None) == -2


@pytest.mark.parametrize("null", ["q", "policy", "stable_since", "converged_at", "conv_since", "changes", "args"])
def test_missing_arrays_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    a = None if null == "args" else ctypes.byref(_args(**({} if null in ("q", "args") else {null: None})))
    assert lib.thrl_policy_track(ctypes.byref(cfg), q, a, None) == -2


# ------------------------------------------------------------------------------------------------ the mirror
SHAPES = [(3, 4), (2, 3)]               # two agents: 3 rows x 4 actions, 2 rows x 3 actions
OFFSETS = [0, 12]
STRIDE = 18


def _tables(rows0, rows1):
    """One game's flat tables with a one-hot maximum at the given action of every row."""
    q = np.zeros(STRIDE)
    for r, a in enumerate(rows0):
        q[r * 4 + a] = 1.0
    for r, a in enumerate(rows1):
        q[12 + r * 3 + a] = 1.0
    return q[None, :]


def test_mirror_ties_take_the_first_maximum():
    q = np.zeros((1, STRIDE))
    q[0, 1] = q[0, 3] = 2.0                      # row 0 of agent 0: tie between actions 1 and 3
    q[0, 12 + 3:12 + 6] = [-0.0, 0.0, -1.0]      # row 1 of agent 1: -0.0 == 0.0, first wins
    pol = M.policy_of(q, SHAPES, OFFSETS)
    assert pol.dtype == np.uint16 and pol.tolist() == [[1, 0, 0, 0, 0]]


def test_mirror_change_in_one_row_of_one_agent():
    m = M.Mirror(_tables([0, 1, 2], [0, 1]), SHAPES, OFFSETS, episode=0, window=10)
    assert m.check(_tables([0, 1, 2], [0, 1]), 5) == 0
    assert m.stable_since.tolist() == [0] and m.changes.tolist() == [0]
    assert m.check(_tables([0, 1, 2], [0, 2]), 10) == 0      # agent 1, row 1 only
    assert m.stable_since.tolist() == [10] and m.changes.tolist() == [1]
    assert m.policy.tolist() == [[0, 1, 2, 0, 2]]


def test_mirror_change_that_reverts_between_checks_is_not_seen():
    m = M.Mirror(_tables([0, 1, 2], [0, 1]), SHAPES, OFFSETS, episode=0, window=10)
    # the tables change at episode 3 and change back at episode 7; the checks are at 5k
    assert m.check(_tables([0, 1, 2], [0, 1]), 5) == 0
    assert m.check(_tables([0, 1, 2], [0, 1]), 10) == 1
    assert m.changes.tolist() == [0] and m.converged_at.tolist() == [10] and m.conv_since.tolist() == [0]


def test_mirror_converges_exactly_at_the_window():
    m = M.Mirror(_tables([0, 0, 0], [0, 0]), SHAPES, OFFSETS, episode=4, window=6)
    assert m.check(_tables([1, 0, 0], [0, 0]), 5) == 0       # changed: stable since 5
    assert m.check(_tables([1, 0, 0], [0, 0]), 10) == 0      # 10 - 5 = 5 < 6
    assert m.converged_at.tolist() == [-1]
    assert m.check(_tables([1, 0, 0], [0, 0]), 11) == 1      # 11 - 5 = 6 = W
    assert m.converged_at.tolist() == [11] and m.conv_since.tolist() == [5]


def test_mirror_changes_after_convergence_keep_the_first():
    m = M.Mirror(_tables([0, 0, 0], [0, 0]), SHAPES, OFFSETS, episode=0, window=2, state=[1.0], snapshot=True)
    q_conv = _tables([0, 0, 0], [0, 0])
    assert m.check(q_conv, 2, state=[3.5]) == 1
    assert m.check(_tables([0, 0, 3], [0, 0]), 4, state=[4.0]) == 1
    assert m.check(_tables([0, 0, 3], [0, 0]), 8, state=[4.5]) == 1     # stable again: still one convergence
    assert m.converged_at.tolist() == [2] and m.conv_since.tolist() == [0]
    assert m.stable_since.tolist() == [4] and m.changes.tolist() == [1]
    assert np.array_equal(m.q_conv, q_conv) and m.state_conv.tolist() == [3.5]


def test_mirror_counts_games_independently():
    q0 = np.concatenate([_tables([0, 0, 0], [0, 0]), _tables([1, 1, 1], [1, 1])])
    m = M.Mirror(q0, SHAPES, OFFSETS, episode=0, window=3)
    q1 = np.concatenate([_tables([0, 0, 0], [0, 0]), _tables([1, 1, 1], [1, 0])])
    assert m.check(q1, 3) == 1
    assert m.converged_at.tolist() == [3, -1] and m.stable_since.tolist() == [0, 3] and m.changes.tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_defaults():
    o = cv.parse_options(True, CFG)
    assert o == {"window": 1000, "every": 20, "stop": None, "snapshot": False}
    one = dict(CFG, environment=dict(ENV, max_steps=1))
    assert cv.parse_options({}, one)["window"] == 100000
    odd = dict(CFG, environment=dict(ENV, max_steps=7))
    assert cv.parse_options({}, odd)["window"] == 14286
    o = cv.parse_options({"window": 5, "every": 3, "stop": 1, "snapshot": True}, CFG)
    assert o == {"window": 5, "every": 3, "stop": 1.0, "snapshot": True}


@pytest.mark.parametrize("bad", [{"window": 0}, {"every": 0}, {"every": 2.5}, {"window": True}, {"stop": 0},
                                 {"stop": 1.5}, {"stop": -0.1}, {"stop": True}, {"snapshot": 1}, {"nope": 1}, 3])
def test_parse_options_refuses(bad):
    with pytest.raises(ValueError):
        cv.parse_options(bad, CFG)


def test_neural_configs_are_refused_before_training():
    with pytest.raises(ValueError, match="QTable agents only"):
        cv.parse_options(True, MIXED)


def test_every_rounds_up_to_the_training_cycle():
    assert cv.every_used(20, 1) == 20
    assert cv.every_used(20, 0) == 20
    assert cv.every_used(20, 8) == 24
    assert cv.every_used(1, 5) == 5
    assert cv.every_used(10, 5) == 10


def test_deviation_tables_option():
    from th_rl_amd import deviation as dv
    assert "tables" not in dv.parse_options(True, CFG)                 # deviation.json of main's runs unchanged
    assert dv.parse_options({"tables": "converged"}, CFG)["tables"] == "converged"
    with pytest.raises(ValueError):
        dv.parse_options({"tables": "latest"}, CFG)


# ------------------------------------------------------------------------------------------------ summary
def _games(G, rs):
    ca = np.where(rs.rand(G) < 0.6, rs.randint(0, 50, G) * 20, -1).astype(np.int64)
    cs = np.where(ca >= 0, np.maximum(ca - 1000, 0), -1).astype(np.int64)
    ss = rs.randint(0, 60, G).astype(np.int64) * 20
    ch = rs.randint(0, 9, G).astype(np.int32)
    return {"converged_at": ca, "conv_since": cs, "stable_since": ss, "changes": ch}


def test_summary_by_hand():
    games = {"converged_at": np.array([100, -1, 60, 40]), "conv_since": np.array([0, -1, 20, 0]),
             "stable_since": np.array([0, 90, 20, 100]), "changes": np.array([0, 4, 1, 2])}
    s = cv.summarize(games, [0, 0, 1, 1], 2, 40, 120)
    assert s[0]["games"] == 2 and s[0]["converged"] == 1 and s[0]["fraction"] == 0.5
    assert s[0]["converged_at_mean"] == 100 and s[0]["conv_since_q50"] == 0
    assert s[0]["still_stable"] == 1 and s[0]["changes_mean"] == 2.0
    assert s[1]["converged"] == 2 and s[1]["converged_at_mean"] == 50 and s[1]["converged_at_q25"] == 45
    assert s[1]["still_stable"] == 1 and s[1]["conv_since_mean"] == 10
    empty = cv.summarize(games, [0, 0, 0, 0], 2, 40, 120)[1]
    assert empty["games"] == 0 and empty["fraction"] is None and empty["converged_at_mean"] is None
    none = cv.summarize({k: v[1:2] for k, v in games.items()}, [0], 1, 40, 120)[0]
    assert none["converged"] == 0 and none["converged_at_q75"] is None and none["still_stable"] == 0


def test_combine_over_shards_equals_one_run():
    rs = np.random.RandomState(3)
    G = 50
    g = _games(G, rs)
    ids = rs.randint(0, 3, G)
    parts = [{f: v[lo:hi] for f, v in g.items()} for lo, hi in ((0, 17), (17, 18), (18, 50))]
    merged = cv.combine(parts)
    assert all(np.array_equal(merged[f], g[f]) for f in g)
    assert cv.summarize(merged, ids, 3, 1000, 1200) == cv.summarize(g, ids, 3, 1000, 1200)


def _write_run(d, games, offset=0, shard=False):
    os.makedirs(d, exist_ok=True)
    cv.save_games(d, games)
    cfg = dict(CFG, training={"game_offset": offset, "convergence": True})
    with open(os.path.join(d, "shard_config.json" if shard else "config.json"), "w") as f:
        json.dump(cfg, f)


def test_readers_on_synthetic_files(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(11)
    G = 40
    g = _games(G, rs)
    one = tmp_path / "one"
    _write_run(str(one), g)
    opt = cv.parse_options(True, CFG)
    summary = cv.summarize(g, np.zeros(G, int), 1, opt["window"], 1200)
    cv.save_json(str(one / "convergence.json"), cv.describe(opt, 20, 1200, 1200, False, summary))
    df = utils.convergence_summary(str(one))
    assert len(df) == 1 and df["games"].tolist() == [G] and df["converged"].iloc[0] == np.sum(g["converged_at"] >= 0)
    assert df["window"].iloc[0] == 1000 and df["every_used"].iloc[0] == 20 and not df["stopped_early"].iloc[0]
    games = utils.convergence_games(str(one))
    assert games.index.tolist() == list(range(G))
    assert all(games[f].tolist() == g[f].tolist() for f in cv.FILES)
    assert np.load(str(one / "conv_changes.npy")).dtype == np.int32
    assert np.load(str(one / "conv_episode.npy")).dtype == np.int64
    two = tmp_path / "two"
    for r, (lo, hi) in enumerate(((0, 15), (15, 40))):
        _write_run(str(two / ("shard%d" % r)), {f: v[lo:hi] for f, v in g.items()}, offset=lo, shard=True)
    g2 = utils.convergence_games(str(two))
    assert g2.index.tolist() == list(range(G))
    assert g2.equals(games)
    with pytest.raises(KeyError):
        utils.convergence_games(str(tmp_path / "nothing"))


def test_truncate_rows_keeps_the_first_rows(tmp_path):
    from numpy.lib.format import open_memmap
    p = str(tmp_path / "game_rewards.npy")
    a = open_memmap(p, mode="w+", dtype=np.float64, shape=(10, 2, 3))
    a[:] = np.arange(60).reshape(10, 2, 3)
    a.flush()
    del a
    cv.truncate_rows(p, 4)
    b = np.load(p)
    assert b.shape == (4, 2, 3) and np.array_equal(b, np.arange(24).reshape(4, 2, 3))
    h = str(tmp_path / "group_hist.npy")
    np.save(h, np.arange(30, dtype=np.uint32).reshape(5, 1, 6))
    cv.truncate_rows(h, 5)                               # already that long: untouched
    assert np.load(h).shape == (5, 1, 6)
    cv.truncate_rows(h, 0)
    assert np.load(h).shape == (0, 1, 6) and np.load(h).dtype == np.uint32
