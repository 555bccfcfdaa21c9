"""Host side of cross-play (thrl_crossplay, th_rl_amd.crossplay): the pairing designs, option parsing and refusals, the
summary on hand-made arrays, the shard combination and the utils readers, the mirror against self-play, the ctypes
mirror of the args struct and the entry point's validation through the library loaded without a GPU.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import crossplay_mirror as X
import deviation_mirror as M
from th_rl_amd import crossplay as xp

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


# ------------------------------------------------------------------------------------------------ pairings
IDS = np.array([0, 1, 0, 2, 1, 0, 3, 3, 0])           # sizes 4, 2, 1, 2


@pytest.mark.parametrize("scheme", ["rotate", "random"])
@pytest.mark.parametrize("against", ["own", "all"])
@pytest.mark.parametrize("n_agents", [2, 3])
def test_pairings_design(scheme, against, n_agents):
    R = 3
    rounds = xp.pairings(IDS, 4, scheme, R, against, seed=5, n_agents=n_agents)
    assert len(rounds) == (R if against == "own" else 4 * R)
    members = [np.flatnonzero(IDS == k) for k in range(4)]
    for r, s in enumerate(rounds):
        assert s.dtype == np.int32 and s.shape == (n_agents, IDS.size)
        assert s[0].tolist() == list(range(IDS.size))                   # seat 0 = the game itself
        assert s.min() >= 0 and s.max() < IDS.size
        for m in range(IDS.size):
            target = IDS[m] if against == "own" else r // R
            for i in range(1, n_agents):
                assert IDS[s[i, m]] == target, (r, i, m)
        flag = xp.self_seat(s)
        assert flag.tolist() == [any(s[i, m] == m for i in range(1, n_agents)) for m in range(IDS.size)]
        if against == "own":
            assert flag[3]                                              # a group of one game meets itself
    again = xp.pairings(IDS, 4, scheme, R, against, seed=5, n_agents=n_agents)
    assert all(np.array_equal(a, b) for a, b in zip(rounds, again))
    if scheme == "random":
        other = xp.pairings(IDS, 4, scheme, R, against, seed=6, n_agents=n_agents)
        assert any(not np.array_equal(a, b) for a, b in zip(rounds, other))


def test_rotate_is_the_stated_formula():
    rounds = xp.pairings(IDS, 4, "rotate", 3, "own", n_agents=3)
    g0 = [0, 2, 5, 8]
    for k, s in enumerate(rounds, start=1):
        for pos, m in enumerate(g0):
            for i in (1, 2):
                assert s[i, m] == g0[(pos + i * k) % 4]
        # a group of two: k odd swaps the pair, k even seats every game on itself (seat 1), seat 2 moves by 2k: itself
        assert s[1, 1] == (4 if k % 2 else 1) and s[1, 4] == (1 if k % 2 else 4) and s[2, 1] == 1
        assert xp.self_seat(s)[[1, 4]].all()
    allr = xp.pairings(IDS, 4, "rotate", 2, "all")
    assert len(allr) == 8
    s = allr[1 * 2 + 0]                                # target group 1 (games 1, 4), k = 1
    assert s[1].tolist() == [[1, 4][(p + 1) % 2] for p in [0, 0, 1, 0, 1, 2, 0, 1, 3]]
    # a target group without games (a shard that holds none of them): everybody stays at home, flagged
    empty = xp.pairings(np.array([0, 0, 2]), 3, "rotate", 1, "all")[1]
    assert empty.tolist() == [[0, 1, 2], [0, 1, 2]] and xp.self_seat(empty).all()
    with pytest.raises(ValueError):
        xp.pairings(IDS, 3, "rotate", 1)
    with pytest.raises(ValueError):
        xp.pairings(IDS, 4, "swap", 1)
    assert xp.identity(3, 4).tolist() == [[0, 1, 2, 3]] * 3


def test_random_is_a_permutation_of_the_target_group():
    ids = np.repeat([0, 1], [50, 30])
    for s in xp.pairings(ids, 2, "random", 4, "own", seed=3, n_agents=3):
        for i in (1, 2):
            assert sorted(s[i, :50].tolist()) == list(range(50)) and sorted(s[i, 50:].tolist()) == list(range(50, 80))
    s = xp.pairings(ids, 2, "random", 1, "all", seed=3)[1]              # every game against group 1: pos mod 30
    assert set(s[1].tolist()) == set(range(50, 80)) and s[1, 0] == s[1, 30] == s[1, 50]


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_and_refusals(tmp_path):
    assert xp.parse_options(True, CFG) == dict(rounds=8, scheme="rotate", against="own", steps=0, horizon=None, seed=0)
    o = xp.parse_options({"rounds": 2, "scheme": "random", "against": "all", "steps": 5, "horizon": 9, "seed": 4,
                          "tables": "converged"}, CFG)
    assert o == dict(rounds=2, scheme="random", against="all", steps=5, horizon=9, seed=4, tables="converged")
    for bad in ({"rounds": 0}, {"rounds": 1.5}, {"scheme": "swap"}, {"against": "others"}, {"steps": -1},
                {"steps": (1 << 20) + 1}, {"horizon": 0}, {"seed": -1}, {"tables": "best"}, {"agents": [0]}, 5):
        with pytest.raises(ValueError):
            xp.parse_options(bad, CFG)
    with pytest.raises(ValueError, match="follow-up"):
        xp.parse_options(True, MIXED)
    # train_one refuses before it builds a batch (no GPU is touched)
    from th_rl_amd import trainer
    for cfg in (dict(MIXED, training={"epochs": 1, "n_games": 4, "crossplay": True}),
                dict(CFG, training={"epochs": 1, "n_games": 4, "crossplay": {"partners": 3}}),
                dict(CFG, training={"epochs": 1, "n_games": 4, "crossplay": {"tables": "converged"}})):
        (tmp_path / "c.json").write_text(json.dumps(cfg))
        with pytest.raises(ValueError):
            trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))


# ------------------------------------------------------------------------------------------------ summary
def _hand_made():
    """Four games in two groups (0 0 1 1), two rounds; Nash 2, Cartel 4, so delta = (r_0 + r_1 - 2) / 2."""
    seats = np.array([[[0, 1, 2, 3], [1, 0, 3, 2]],          # partners from the own group
                      [[0, 1, 2, 3], [2, 3, 2, 1]]])         # match 2 sits on itself
    mu = np.array([[0, 1, 2, 0], [3, 0, 0, -1]])             # the last match was refused
    lam = np.array([[1, 2, 0, 1], [1, 5, 1, 0]])
    cr = np.array([[[1.0, 2.0, 0.0, 1.5], [1.0, 1.0, 0.0, 1.5]],
                   [[2.0, 1.0, 9.0, 0.0], [2.0, 0.5, 9.0, 0.0]]])
    games = {"seats": seats, "mu": mu, "lam": lam, "cycle_reward": cr}
    self_play = {"lam": np.array([1, 1, 0, 2]), "cycle_reward": np.array([[2.0, 2.0, 0.0, 1.0], [2.0, 1.0, 0.0, 1.0]])}
    return games, self_play


def test_summary_arithmetic():
    games, self_play = _hand_made()
    s = xp.summarize(games, self_play, [0, 0, 1, 1], 2, 2.0, 4.0)
    assert [(r["group"], r["partner_group"]) for r in s] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    a, b, c, d = s
    assert a["matches"] == 2 and a["cycles"] == 2 and a["fixed_points"] == 1
    assert a["lam_hist"] == [0, 1, 1, 0, 0, 0, 0, 0, 0]
    assert a["delta_mean"] == 0.25 and a["delta_q50"] == 0.25          # deltas 0.0 and 0.5
    assert a["delta_self_mean"] == 0.75 and a["retained"] == 0.25 / 0.75   # self deltas 1.0 and 0.5
    # seat 0: (1 - 2 + 2 - 2) / 2; seat 1 holds agent 1 of games 1 and 0: (1 - 1 + 1 - 2) / 2
    assert a["seat_gain"] == [-0.5, -0.5]
    assert b["matches"] == 2 and b["cycles"] == 2 and b["lam_hist"][1] == 1 and b["lam_hist"][5] == 1
    assert b["delta_mean"] == 0.375                                     # (1.0 + -0.25) / 2
    # partners: agent 1 of game 2 has no self-play cycle, so seat 1's mean is over match 1 alone: 0.5 - 1.0
    assert b["seat_gain"] == [(0.0 + -1.0) / 2, -0.5]
    assert c["matches"] == 0 and c["delta_mean"] is None and c["retained"] is None and c["seat_gain"] == [None, None]
    # group 1 at home: round 0 has match 2 (lam 0) and match 3; round 1's match 2 is self-seated, match 3 refused
    assert d["matches"] == 2 and d["cycles"] == 1 and d["lam_hist"][0] == 1 and d["delta_mean"] == 0.5
    assert d["delta_self_mean"] == 0.0 and d["retained"] is None        # the denominator is not positive
    json.dumps(s)
    one = xp.summarize({f: v[0] for f, v in games.items()}, self_play, [0, 0, 1, 1], 2, 2.0, 4.0)
    assert one[0]["matches"] == 2 and one[1]["matches"] == 0


def test_shards_merged_equal_the_whole_for_given_seats(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(3)
    G, H = 24, 60
    q = (250 + rs.randn(G, 2 * 101 * 21)).astype(np.float32)
    s0 = rs.uniform(0, 10, G)
    ids = np.arange(G) % 2
    cuts = ((0, 10), (10, G))
    # partners inside each shard, as the trainer draws them, written as global ids
    shard_seats = [np.stack(xp.pairings(ids[lo:hi], 2, "rotate", 2, "own")) + lo for lo, hi in cuts]
    seats = np.concatenate(shard_seats, axis=-1)

    def play(qq, ss, st):
        rounds = [X.analyse(CFG, qq, s, st, horizon=H) for s in ss]
        g = {f: np.stack([r[f] for r in rounds]) for f in ("mu", "lam", "cycle_reward", "cycle_action")}
        sp = X.analyse(CFG, qq, xp.identity(2, qq.shape[0]), st, horizon=H)
        return g, {f: sp[f] for f in ("mu", "lam", "cycle_reward")}

    whole, whole_self = play(q, seats, s0)
    whole["seats"] = seats
    parts = []
    for (lo, hi), ss in zip(cuts, shard_seats):
        g, sp = play(q[lo:hi], ss - lo, s0[lo:hi])
        parts.append((dict(g, seats=ss), sp))
    merged, merged_self = xp.combine(g for g, _ in parts), xp.combine(s for _, s in parts)
    for f in whole:
        assert np.array_equal(merged[f], whole[f]), f
    for f in whole_self:
        assert np.array_equal(merged_self[f], whole_self[f]), f
    nash, cartel = xp.optimal(CFG)
    summary = xp.summarize(merged, merged_self, ids, 2, nash, cartel)
    assert summary == xp.summarize(whole, whole_self, ids, 2, nash, cartel)
    assert sum(r["matches"] for r in summary) == int(sum((~xp.self_seat(s)).sum() for s in seats))
    # the artefact round trip and the readers, sharded and not
    opt = xp.parse_options({"rounds": 2}, CFG)
    one = tmp_path / "one"
    one.mkdir()
    xp.save_games(str(one), whole, whole_self)
    xp.save_json(str(one / "crossplay.json"), xp.describe(opt, nash, cartel, summary))
    back, back_self = xp.load_games(str(one))
    for f in whole:
        assert np.array_equal(back[f], whole[f]), f
    assert np.load(one / "xplay_cycle.npy").shape == (2, 2, G) and np.load(one / "xplay_seats.npy").dtype == np.int32
    two = tmp_path / "two"
    for r, (g, sp) in enumerate(parts):
        d = two / ("shard%d" % r)
        d.mkdir(parents=True)
        xp.save_games(str(d), g, sp)
        xp.save_json(str(d / "crossplay.json"), xp.describe(opt, nash, cartel, []))
    for rnd in (0, 1):
        a, b = utils.crossplay_games(str(one), rnd), utils.crossplay_games(str(two), rnd)
        assert a.index.tolist() == b.index.tolist() == list(range(G))
        for c in a.columns:
            assert np.array_equal(a[c].to_numpy(), b[c].to_numpy()), c
        assert a["seat_1"].tolist() == seats[rnd, 1].tolist() and a["lam"].tolist() == whole["lam"][rnd].tolist()
    df = utils.crossplay_summary(str(one))
    assert len(df) == 4 and df["matches"].sum() == sum(r["matches"] for r in summary) and "seat_gain_1" in df
    with pytest.raises(KeyError):
        utils.crossplay_games(str(tmp_path), 0)
    with pytest.raises(KeyError):
        utils.crossplay_games(str(one), 2)


# ------------------------------------------------------------------------------------------------ the mirror
def test_mirror_identity_seats_are_the_deviation_mirror_and_strangers_are_not():
    """The condition the device tests rest on, for the fresh headline case: cross-play must not be satisfiable by
    self-play."""
    rs = np.random.RandomState(11)
    G = 203
    q = (250 + rs.randn(G, 2 * 101 * 21)).astype(np.float32)
    s0 = rs.uniform(0, 10, G)
    own = X.analyse(CFG, q, xp.identity(2, G), s0, steps=3)
    dev = M.analyse(CFG, q, s0, steps=2)
    for f in ("mu", "lam", "cycle_reward", "cycle_action"):
        assert np.array_equal(own[f], dev[f]), f
    for k in (1, 7):
        seats = xp.pairings(np.zeros(G, int), 1, "rotate", k)[-1]
        ref = X.analyse(CFG, q, seats, s0)
        assert X.differs_from_self_play(CFG, q, seats, s0, ref).mean() >= 0.5
    assert np.array_equal(X.policies(CFG, q)[:, :101], np.argmax(q[:, :2121].reshape(G, 101, 21), axis=2))


# ------------------------------------------------------------------------------------------------ the entry point
FIELDS = ("seat", "state0", "policy", "mu", "lam", "cycle_reward", "cycle_action")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.CrossplayArgs()
    a.n_games, a.n_matches, a.n_steps, a.horizon = 64, 100, 8, 442
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in FIELDS:
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_matches=0), dict(n_matches=-3), dict(n_games=0), dict(n_games=65), dict(horizon=0),
                                 dict(horizon=(1 << 24) + 1), dict(n_steps=-1), dict(n_steps=(1 << 20) + 1),
                                 dict(row_begin=-1), dict(row_count=-1), dict(row_begin=4, row_count=5),
                                 dict(n_steps=0, row_count=1), dict(flags=2), dict(flags=3), dict(flags=-1)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_crossplay(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


def test_too_many_actions_is_bad_config(lib):
    from th_rl_amd import _lib
    wide = {"agents": [dict(AG, actions=70000), dict(AG)], "environment": dict(ENV)}
    cfg, _ = _lib.cfg_from_config(wide, 64, 0)
    assert lib.thrl_crossplay(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == -1


@pytest.mark.parametrize("null", FIELDS + ("q", "args", "cfg"))
def test_missing_pointers_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    a = None if null == "args" else ctypes.byref(_args(**({null: None} if null in FIELDS else {})))
    assert lib.thrl_crossplay(None if null == "cfg" else ctypes.byref(cfg), q, a, None) == -2
    # with the policies given q may be missing, the policy array may not
    given = _args(flags=1, policy=None)
    assert lib.thrl_crossplay(ctypes.byref(cfg), None, ctypes.byref(given), None) == -2
    assert b"policy" in lib.thrl_last_error()


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %zu %zu %d %d %d %d\\n",'
           'sizeof(thrl_crossplay_args),offsetof(thrl_crossplay_args,seat),offsetof(thrl_crossplay_args,action_rows),'
           'THRL_XPLAY_POLICY_GIVEN,THRL_DEV_MAX_STEPS,THRL_DEV_MAX_HORIZON,THRL_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    A = _lib.CrossplayArgs
    assert got == [ctypes.sizeof(A), A.seat.offset, A.action_rows.offset, _lib.XPLAY_POLICY_GIVEN, _lib.DEV_MAX_STEPS,
                   _lib.DEV_MAX_HORIZON, 4]
    assert "thrl_crossplay" in _lib.SYMBOLS


def test_docs_say_that_shards_pair_inside_themselves():
    from th_rl_amd import launch
    for text in (launch.merge_analysis.__doc__, xp.__doc__, open(os.path.join(ROOT, "README.md")).read(),
                 open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "inside" in text.lower() and "shard" in text.lower()
