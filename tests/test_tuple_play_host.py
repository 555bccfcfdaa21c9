"""Host side of the tuple form of greedy play (th_rl_amd.tuple_play, thrl_tuple_policy / thrl_tuple_walk): the per-config
tables against the golden payoff grid, the tuple order, start tuples, option parsing and refusals, the mirror's known
answers on hand-written strategies, the ctypes mirrors of the two args structs and the entry points' validation through
the library loaded without a GPU.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tuple_play_mirror as TM
from th_rl_amd import tuple_play as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
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


# ------------------------------------------------------------------------------------------------ tables
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_tables_equal_the_golden_payoff_grid():
    d = np.load(os.path.join(GOLDEN, "g1_payoff_grid.npz"))
    t = tp.tables(CFG)
    assert t["T"] == 441 and t["n_actions"].tolist() == [21, 21] and t["kinds"] == ["QTable", "QTable"]
    assert _same_bits(t["price"].reshape(21, 21), d["price"])
    assert _same_bits(t["reward"].reshape(2, 21, 21).transpose(1, 2, 0), d["rewards"])
    assert _same_bits(t["scaled"][0].reshape(21, 21)[:, 0], d["scaled"])
    assert _same_bits(t["scaled"][1].reshape(21, 21)[0, :], d["scaled"])


def test_a_network_scales_by_its_action_count():
    t = tp.tables(MIXED)
    lo, hi, A = 0.2, 0.4, 21
    want = [k / A * (hi - lo) + lo for k in range(A)]                 # Reinforce.scale in Python floats
    assert t["scaled"][1].reshape(21, 21)[0].tolist() == want
    assert t["scaled"][0].reshape(21, 21)[:, 0].tolist() == [k / (A - 1) * (hi - lo) + lo for k in range(A)]
    assert t["kinds"] == ["QTable", "Reinforce"]
    # the price and reward of one tuple by hand, in env_step's order
    k0, k1 = 7, 13
    s0, s1 = k0 / 20 * (hi - lo) + lo, k1 / 21 * (hi - lo) + lo
    ratio = 10.0 / 1.0
    q0, q1 = ratio * s0, ratio * s1
    p = 10.0 - 1.0 * ((0.0 + q0) + q1)
    assert t["price"][k0 * 21 + k1] == p and t["reward"][0][k0 * 21 + k1] == p * q0 and t["reward"][1][k0 * 21 + k1] == p * q1


def test_tuple_order_has_agent_0_slowest():
    cfg = {"agents": [dict(AG, actions=3, action_range=[0.0, 0.2]), dict(RF, actions=4), dict(AG, actions=5)],
           "environment": dict(ENV, nplayers=3)}
    t = tp.tables(cfg)
    assert t["T"] == 60 and t["scaled"].shape == (3, 60) and t["reward"].shape == (3, 60)
    for k0 in range(3):
        for k1 in range(4):
            for k2 in range(5):
                at = (k0 * 4 + k1) * 5 + k2
                assert t["scaled"][0][at] == k0 / 2 * (0.2 - 0.0) + 0.0
                assert t["scaled"][1][at] == k1 / 4 * (0.4 - 0.2) + 0.2
                assert t["scaled"][2][at] == k2 / 4 * (0.4 - 0.2) + 0.2


def test_cac_and_too_many_tuples_raise():
    with pytest.raises(ValueError, match="continuous"):
        tp.tables(CAC)
    with pytest.raises(ValueError, match="4096"):
        tp.tables({"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)})
    assert tp.tables({"agents": [dict(AG, actions=64), dict(AG, actions=64)], "environment": dict(ENV)})["T"] == 4096


# ------------------------------------------------------------------------------------------------ start tuples
def test_start_tuples():
    import torch
    t = tp.tables(CFG)
    price = t["price"]
    # tuples (1, 9) and (0, 10) sell the same quantity: one price, and the first tuple with it is returned
    assert price[1 * 21 + 9] == price[0 * 21 + 10]
    states = np.array([price[0], price[440], price[1 * 21 + 9], 1.2345, np.nextafter(price[5], 11.0), price[200]])
    first = [int(np.flatnonzero(price.view(np.int64) == p.view(np.int64))[0]) for p in states[[0, 1, 2, 5]]]
    want = [first[0], first[1], first[2], -1, -1, first[3]]
    assert first[2] == 10
    got = tp.start_tuples(states, t)
    assert got.dtype == np.int32 and got.tolist() == want
    got_t = tp.start_tuples(torch.from_numpy(states), t)              # a CPU tensor
    assert got_t.dtype == torch.int32 and got_t.tolist() == want

    class Holder:
        state = torch.from_numpy(states)
    assert tp.start_tuples(Holder(), t).tolist() == want


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_and_refusals(tmp_path):
    assert tp.parse_options(True, MIXED) == dict(rounds=0, scheme="rotate", against="own", seed=0, steps=0, horizon=None)
    o = tp.parse_options({"rounds": 2, "scheme": "random", "against": "all", "steps": 5, "horizon": 9, "seed": 4}, CFG)
    assert o == dict(rounds=2, scheme="random", against="all", steps=5, horizon=9, seed=4)
    for bad in ({"rounds": -1}, {"rounds": 1.5}, {"rounds": True}, {"scheme": "swap"}, {"against": "others"}, {"steps": -1},
                {"steps": (1 << 20) + 1}, {"horizon": 0}, {"horizon": (1 << 24) + 1}, {"horizon": 2.5}, {"seed": -1},
                {"tables": "final"}, {"agents": [0]}, 5, "yes"):
        with pytest.raises(ValueError):
            tp.parse_options(bad, MIXED)
    with pytest.raises(ValueError, match="continuous"):
        tp.parse_options(True, CAC)
    with pytest.raises(ValueError, match="4096"):
        tp.parse_options(True, {"agents": [dict(AG, actions=100), dict(RF, actions=21), dict(AG, actions=21)],
                                "environment": dict(ENV, nplayers=3)})
    # train_one refuses before it builds a batch, the launcher before it starts a shard (no GPU is touched)
    from th_rl_amd import launch, trainer
    for cfg in (dict(CAC, training={"epochs": 1, "n_games": 4, "greedy_cycles": True}),
                dict(MIXED, training={"epochs": 1, "n_games": 4, "greedy_cycles": {"partners": 3}}),
                dict(MIXED, training={"epochs": 1, "n_games": 4, "greedy_cycles": {"rounds": -2}})):
        (tmp_path / "c.json").write_text(json.dumps(cfg))
        with pytest.raises(ValueError):
            trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))
    (tmp_path / "l.json").write_text(json.dumps(dict(MIXED, training={"epochs": 1, "n_games": 4, "greedy_cycles": True})))
    with pytest.raises(ValueError, match="greedy_cycles"):
        launch.launch(str(tmp_path / "l.json"), str(tmp_path / "out"), gpus=2)
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------ the mirror
def _strategy(nxt):
    """uint16 [1, 2, 9]: the two agents' entries that send tuple t of the 3 x 3 game to tuple nxt[t]."""
    nxt = np.asarray(nxt)
    return np.stack([nxt // 3, nxt % 3])[None].astype(np.uint16)


def test_mirror_known_answers():
    t = tp.tables(SMALL)
    rew, sca = t["reward"], t["scaled"]
    ident = np.zeros((2, 1), np.int64)
    # a fixed point: everybody plays action 1 everywhere
    pol = _strategy([4] * 9)
    r = TM.analyse(t, pol, ident, [0], steps=3)
    assert (r["mu"][0], r["lam"][0], r["cycle_start"][0]) == (1, 1, 4)
    assert r["cycle_reward"][:, 0].tolist() == rew[:, 4].tolist() and r["cycle_action"][:, 0].tolist() == sca[:, 4].tolist()
    assert r["reward_rows"][:, :, 0].tolist() == [rew[:, 4].tolist()] * 3
    r = TM.analyse(t, pol, ident, [4])
    assert (r["mu"][0], r["lam"][0], r["cycle_start"][0]) == (0, 1, 4)
    # 0 -> 1 -> 2 -> 3 -> 4 -> 3: a 2-cycle reached after 3 steps
    pol = _strategy([1, 2, 3, 4, 3, 0, 0, 0, 0])
    r = TM.analyse(t, pol, ident, [0], steps=6)
    assert (r["mu"][0], r["lam"][0], r["cycle_start"][0]) == (3, 2, 3) and r["horizon"] == 10
    for i in (0, 1):                                # the transition taken at t_k plays t_{k+1}: 4 first, then 3
        assert r["cycle_reward"][i, 0] == ((0.0 + rew[i, 4]) + rew[i, 3]) / 2.0
        assert r["cycle_action"][i, 0] == ((0.0 + sca[i, 4]) + sca[i, 3]) / 2.0
    assert r["reward_rows"][:, 0, 0].tolist() == [rew[0, x] for x in (1, 2, 3, 4, 3, 4)]
    assert r["action_rows"][:, 1, 0].tolist() == [sca[1, x] for x in (1, 2, 3, 4, 3, 4)]
    # the cycle counts only when mu + lam <= horizon
    r = TM.analyse(t, pol, ident, [0], horizon=5)
    assert (r["mu"][0], r["lam"][0]) == (3, 2)
    r = TM.analyse(t, pol, ident, [0], horizon=4)
    assert (r["mu"][0], r["lam"][0], r["cycle_start"][0]) == (4, 0, -1)
    assert r["cycle_reward"][:, 0].tolist() == [0.0, 0.0] and r["cycle_action"][:, 0].tolist() == [0.0, 0.0]
    # entries that are no action are clamped to the last one: (7, 65535) is (2, 2)
    pol = _strategy([4] * 9)
    pol[0, 0, 0], pol[0, 1, 0] = 7, 65535
    r = TM.analyse(t, pol, ident, [0], steps=1)
    assert r["reward_rows"][0, :, 0].tolist() == rew[:, 8].tolist() and (r["mu"][0], r["lam"][0]) == (2, 1)
    # the sentinels: a seat outside the games, a start outside the tuples; the match between them is untouched
    seats = np.array([[0, 0, 0, 0], [1, 0, 0, -1]])
    r = TM.analyse(t, _strategy([4] * 9), seats, [0, 0, 9, 0], steps=2)
    assert r["mu"].tolist() == [-1, 1, -1, -1] and r["lam"].tolist() == [0, 1, 0, 0]
    assert r["cycle_start"].tolist() == [-1, 4, -1, -1]
    assert not r["cycle_reward"][:, [0, 2, 3]].any() and not r["reward_rows"][:, :, [0, 2, 3]].any()
    assert TM.analyse(t, _strategy([4] * 9), ident, [-1])["mu"][0] == -1
    # self-play is told apart from a re-seating
    two = np.concatenate([_strategy([4] * 9), _strategy([8] * 9)])
    seats = np.array([[0, 0], [0, 1]])
    ref = TM.analyse(t, two, seats, [0, 0])
    assert TM.differs_from_self_play(t, two, seats, [0, 0], ref).tolist() == [False, True]


def test_summaries_on_hand_made_arrays():
    self_play = {"mu": np.array([0, 1, -1, 2]), "lam": np.array([1, 2, 0, 0]), "start": np.array([3, 4, -1, 0]),
                 "cycle_reward": np.array([[2.0, 1.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0]])}
    s = tp.summarize_self(self_play, [0, 0, 1, 1], 2, 2.0, 4.0)
    assert s[0]["matches"] == 2 and s[0]["no_start"] == 0 and s[0]["cycles"] == 2 and s[0]["fixed_points"] == 1
    assert s[0]["delta_mean"] == 0.75 and s[0]["lam_hist"][:3] == [0, 1, 1]
    assert s[1]["matches"] == 1 and s[1]["no_start"] == 1 and s[1]["cycles"] == 0 and s[1]["delta_mean"] is None
    games = {"seats": np.array([[[0, 1, 2, 3], [1, 0, 3, 2]]]), "mu": np.array([[0, 0, -1, 1]]),
             "lam": np.array([[1, 1, 0, 1]]), "start": np.array([[3, 4, -1, 0]]),
             "cycle_reward": np.array([[[1.0, 2.0, 0.0, 1.0], [1.0, 2.0, 0.0, 1.0]]])}
    rows = tp.summarize(games, self_play, [0, 0, 1, 1], 2, 2.0, 4.0)
    assert [(r["group"], r["partner_group"], r["matches"], r["no_start"]) for r in rows] == \
        [(0, 0, 2, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 1, 1)]
    assert rows[0]["delta_mean"] == 0.5 and rows[0]["delta_self_mean"] == 0.75 and "seat_gain" in rows[0]
    json.dumps(tp.describe({}, 2.0, 4.0, 9, s, rows))
    both = tp.combine([{"mu": np.array([[1, 2]])}, {"mu": np.array([[3]])}])
    assert both["mu"].tolist() == [[1, 2, 3]]


# ------------------------------------------------------------------------------------------------ the entry points
def test_args_structs_and_limits_match_header():
    from th_rl_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",'
           'sizeof(thrl_tuple_policy_args),offsetof(thrl_tuple_policy_args,kind),offsetof(thrl_tuple_policy_args,nn_params),'
           'offsetof(thrl_tuple_policy_args,price),offsetof(thrl_tuple_policy_args,tuple_policy),'
           'sizeof(thrl_tuple_walk_args),offsetof(thrl_tuple_walk_args,seat),offsetof(thrl_tuple_walk_args,cycle_start),'
           'offsetof(thrl_tuple_walk_args,action_rows),THRL_TP_MAX_TUPLES,THRL_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    P, W = _lib.TuplePolicyArgs, _lib.TupleWalkArgs
    assert got == [ctypes.sizeof(P), P.kind.offset, P.nn_params.offset, P.price.offset, P.tuple_policy.offset,
                   ctypes.sizeof(W), W.seat.offset, W.cycle_start.offset, W.action_rows.offset, 4096, 4]
    assert _lib.TP_MAX_TUPLES == tp.MAX_TUPLES == 4096 and _lib.ABI_VERSION == 4
    assert "thrl_tuple_policy" in _lib.SYMBOLS and "thrl_tuple_walk" in _lib.SYMBOLS


FAKE = 4096                           # never dereferenced: validation fails before any launch


def _policy_args(kinds=(0, 1), **kw):
    from th_rl_amd import _lib
    a = _lib.TuplePolicyArgs()
    a.n_games, a.n_tuples = 64, 441
    for i, k in enumerate(kinds):
        a.kind[i] = k
        if k:
            a.nn_params[i] = FAKE
    a.price, a.tuple_policy = FAKE, FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _cfg(config=None, G=64):
    from th_rl_amd import _lib
    return _lib.cfg_from_config(config or CFG, G, 0)[0]


def test_tuple_policy_refusals(lib):
    cfg = _cfg()
    call = lambda a, q=ctypes.c_void_p(FAKE): lib.thrl_tuple_policy(ctypes.byref(cfg), q, ctypes.byref(a), None)
    assert call(_policy_args(kinds=(0, 3))) == -3 and b"CAC" in lib.thrl_last_error()
    for bad in (dict(n_games=0), dict(n_games=65), dict(n_tuples=0), dict(n_tuples=440), dict(n_tuples=21)):
        assert call(_policy_args(**bad)) == -1, bad
    assert call(_policy_args(n_tuples=4097)) == -3
    assert call(_policy_args(kinds=(0, 4))) == -1 and call(_policy_args(kinds=(-1, 0))) == -1
    wide = _cfg({"agents": [dict(AG, actions=21), dict(AG, actions=33)], "environment": dict(ENV)})
    assert lib.thrl_tuple_policy(ctypes.byref(wide), ctypes.c_void_p(FAKE), ctypes.byref(_policy_args(n_tuples=693)), None) == -1
    assert call(_policy_args(price=None)) == -2 and call(_policy_args(tuple_policy=None)) == -2
    a = _policy_args()
    a.nn_params[1] = None
    assert call(a) == -2 and b"nn_params" in lib.thrl_last_error()
    assert call(_policy_args(), q=None) == -2 and b"q is NULL" in lib.thrl_last_error()
    assert lib.thrl_tuple_policy(ctypes.byref(cfg), ctypes.c_void_p(FAKE), None, None) == -2
    assert lib.thrl_tuple_policy(None, ctypes.c_void_p(FAKE), ctypes.byref(_policy_args()), None) == -2


WALK_FIELDS = ("seat", "start", "tuple_policy", "reward", "scaled", "mu", "lam", "cycle_reward", "cycle_action")


def _walk_args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleWalkArgs()
    a.n_games, a.n_matches, a.n_tuples, a.n_steps, a.horizon = 64, 100, 441, 8, 442
    for f in WALK_FIELDS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_matches=0), dict(n_games=0), dict(horizon=0), dict(horizon=(1 << 24) + 1),
                                 dict(n_steps=-1), dict(n_steps=(1 << 20) + 1), dict(row_begin=-1), dict(row_count=-1),
                                 dict(row_begin=4, row_count=5), dict(n_steps=0, row_count=1), dict(reserved=1),
                                 dict(n_tuples=0), dict(n_tuples=442)])
def test_tuple_walk_bad_arguments_are_bad_config(lib, bad):
    cfg = _cfg()
    assert lib.thrl_tuple_walk(ctypes.byref(cfg), ctypes.byref(_walk_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", WALK_FIELDS + ("args", "cfg"))
def test_tuple_walk_missing_pointers_are_null(lib, null):
    cfg = _cfg()
    a = None if null == "args" else ctypes.byref(_walk_args(**({null: None} if null in WALK_FIELDS else {})))
    assert lib.thrl_tuple_walk(None if null == "cfg" else ctypes.byref(cfg), a, None) == -2


def test_tuple_walk_too_many_tuples_is_unsupported(lib):
    cfg = _cfg()
    assert lib.thrl_tuple_walk(ctypes.byref(cfg), ctypes.byref(_walk_args(n_tuples=4097)), None) == -3
