"""Host side of the attractor analysis in tuple form (th_rl_amd.tuple_analysis, thrl_tuple_attractors): the numpy mirror's
known answers on hand-written maps, that random maps are no degenerate input for it, option parsing and refusals, the
summary rows, the ctypes mirror of the args struct against the header and the entry point's validation through the
library loaded without a GPU.  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tuple_attractors_mirror as AM
from th_rl_amd import tuple_analysis as ta, tuple_play as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
RF = dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])
MIXED = {"agents": [dict(AG), dict(RF)], "environment": dict(ENV)}
CAC = {"agents": [dict(AG), dict(name="CAC", gamma=0.99, states=1, action_range=[0.2, 0.4])], "environment": dict(ENV)}
WIDE = {"agents": [dict(AG, actions=129), dict(RF, actions=32)], "environment": dict(ENV)}     # 4128 tuples
FOUR = {"agents": [dict(AG, actions=2), dict(AG, actions=2)], "environment": dict(ENV)}
TEN = {"agents": [dict(AG, actions=2), dict(AG, actions=5)], "environment": dict(ENV)}
KEEP = 8


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _strategy(nxt, second):
    """uint16 [1, 2, T]: the two agents' entries that send tuple t to tuple nxt[t]; `second` = agent 1's action count."""
    nxt = np.asarray(nxt)
    return np.stack([nxt // second, nxt % second])[None].astype(np.uint16)


# ------------------------------------------------------------------------------------------------ mirror, known answers
def test_the_identity_has_four_attractors_ordered_by_rep():
    t = tp.tables(FOUR)
    w = np.array([0.1, 0.2, 0.3, 0.4])
    r = AM.analyse(t, _strategy([0, 1, 2, 3], 2), [2], start_w=w, policies=True)
    assert (r["n_attr"][0], r["mu_max"][0], r["n_cycle_states"][0]) == (4, 0, 4)
    assert r["rep"][:, 0].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    assert r["lam"][:, 0].tolist() == [1] * 4 + [0] * 4 and r["basin"][:, 0].tolist() == [1] * 4 + [0] * 4
    for k in range(4):
        assert r["cycle_reward"][k, :, 0].tolist() == t["reward"][:, k].tolist()
        assert r["cycle_action"][k, :, 0].tolist() == t["scaled"][:, k].tolist()
    assert not r["cycle_reward"][4:].any() and not r["cycle_action"][4:].any()
    assert (r["rep_x0"][0], r["mu_x0"][0], r["slot_x0"][0]) == (2, 0, 2)
    assert r["start_mass"][:, 0].tolist() == [0.1, 0.2, 0.3, 0.4, 0, 0, 0, 0] and r["start_mass_other"][0] == 0.0
    r0 = t["reward"][0]
    assert r["start_reward"][0, 0] == (((0.0 + 0.1 * r0[0]) + 0.2 * r0[1]) + 0.3 * r0[2]) + 0.4 * r0[3]
    assert r["tuple_rep"][0].tolist() == [0, 1, 2, 3] and r["tuple_mu"][0].tolist() == [0] * 4


def test_a_single_four_cycle():
    t = tp.tables(FOUR)
    r = AM.analyse(t, _strategy([1, 2, 3, 0], 2), [3], start_w=np.full(4, 0.25), policies=True)
    assert (r["n_attr"][0], r["mu_max"][0], r["n_cycle_states"][0]) == (1, 0, 4)
    assert (r["rep"][0, 0], r["lam"][0, 0], r["basin"][0, 0]) == (0, 4, 4) and (r["rep"][1:, 0] == -1).all()
    for tab, f in ((t["reward"], "cycle_reward"), (t["scaled"], "cycle_action")):
        for i in (0, 1):
            x = tab[i]
            assert r[f][0, i, 0] == ((((0.0 + x[1]) + x[2]) + x[3]) + x[0]) / 4.0      # from F(rep), the rep last
    assert (r["rep_x0"][0], r["mu_x0"][0], r["slot_x0"][0]) == (0, 0, 0)
    assert r["start_mass"][0, 0] == 1.0 and r["start_mass_other"][0] == 0.0
    c = r["cycle_reward"][0, 1, 0]
    assert r["start_reward"][1, 0] == (((0.0 + 0.25 * c) + 0.25 * c) + 0.25 * c) + 0.25 * c
    assert r["tuple_rep"][0].tolist() == [0] * 4


def test_a_chain_into_a_fixed_point_and_starts_without_a_tuple():
    t = tp.tables(FOUR)
    pol = np.concatenate([_strategy([0, 0, 1, 2], 2)] * 3)
    r = AM.analyse(t, pol, [3, -1, 4], policies=True)
    assert r["n_attr"].tolist() == [1] * 3 and r["mu_max"].tolist() == [3] * 3 and r["n_cycle_states"].tolist() == [1] * 3
    assert r["tuple_mu"][0].tolist() == [0, 1, 2, 3] and r["tuple_rep"][0].tolist() == [0] * 4
    assert (r["rep"][0, 0], r["lam"][0, 0], r["basin"][0, 0]) == (0, 1, 4)
    assert r["cycle_reward"][0, :, 0].tolist() == t["reward"][:, 0].tolist()
    assert r["rep_x0"].tolist() == [0, -1, -1] and r["mu_x0"].tolist() == [3, -1, -1] and r["slot_x0"].tolist() == [0, -1, -1]
    assert "start_mass" not in r
    # an entry at or above the agent's action count is clamped to its last action
    hi = pol.copy()
    hi[0, :, 3] = (7, 9)                                                # -> (1, 1) = tuple 3: a second fixed point
    r = AM.analyse(t, hi, [3, 3, 3])
    assert r["n_attr"].tolist() == [2, 1, 1] and r["rep"][:2, 0].tolist() == [0, 3] and r["basin"][:2, 0].tolist() == [3, 1]


def test_ties_between_basins_go_to_the_smaller_rep_and_a_larger_basin_comes_first():
    t = tp.tables(FOUR)
    r = AM.analyse(t, _strategy([1, 0, 3, 2], 2), [2])
    assert r["n_attr"][0] == 2 and r["rep"][:2, 0].tolist() == [0, 2] and r["basin"][:2, 0].tolist() == [2, 2]
    assert r["lam"][:2, 0].tolist() == [2, 2] and r["slot_x0"][0] == 1 and r["rep_x0"][0] == 2
    x = t["reward"][1]
    assert r["cycle_reward"][1, 1, 0] == ((0.0 + x[3]) + x[2]) / 2.0
    r = AM.analyse(t, _strategy([0, 3, 3, 3], 2), [0])
    assert r["rep"][:2, 0].tolist() == [3, 0] and r["basin"][:2, 0].tolist() == [3, 1] and r["slot_x0"][0] == 1
    assert r["mu_max"][0] == 1


def test_ten_fixed_points_against_eight_slots():
    t = tp.tables(TEN)
    assert t["T"] == 10
    w = np.arange(1, 11) / 64.0
    r = AM.analyse(t, _strategy(np.arange(10), 5), [9], start_w=w)
    assert r["n_attr"][0] == 10 and r["rep"][:, 0].tolist() == list(range(8)) and r["n_cycle_states"][0] == 10
    assert (r["rep_x0"][0], r["mu_x0"][0], r["slot_x0"][0]) == (9, 0, -1)
    assert r["start_mass"][:, 0].tolist() == w[:8].tolist()
    assert r["start_mass_other"][0] == (0.0 + w[8]) + w[9] and r["start_mass_other"][0] > 0
    want = 0.0
    for k in range(10):                                                  # every tuple, kept or not
        want = want + w[k] * t["reward"][0, k]
    assert r["start_reward"][0, 0] == want


# ------------------------------------------------------------------------------------------------ random maps
def random_policy(actions, seed, n_games=203):
    """uint16 [G, N, T]: per game, per agent i in order, rs.randint(0, A_i, T)."""
    rs = np.random.RandomState(seed)
    T = int(np.prod(actions))
    return np.stack([np.stack([rs.randint(0, A, T) for A in actions]) for _ in range(n_games)]).astype(np.uint16)


def random_tables(actions, seed):
    """Per-config tables of a game with these action counts whose rewards and scaled actions are random numbers."""
    rs = np.random.RandomState(seed + 1000)
    T = int(np.prod(actions))
    return dict(T=T, n_actions=np.asarray(actions, np.int32), reward=rs.uniform(0.0, 3.0, (len(actions), T)),
                scaled=rs.uniform(0.0, 1.0, (len(actions), T)))


@pytest.mark.parametrize("actions,seed", [((21, 21), 17), ((21, 5), 18), ((7, 11, 5), 19)])
def test_random_maps_are_not_degenerate(actions, seed):
    pol = random_policy(actions, seed)
    T = int(np.prod(actions))
    multi = cyc = deep = tie = 0
    for g in range(pol.shape[0]):
        rep, mu, lam = AM.structure(AM.greedy_map(actions, pol[g]))
        basin = sorted(int(np.sum(rep == r)) for r in lam)
        multi += len(lam) >= 2
        cyc += max(lam.values()) > 1
        deep += mu.max() >= 8
        tie += len(set(basin)) < len(basin)
    G = float(pol.shape[0])
    print("T=%d: n_attr >= 2 %.2f, lam > 1 %.2f, mu_max >= 8 %.2f, equal basins %.2f" % (T, multi / G, cyc / G, deep / G, tie / G))
    assert multi / G >= 0.5 and cyc / G >= 0.5 and deep / G >= 0.5 and tie / G >= 0.05


# ------------------------------------------------------------------------------------------------ options, summaries
def test_option_parsing_and_refusals(tmp_path):
    o = ta.parse_attractor_options(True, MIXED)
    assert o == dict(policies=False, weights="uniform")
    assert "uniformly over action profiles" in ta.UNIFORM_LABEL and "not the environment's reset" in ta.UNIFORM_LABEL
    assert ta.parse_attractor_options({"policies": True, "weights": None}, MIXED) == dict(policies=True, weights=None)
    o = ta.parse_attractor_options({"weights": [1] * 441}, MIXED)
    assert o["weights"] == [1.0] * 441 and json.dumps(o)
    assert ta.start_weights("uniform", 441).tolist() == [1.0 / 441.0] * 441 and ta.start_weights(None, 441) is None
    for bad in ({"tables": "final"}, {"agents": [0]}, {"policies": 1}, {"weights": "reset"}, {"weights": [1.0] * 440},
                {"weights": [-1.0] + [1.0] * 440}, {"weights": [float("nan")] * 441}, {"weights": 3}, {"weights": ["x"] * 441}):
        with pytest.raises(ValueError):
            ta.parse_attractor_options(bad, MIXED)
    with pytest.raises(ValueError):
        ta.parse_attractor_options(3, MIXED)
    with pytest.raises(ValueError, match="continuous"):
        ta.parse_attractor_options(True, CAC)
    with pytest.raises(ValueError, match="4096"):
        ta.parse_attractor_options(True, WIDE)
    # train_one refuses before it builds a batch, the launcher before it starts a shard (no GPU is touched)
    from th_rl_amd import launch, trainer
    for cfg in (dict(CAC, training={"epochs": 1, "n_games": 4, "greedy_attractors": True}),
                dict(WIDE, training={"epochs": 1, "n_games": 4, "greedy_attractors": True}),
                dict(MIXED, training={"epochs": 1, "n_games": 4, "greedy_attractors": {"tables": "converged"}})):
        (tmp_path / "c.json").write_text(json.dumps(cfg))
        with pytest.raises(ValueError):
            trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))
    (tmp_path / "l.json").write_text(json.dumps(dict(MIXED, training={"epochs": 1, "n_games": 4, "greedy_attractors": True})))
    with pytest.raises(ValueError, match="greedy_attractors is not available under th_rl_amd.launch"):
        launch.launch(str(tmp_path / "l.json"), str(tmp_path / "out"), gpus=2)
    assert not (tmp_path / "out").exists()
    # the QTable-only analysis keeps its refusal, word for word
    from th_rl_amd import attractors as at
    with pytest.raises(ValueError, match="follow-up on the mixed path's policy tables"):
        at.parse_options(True, MIXED)


def test_summary_rows_and_the_games_without_a_start():
    G = 5
    cr = np.zeros((KEEP, 2, G))
    cr[0] = [[1.0, 1.0, 2.0, 1.5, 1.0], [1.0, 1.0, 2.0, 1.5, 1.0]]         # slot 0: gains 0, 0, 1, 0.5, 0
    cr[1] = [[2.0, 0.0, 0.0, 0.0, 2.0], [2.0, 0.0, 0.0, 0.0, 2.0]]         # slot 1 of games 0 and 4: gain 1
    mass = np.zeros((KEEP, G))
    mass[0] = [0.25, 1.0, 1.0, 1.0, 0.5]
    mass[1] = [0.75, 0.0, 0.0, 0.0, 0.5]
    games = {"n_attr": np.array([2, 1, 1, 1, 2]), "mu_max": np.array([4, 8, 2, 6, 1]), "slot_x0": np.array([1, 0, 0, -1, -1]),
             "cycle_reward": cr, "start_mass": mass, "start_mass_other": np.zeros(G),
             "start_reward": np.array([[1.75, 1.0, 2.0, 1.5, 1.5]] * 2), "start": np.array([7, 3, 0, -1, -1])}
    s = ta.summarize_attractors(games, [0, 0, 0, 1, 1], 2, 2.0, 4.0)
    assert [(r["group"], r["games"], r["no_start"]) for r in s] == [(0, 3, 0), (1, 2, 2)]
    a, b = s
    assert a["single"] == 2.0 / 3.0 and a["n_attr_max"] == 2 and a["mu_max_q50"] == 4.0
    assert a["delta_train_mean"] == (1.0 + 0.0 + 1.0) / 3.0 and a["delta_largest_mean"] == 1.0 / 3.0
    assert a["delta_start_mean"] == (0.75 + 0.0 + 1.0) / 3.0 and "delta_reset_mean" not in a
    assert a["train_is_largest"] == 2.0 / 3.0 and a["train_mass_q50"] == 1.0
    assert abs(a["luck_mean"] - 0.25 / 3.0) < 1e-15
    # a group whose games have no start tuple has no training attractor to report
    assert b["delta_train_mean"] is None and b["train_mass_q50"] is None and b["luck_mean"] is None
    assert b["delta_largest_mean"] == 0.25 and b["delta_start_mean"] == 0.5 and b["train_is_largest"] == 0.0
    json.dumps(s)
    gn = ta.attractor_gains(games, 2.0, 4.0)
    assert gn["train"][:3].tolist() == [1.0, 0.0, 1.0] and np.isnan(gn["train"][3:]).all() and gn["start"][0] == 0.75
    del games["start_mass"], games["start_mass_other"], games["start_reward"]
    s = ta.summarize_attractors(games, [0, 0, 0, 1, 1], 2, 2.0, 4.0)
    assert s[0]["delta_start_mean"] is None and s[0]["train_mass_q50"] is None and s[0]["luck_mean"] is None


def test_artefacts_round_trip(tmp_path):
    rs = np.random.RandomState(4)
    G, N, T = 6, 2, 12
    r = {f: rs.randint(0, 9, G).astype(np.int32) for f in ("n_attr", "mu_max", "n_cycle_states", "rep_x0", "mu_x0", "slot_x0")}
    r.update({f: rs.randint(0, 9, (KEEP, G)).astype(np.int32) for f in ("rep", "lam", "basin")})
    r.update(cycle_reward=rs.rand(KEEP, N, G), cycle_action=rs.rand(KEEP, N, G), start=rs.randint(-1, T, G).astype(np.int32))
    ta.save_attractor_games(str(tmp_path), r)
    assert sorted(os.listdir(tmp_path)) == ["gattr_cycle.npy", "gattr_games.npy", "gattr_slots.npy", "gattr_start.npy"]
    r.update(start_mass=rs.rand(KEEP, G), start_mass_other=rs.rand(G), start_reward=rs.rand(N, G),
             tuple_rep=rs.randint(0, T, (G, T)).astype(np.uint16), tuple_mu=rs.randint(0, T, (G, T)).astype(np.uint16))
    ta.save_attractor_games(str(tmp_path), r)
    assert np.load(tmp_path / "gattr_games.npy").shape == (6, G) and np.load(tmp_path / "gattr_slots.npy").shape == (3, KEEP, G)
    assert np.load(tmp_path / "gattr_cycle.npy").shape == (2, KEEP, N, G)
    assert np.load(tmp_path / "gattr_start_mass.npy").shape == (KEEP + 1, G)
    assert np.load(tmp_path / "gattr_state.npy").shape == (2, G, T) and np.load(tmp_path / "gattr_state.npy").dtype == np.uint16
    back = ta.load_attractor_games(str(tmp_path))
    assert sorted(back) == sorted(r)
    for f in r:
        assert np.array_equal(back[f], r[f]), f


# ------------------------------------------------------------------------------------------------ the entry point
def test_args_struct_matches_header():
    from th_rl_amd import _lib
    A = _lib.TupleAttractorsArgs
    fields = [n for n, _ in A._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %d %d %d",' \
          'sizeof(thrl_tuple_attractors_args),THRL_TP_MAX_TUPLES,THRL_ATTR_KEEP,THRL_ABI_VERSION);\n'
    for f in fields:
        src += 'printf(" %%zu",offsetof(thrl_tuple_attractors_args,%s));\n' % f
    src += 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [ctypes.sizeof(A), 4096, KEEP, 4] + [getattr(A, f).offset for f in fields]
    assert len(fields) == 25 and "thrl_tuple_attractors" in _lib.SYMBOLS and _lib.ABI_VERSION == 4 and ta.KEEP == KEEP


FAKE = 4096                           # never dereferenced: validation fails before any launch
REQUIRED = ("start", "tuple_policy", "reward", "scaled", "n_attr", "mu_max", "n_cycle_states", "rep", "lam", "basin",
            "cycle_reward", "cycle_action", "rep_x0", "mu_x0", "slot_x0")
WEIGHTED = ("start_mass", "start_mass_other", "start_reward")


def _cfg(config=None, G=64):
    from th_rl_amd import _lib
    return _lib.cfg_from_config(config or CFG, G, 0)[0]


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleAttractorsArgs()
    a.n_games, a.n_tuples = 64, 441
    for f in REQUIRED:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(n_games=-3), dict(n_tuples=0), dict(n_tuples=440), dict(n_tuples=442),
                                 dict(reserved=1), dict(reserved2=1)])
def test_bad_arguments_are_bad_config(lib, bad):
    cfg = _cfg()
    assert lib.thrl_tuple_attractors(ctypes.byref(cfg), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


def test_more_than_4096_tuples_is_unsupported(lib):
    cfg = _cfg()
    assert lib.thrl_tuple_attractors(ctypes.byref(cfg), ctypes.byref(_args(n_tuples=4097)), None) == -3
    wide = _cfg({"agents": [dict(AG, actions=129), dict(AG, actions=32)], "environment": dict(ENV)})
    assert lib.thrl_tuple_attractors(ctypes.byref(wide), ctypes.byref(_args(n_tuples=4128)), None) == -3
    # 4096 itself passes the count check: the next refusal is the missing output
    big = _cfg({"agents": [dict(AG, actions=128), dict(AG, actions=32)], "environment": dict(ENV)})
    assert lib.thrl_tuple_attractors(ctypes.byref(big), ctypes.byref(_args(n_tuples=4096, slot_x0=None)), None) == -2


@pytest.mark.parametrize("null", REQUIRED + ("args", "cfg"))
def test_missing_pointers_are_null(lib, null):
    cfg = _cfg()
    a = None if null == "args" else ctypes.byref(_args(**({null: None} if null in REQUIRED else {})))
    assert lib.thrl_tuple_attractors(None if null == "cfg" else ctypes.byref(cfg), a, None) == -2


@pytest.mark.parametrize("null", WEIGHTED)
def test_missing_weighted_outputs_are_null_with_start_w(lib, null):
    cfg = _cfg()
    kw = {f: FAKE for f in WEIGHTED}
    kw[null] = None
    assert lib.thrl_tuple_attractors(ctypes.byref(cfg), ctypes.byref(_args(start_w=FAKE, **kw)), None) == -2
    assert b"start_w" in lib.thrl_last_error()
