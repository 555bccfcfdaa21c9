"""Host side of the attractor analysis (thrl_attractors, th_rl_amd.attractors): the numpy mirror against a brute-force
restatement on small hand-made and random maps, the reset starts against encode at the interval midpoints, the entry
point's validation through the library loaded without a GPU, the ctypes mirror of the args struct, option parsing, the
summary on hand-made games, the shard combination, the readers, and the condition the device tests rest on (fresh
headline games mostly have several attractors, never more than KEEP).  No GPU."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import attractors_mirror as A
import deviation_mirror as M
import equilibrium_mirror as E
from th_rl_amd import attractors as at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def fresh_tables(G, seed):
    """The headline start: 12.5 / (1 - gamma) = 250 plus a standard normal per entry (QTable.__init__)."""
    rs = np.random.RandomState(seed)
    return 250.0 + rs.standard_normal((G, 2 * 101 * 21)), rs.uniform(0.0, 10.0, G)


# ------------------------------------------------------------------------------------------------ the mirror itself
def test_mirror_on_hand_made_maps():
    # 0 -> 1 -> 2 -> 0 (a 3-cycle), 3 -> 0 and 4 -> 3 (its tail), 5 -> 5 (a fixed point), 6 -> 5
    mu, rep, lam = A.map_structure([1, 2, 0, 0, 3, 5, 5])
    assert mu.tolist() == [0, 0, 0, 1, 2, 0, 1]
    assert rep.tolist() == [0, 0, 0, 0, 0, 5, 5]
    assert lam.tolist() == [3, 3, 3, 3, 3, 1, 1]
    assert A.ordered(None, rep, mu) == [(0, 5), (5, 2)]
    # a tie in basin size is broken by the smaller rep; the rep is the smallest state ON the cycle, not of the basin
    mu, rep, lam = A.map_structure([2, 3, 3, 2, 5, 4])            # 2 <-> 3 with tails 0, 1; 4 <-> 5
    assert rep.tolist() == [2, 2, 2, 2, 4, 4] and mu.tolist() == [1, 1, 0, 0, 0, 0] and lam.tolist() == [2] * 6
    mu, rep, lam = A.map_structure([1, 0, 3, 2])
    assert A.ordered(None, rep, mu) == [(0, 2), (2, 2)]
    # identity and a single long cycle
    mu, rep, lam = A.map_structure(list(range(9)))
    assert rep.tolist() == list(range(9)) and not mu.any() and lam.tolist() == [1] * 9
    mu, rep, lam = A.map_structure([(s + 1) % 11 for s in range(11)])
    assert not rep.any() and not mu.any() and lam.tolist() == [11] * 11


def test_mirror_against_brute_force_on_random_maps():
    rs = np.random.RandomState(0)
    for S in (1, 2, 3, 5, 8, 13, 20):
        for _ in range(30):
            f = rs.randint(0, S, S)
            walk, brute = A.map_structure(f), A.brute_structure(f)
            for x, y, name in zip(walk, brute, ("mu", "rep", "lam")):
                assert x.tolist() == y.tolist(), (name, f.tolist())


def test_mirror_training_state_equals_the_deviation_mirror():
    q, s0 = fresh_tables(40, 5)
    r = A.analyse(CFG, q, s0)
    d = M.analyse(CFG, q, s0, steps=2)
    assert r["mu_x0"].tolist() == d["mu"].tolist()
    G = np.arange(40)
    assert (r["slot_x0"] >= 0).all() and r["lam"][r["slot_x0"], G].tolist() == d["lam"].tolist()
    for i in range(2):
        got = r["cycle_reward"][r["slot_x0"], i, G]
        assert np.all(np.abs(got - d["cycle_reward"][i]) <= 4 * d["lam"] * np.spacing(np.abs(d["cycle_reward"][i])))
    assert (r["basin"].sum(axis=0) == 41).all() and (r["n_attr"] == (r["rep"] >= 0).sum(axis=0)).all()


def test_fresh_headline_games_have_several_attractors():
    """What the device tests rest on: at least half of the fresh seeded headline games have two or more attractors,
    and none has more than KEEP (measured on 4,096 such games: 78 %, at most 7)."""
    q, s0 = fresh_tables(256, 11)
    r = A.analyse(CFG, q, s0, reset=at.starts(CFG))
    assert np.mean(r["n_attr"] >= 2) >= 0.5
    assert r["n_attr"].max() <= A.KEEP and (r["slot_x0"] >= 0).all()
    assert not r["reset_mass_other"].any()
    assert np.all(np.abs(r["reset_mass"].sum(axis=0) - 1.0) <= 101 * 2.0 ** -52)


# ------------------------------------------------------------------------------------------------ the reset starts
@pytest.mark.parametrize("name", ["headline", "three", "big"])
def test_starts_against_encode_at_the_midpoints(name):
    config = {"headline": CFG, "three": THREE, "big": BIG}[name]
    rows, w = at.starts(config)
    ag, a, _ = M.params(config)
    N, J = rows.shape
    assert rows.dtype == np.int32 and w.dtype == np.float64 and w.shape == (J,) and N == len(ag)
    if name == "headline":
        assert J == 101 and rows[0].tolist() == list(range(101)) and np.array_equal(rows[0], rows[1])
    if name == "big":
        assert J == 3001
    assert (w > 0).all() and abs(w.sum() - 1.0) <= 1e-15 * J
    # the intervals, rebuilt from the weights, and encode at their midpoints and just inside their ends
    edges = np.concatenate([[0.0], np.cumsum(w)]) * a
    mid = (edges[:-1] + edges[1:]) / 2
    for i, p in enumerate(ag):
        assert rows[i].tolist() == M.encode(mid, p).tolist()
        eps = 1e-9 * a
        assert rows[i].tolist() == M.encode(edges[:-1] + eps, p).tolist() == M.encode(edges[1:] - eps, p).tolist()
        assert (np.diff(rows[i]) >= 0).all()
    # consecutive intervals differ in some agent's row: the cut is the coarsest one
    assert (np.abs(np.diff(rows, axis=1)).sum(axis=0) >= 1).all()


# ------------------------------------------------------------------------------------------------ the entry point
OUTPUTS = ("n_attr", "mu_max", "n_cycle_states", "rep", "lam", "basin", "cycle_reward", "cycle_action", "rep_x0", "mu_x0",
           "slot_x0")
RESET = ("start_rows", "start_w", "reset_mass", "reset_mass_other", "reset_reward")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.AttractorsArgs()
    a.n_games = 64
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("state0", "policy") + OUTPUTS:
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _starts_args(**kw):
    return _args(**dict(dict({f: 4096 for f in RESET}, n_starts=101), **kw))


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(n_games=65), dict(flags=2), dict(flags=-1), dict(n_starts=-1),
                                 dict(n_starts=(1 << 20) + 1)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_attractors(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_starts_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", ("q", "args", "state0", "policy") + OUTPUTS + RESET)
def test_missing_pointers_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    a = None if null == "args" else ctypes.byref(_starts_args(**({} if null in ("q", "args") else {null: None})))
    assert lib.thrl_attractors(ctypes.byref(cfg), q, a, None) == -2


def test_policy_given_needs_no_q_and_no_starts_need_no_tables(lib):
    """Which pointer a THRL_ERR_NULL names: q only without the flag, the reset tables only with J > 0.  Every call here
    fails its validation, so nothing is launched."""
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    call = lambda a: lib.thrl_attractors(ctypes.byref(cfg), None, ctypes.byref(a), None)
    assert call(_args()) == -2 and b"q is NULL" in lib.thrl_last_error()                 # J = 0: NULL reset tables pass
    assert call(_args(n_starts=101)) == -2 and b"start_rows" in lib.thrl_last_error()
    assert call(_starts_args()) == -2 and b"q is NULL" in lib.thrl_last_error()
    given = _args(flags=_lib.ATTR_POLICY_GIVEN, n_attr=None)
    assert call(given) == -2 and b"q is NULL" not in lib.thrl_last_error() and b"n_attr" in lib.thrl_last_error()


def test_limits_are_unsupported_and_n_states_is_reported(lib):
    from th_rl_amd import _lib
    s = ctypes.c_int32(-1)
    for config, want in ((CFG, 41), (THREE, 87), (BIG, 41)):
        cfg, _ = _lib.cfg_from_config(config, 64, 0)
        a = _args(n_states=ctypes.pointer(s))
        assert lib.thrl_attractors(ctypes.byref(cfg), None, ctypes.byref(a), None) == -2 and s.value == want
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}       # 4,160 tuples
    cfg, _ = _lib.cfg_from_config(wide, 64, 0)
    assert lib.thrl_attractors(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED
    fine = {"agents": [dict(AG, actions=64, states=30000), dict(AG, actions=64, states=30000, action_range=[0.2, 0.4037])],
            "environment": dict(ENV)}
    cfg, _ = _lib.cfg_from_config(fine, 64, 0)
    assert lib.thrl_attractors(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED
    assert b"states" in lib.thrl_last_error()


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    fields = ("state0", "n_states", "rep", "slot_x0", "reset_reward", "state_mu")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %d %d %d %d"'
           + "".join(' " %zu"' for _ in fields) + ',sizeof(thrl_attractors_args),THRL_ATTR_KEEP,THRL_ATTR_POLICY_GIVEN,'
           'THRL_ATTR_MAX_STARTS,THRL_ABI_VERSION' + "".join(",offsetof(thrl_attractors_args,%s)" % f for f in fields)
           + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    want = [ctypes.sizeof(_lib.AttractorsArgs), _lib.ATTR_KEEP, _lib.ATTR_POLICY_GIVEN, _lib.ATTR_MAX_STARTS, 4]
    assert got == want + [getattr(_lib.AttractorsArgs, f).offset for f in fields]
    assert A.KEEP == at.KEEP == _lib.ATTR_KEEP and "thrl_attractors" in _lib.SYMBOLS


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_and_refusals(tmp_path):
    assert at.parse_options(True, CFG) == dict(policies=False)
    assert at.parse_options({"policies": True, "tables": "converged"}, CFG) == dict(policies=True, tables="converged")
    for bad in ({"tables": "best"}, {"policies": 1}, {"steps": 3}, 5, False):
        with pytest.raises(ValueError):
            at.parse_options(bad, CFG)
    with pytest.raises(ValueError, match="follow-up"):
        at.parse_options(True, MIXED)
    with pytest.raises(ValueError, match="follow-up"):
        at.check_config(MIXED)
    # train_one refuses before it builds a batch (no GPU is touched)
    from th_rl_amd import trainer
    for cfg in (dict(MIXED, training={"epochs": 1, "n_games": 4, "attractors": True}),
                dict(CFG, training={"epochs": 1, "n_games": 4, "attractors": {"tables": "converged"}}),
                dict(CFG, training={"epochs": 1, "n_games": 4, "attractors": {"rounds": 2}})):
        (tmp_path / "c.json").write_text(json.dumps(cfg))
        with pytest.raises(ValueError):
            trainer.train_one(str(tmp_path / "run"), str(tmp_path / "c.json"))


# ------------------------------------------------------------------------------------------------ summary
def _games():
    """Four games, two agents, two groups (ids 0 0 1 1); Nash = 2, Cartel = 4 in the arithmetic below."""
    K, N, G = at.KEEP, 2, 4
    g = {"n_attr": np.array([1, 3, 2, 9]), "mu_max": np.array([4, 2, 6, 1]), "n_cycle_states": np.array([1, 4, 3, 9]),
         "rep_x0": np.array([7, 3, 0, 40]), "mu_x0": np.array([0, 1, 2, 0]), "slot_x0": np.array([0, 1, 0, -1]),
         "rep": np.full((K, G), -1), "lam": np.zeros((K, G), int), "basin": np.zeros((K, G), int),
         "cycle_reward": np.zeros((K, N, G)), "cycle_action": np.zeros((K, N, G)),
         "reset_mass": np.zeros((K, G)), "reset_mass_other": np.array([0.0, 0.0, 0.0, 0.25]), "reset_reward": np.zeros((N, G))}
    g["cycle_reward"][0] = [[2.0, 1.0, 1.5, 1.0], [2.0, 1.0, 1.5, 1.0]]        # gains of slot 0: 1, 0, .5, 0
    g["cycle_reward"][1, :, 1] = [1.75, 1.75]                                    # game 1 trains into slot 1: gain .75
    g["reset_reward"][:] = [[2.0, 1.25, 1.25, 1.0], [2.0, 1.25, 1.25, 1.0]]     # reset gains: 1, .25, .25, 0
    g["reset_mass"][0] = [1.0, 0.7, 0.6, 0.5]
    g["reset_mass"][1] = [0.0, 0.3, 0.4, 0.25]
    return g, np.array([0, 0, 1, 1])


def test_summary_arithmetic():
    g, ids = _games()
    s = at.summarize(g, ids, 2, 2.0, 4.0)
    a, b = s
    assert (a["group"], a["games"], a["single"], a["n_attr_q50"], a["n_attr_max"], a["mu_max_q50"]) == (0, 2, 0.5, 2.0, 3, 3.0)
    assert a["delta_train_mean"] == (1.0 + 0.75) / 2 and a["delta_largest_mean"] == 0.5 and a["delta_reset_mean"] == 0.625
    assert a["train_is_largest"] == 0.5 and a["train_mass_q50"] == (1.0 + 0.3) / 2
    assert a["luck_mean"] == ((1.0 - 1.0) + (0.75 - 0.25)) / 2
    # game 3's training attractor is not among the kept: it is left out of the training statistics only
    assert b["games"] == 2 and b["delta_train_mean"] == 0.5 and b["train_mass_q50"] == 0.6 and b["luck_mean"] == 0.25
    assert b["delta_largest_mean"] == 0.25 and b["train_is_largest"] == 0.5 and b["n_attr_max"] == 9
    none = at.summarize({k: v for k, v in g.items() if not k.startswith("reset")}, ids, 2, 2.0, 4.0)
    assert none[0]["delta_reset_mean"] is None and none[0]["luck_mean"] is None and none[0]["train_mass_q50"] is None
    assert none[0]["delta_train_mean"] == a["delta_train_mean"]
    empty = at.summarize(g, ids, 3, 2.0, 4.0)[-1]
    assert empty["games"] == 0 and empty["single"] is None and empty["n_attr_q50"] is None and empty["delta_train_mean"] is None
    json.dumps(s + [empty])


def test_shards_combine_to_the_unsharded_run(tmp_path):
    from th_rl_amd import utils
    G = 23
    q, s0 = fresh_tables(G, 1)
    reset = at.starts(CFG)
    full = A.analyse(CFG, q, s0, reset=reset)
    cuts = ((0, 9), (9, 16), (16, G))
    parts = [A.analyse(CFG, q[lo:hi], s0[lo:hi], reset=reset) for lo, hi in cuts]
    fields = [f for f in full if f != "n_states"]
    for p in parts:
        p.pop("n_states")
    whole = at.combine(parts)
    for f in fields:
        assert np.array_equal(np.asarray(whole[f]), np.asarray(full[f])), f
    ids = np.arange(G) % 2
    nash, cartel = at.optimal(CFG)
    assert at.summarize(whole, ids, 2, nash, cartel) == at.summarize(full, ids, 2, nash, cartel)
    # the artefact round trip and the readers, sharded and not
    opt = at.parse_options(True, CFG)
    one = tmp_path / "one"
    one.mkdir()
    at.save_games(str(one), full)
    at.save_json(str(one / "attractors.json"), at.describe(opt, 41, 101, nash, cartel, at.summarize(full, ids, 2, nash, cartel)))
    (one / "config.json").write_text(json.dumps(dict(CFG, training={"n_games": G})))
    back = at.load_games(str(one))
    for f in fields:
        assert np.array_equal(back[f], np.asarray(full[f])) and back[f].dtype == np.asarray(full[f]).dtype, f
    two = tmp_path / "two"
    for r, (lo, hi) in enumerate(cuts):
        d = two / ("shard%d" % r)
        d.mkdir(parents=True)
        at.save_games(str(d), parts[r])
        at.save_json(str(d / "attractors.json"), at.describe(opt, 41, 101, nash, cartel, []))
        (d / "shard_config.json").write_text(json.dumps(dict(CFG, training={"n_games": hi - lo, "game_offset": lo})))
    a, b = utils.attractor_games(str(one)), utils.attractor_games(str(two))
    assert a.index.tolist() == b.index.tolist() == list(range(G))
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
    assert a["n_attr"].tolist() == full["n_attr"].tolist() and a["basin_0"].tolist() == full["basin"][0].tolist()
    assert np.array_equal(a["delta_reset"].to_numpy(), at.profit_gain(full["reset_reward"], nash, cartel))
    k = int(full["n_attr"][0])
    assert np.isfinite(a["delta_%d" % (k - 1)][0]) and (k == at.KEEP or np.isnan(a["delta_%d" % k][0]))
    df = utils.attractor_summary(str(one))
    assert len(df) == 2 and df["n_states"].tolist() == [41] * 2 and df["n_starts"].tolist() == [101] * 2
    with pytest.raises(KeyError):
        utils.attractor_games(str(tmp_path))
    # launch.merge_analysis: the shards' files merged are the whole run's
    from th_rl_amd import launch
    cfg = dict(CFG, training={"n_games": G, "attractors": True, "groups": ids.tolist(), "n_groups": 2})
    launch.merge_analysis("attractors", cfg, str(two), 3)
    merged = at.load_games(str(two))
    for f in fields:
        assert np.array_equal(merged[f], np.asarray(full[f])), f
    assert json.load(open(two / "attractors.json"))["summary"] == json.load(open(one / "attractors.json"))["summary"]
