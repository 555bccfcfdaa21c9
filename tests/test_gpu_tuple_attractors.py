"""The attractor analysis in tuple form on the device (thrl_tuple_attractors, MixedGameBatch.greedy_attractors,
training.greedy_attractors): bit-equal to the numpy mirror (tests/tuple_attractors_mirror.py) on random maps, on
hand-built maps at the edges of the tuple count and of the launch shape, and on strategies extracted from batches with
networks; consistent with thrl_tuple_walk and, on an all-QTable batch, with thrl_attractors, with no mirror in between;
the trainer's artefacts.

The random maps carry the coverage (tests/test_tuple_attractors_host.py asserts on the mirror that they have several
attractors, cycles longer than 1, long tails and tied basins); the share of extracted games with n_attr >= 2 is printed,
not asserted."""
import json

import numpy as np
import pytest

import tuple_attractors_mirror as AM

pytestmark = pytest.mark.gpu

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
BIG = {"agents": [dict(AG, actions=128), dict(RF, actions=32)], "environment": dict(ENV)}          # T = 4096 exactly
WIDE = {"agents": [dict(AG, actions=129), dict(RF, actions=32)], "environment": dict(ENV)}         # 4128 tuples
CONFIGS = {"MIXED": (MIXED, 441), "AC": (AC, 105), "NN2": (NN2, 672), "THREE": (THREE, 385)}
G = 203                                                                 # no multiple of a wave or of a block
KEEP = 8
GAME = ("n_attr", "mu_max", "n_cycle_states", "rep_x0", "mu_x0", "slot_x0")
SLOT = ("rep", "lam", "basin", "cycle_reward", "cycle_action")
START = ("start_mass", "start_mass_other", "start_reward")
TUPLE = ("tuple_rep", "tuple_mu")
ALL = GAME + SLOT + START + TUPLE


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _kinked_weights(rs, n_games, A, P, lo, hi):
    """w1 ~ U(-1, 1), b1 = -w1 * c with c ~ U(min price, max price) per hidden unit, W2, b2 ~ U(-1, 1); a value head
    (ActorCritic) keeps zeros."""
    w = np.zeros((n_games, P), np.float32)
    w1 = rs.uniform(-1, 1, (n_games, 256))
    c = rs.uniform(lo, hi, (n_games, 256))
    w[:, :256], w[:, 256:512] = w1, -w1 * c
    n2 = A * 256 + A
    w[:, 512:512 + n2] = rs.uniform(-1, 1, (n_games, n2))
    return w


def _mixed(config, n_games=G, dtype="float32", seed=3, weights_seed=1):
    from th_rl_amd import tuple_play as tp
    from th_rl_amd.mixed import MixedGameBatch
    mb = MixedGameBatch(config, n_games=n_games, dtype=dtype, seed=seed).init_tables()
    price = tp.tables(config)["price"]
    rs = np.random.RandomState(weights_seed)
    for i, rb in mb.nn.items():
        rb.set_params(_kinked_weights(rs, n_games, rb.A, rb.P, price.min(), price.max()))
    return mb


def _starts(T, n_games, seed):
    """Random start tuples with -1 (and one T) mixed in."""
    rs = np.random.RandomState(seed)
    start = rs.randint(0, T, size=n_games).astype(np.int32)
    if n_games > 8:
        start[rs.choice(n_games, n_games // 8, replace=False)] = -1
        start[0], start[5] = 0, T
    return start


def _device(mb, pol):
    """A uint16 strategy array [G, N, T] as the device tensor the runners take."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(pol).view(np.int16)).to(mb.state.device)


def _policy_of(F, second):
    """uint16 [2, T]: the two agents' entries that send tuple t to tuple F[t]; `second` = agent 1's action count."""
    F = np.asarray(F)
    return np.stack([F // second, F % second]).astype(np.uint16)


def _check(mb, tabs, pol, start, w, what):
    out = mb.greedy_attractors(start=start, weights=w, policies=True, tuple_policy=_device(mb, pol))
    ref = AM.analyse(tabs, pol, start, start_w=w, policies=True)
    for f in ALL:
        _bits_equal(out[f], ref[f], "%s %s" % (what, f))
    assert out["n_states"] == tabs["T"] and np.array_equal(out["start"], start)
    return out, ref


_BATCH = {}


def _batch(name):
    if name not in _BATCH:
        _BATCH[name] = _mixed(CONFIGS[name][0])
    return _BATCH[name]


# ------------------------------------------------------------------------------------------------ random maps
@pytest.mark.parametrize("name,actions,seed", [("MIXED", (21, 21), 17), ("AC", (21, 5), 18), ("THREE", (7, 11, 5), 19)])
def test_random_maps_equal_mirror(name, actions, seed):
    from test_tuple_attractors_host import random_policy
    from th_rl_amd import tuple_play as tp
    config, T = CONFIGS[name]
    tabs = tp.tables(config)
    assert [int(x) for x in tabs["n_actions"]] == list(actions) and T == int(np.prod(actions))
    pol = random_policy(actions, seed, G)
    rs = np.random.RandomState(seed + 100)
    for i, A in enumerate(actions):                                      # entries at or above the action count: clamped
        hit = rs.rand(G, T) < 0.02
        pol[:, i][hit] += np.uint16(A)
    pol[3, 0, :] = 65535
    start = _starts(T, G, seed + 1)
    w = rs.uniform(0.0, 1.0, T)
    out, ref = _check(_batch(name), tabs, pol, start, w, name)
    none = (start < 0) | (start >= T)
    assert none.sum() >= G // 8 and (out["rep_x0"][none] == -1).all() and (out["mu_x0"][none] == -1).all() \
        and (out["slot_x0"][none] == -1).all() and (out["rep_x0"][~none] >= 0).all()
    print("%s: n_attr >= 2 %.2f, more than KEEP %.2f, mu_max up to %d, start_mass_other > 0 %.2f"
          % (name, np.mean(ref["n_attr"] >= 2), np.mean(ref["n_attr"] > KEEP), ref["mu_max"].max(),
             np.mean(ref["start_mass_other"] > 0)))
    # no start weights: the same integers and cycle means, no start_* fields
    bare = _batch(name).greedy_attractors(start=start, weights=None, tuple_policy=_device(_batch(name), pol))
    assert not any(f in bare for f in START + TUPLE)
    for f in GAME + SLOT:
        _bits_equal(bare[f], out[f], f)
    # uniform weights are 1 / T per tuple
    uni = _batch(name).greedy_attractors(start=start, tuple_policy=_device(_batch(name), pol))
    ref_u = AM.analyse(tabs, pol, start, start_w=np.full(T, 1.0 / T))
    for f in START:
        _bits_equal(uni[f], ref_u[f], "uniform " + f)


# ------------------------------------------------------------------------------------------------ edges
def test_four_tuples():
    from th_rl_amd import tuple_play as tp
    maps = [[0, 1, 2, 3], [1, 2, 3, 0], [0, 0, 1, 2], [1, 0, 3, 2], [0, 3, 3, 3], [3, 3, 3, 3]]
    pol = np.stack([_policy_of(F, 2) for F in maps])
    gb = _mixed(FOUR, n_games=len(maps))
    tabs = tp.tables(FOUR)
    start = np.array([2, 3, 3, 2, 0, -1], np.int32)
    out, _ = _check(gb, tabs, pol, start, np.array([0.1, 0.2, 0.3, 0.4]), "T=4")
    assert out["n_attr"].tolist() == [4, 1, 1, 2, 2, 1] and out["mu_max"].tolist() == [0, 0, 3, 0, 1, 1]
    assert out["rep"][:2, 3].tolist() == [0, 2] and out["rep"][:2, 4].tolist() == [3, 0]
    one = _mixed(FOUR, n_games=1)
    _check(one, tabs, pol[3:4], start[3:4], np.array([0.1, 0.2, 0.3, 0.4]), "T=4 G=1")


def test_4096_tuples_exactly():
    from th_rl_amd import tuple_play as tp
    T = 4096
    t = np.arange(T)
    rs = np.random.RandomState(31)
    maps = [(t + 1) % T, np.maximum(t - 1, 0), t, rs.randint(0, T, T), rs.randint(0, T, T)]
    pol = np.stack([_policy_of(F, 32) for F in maps])
    mb = _mixed(BIG, n_games=len(maps), seed=23, weights_seed=9)
    tabs = tp.tables(BIG)
    assert tabs["T"] == T
    start = np.array([4095, 4095, 1234, -1, 4096], np.int32)
    out, _ = _check(mb, tabs, pol, start, rs.uniform(0.0, 1.0, T), "T=4096")
    assert out["n_attr"][:3].tolist() == [1, 1, T] and out["mu_max"][:3].tolist() == [0, T - 1, 0]
    assert out["lam"][0, :3].tolist() == [T, 1, 1] and out["n_cycle_states"][:3].tolist() == [T, 1, T]
    assert out["mu_x0"][:3].tolist() == [0, T - 1, 0] and out["slot_x0"][:3].tolist() == [0, 0, -1]
    assert out["rep"][:, 2].tolist() == list(range(KEEP)) and out["start_mass_other"][2] > 0
    # one game alone, and the strategies the batch itself holds
    single = _mixed(BIG, n_games=1, seed=23, weights_seed=9)
    _check(single, tabs, pol[1:2], start[1:2], rs.uniform(0.0, 1.0, T), "T=4096 G=1")
    given = tp.extract(mb)
    _check(mb, tabs, given.cpu().numpy().view(np.uint16), start, np.full(T, 1.0 / T), "T=4096 extracted")


def test_halves_equal_the_whole():
    from test_tuple_attractors_host import random_policy
    from th_rl_amd import tuple_play as tp
    tabs = tp.tables(MIXED)
    pol = random_policy((21, 21), 23, G)
    start = _starts(441, G, 24)
    w = np.random.RandomState(25).uniform(0.0, 1.0, 441)
    mb = _batch("MIXED")
    whole = mb.greedy_attractors(start=start, weights=w, policies=True, tuple_policy=_device(mb, pol))
    for lo, hi in ((0, 101), (101, 203), (7, 8)):
        part = _mixed(MIXED, n_games=hi - lo)
        sub = part.greedy_attractors(start=start[lo:hi], weights=w, policies=True, tuple_policy=_device(part, pol[lo:hi]))
        for f in GAME + SLOT + START:
            _bits_equal(sub[f], whole[f][..., lo:hi], f)
        for f in TUPLE:
            _bits_equal(sub[f], whole[f][lo:hi], f)


# ------------------------------------------------------------------------------------------------ extracted strategies
_CACHE = {}


def _case(name, episodes):
    """(batch, tables, strategies as numpy, as the device tensor, start tuples) of one config, built once."""
    from th_rl_amd import tuple_play as tp
    key = (name, episodes)
    if key not in _CACHE:
        config, T = CONFIGS[name]
        mb = _mixed(config, seed=5 + episodes, weights_seed=2 + episodes)
        if episodes:
            mb.run(episodes, per_game_logs=False)
        given = tp.extract(mb)
        pol = given.cpu().numpy().view(np.uint16)
        assert pol.shape == (G, len(config["agents"]), T)
        _CACHE[key] = (mb, tp.tables(config), pol, given, _starts(T, G, 17 + episodes))
    return _CACHE[key]


@pytest.mark.parametrize("episodes", [0, 20])
@pytest.mark.parametrize("name", ["MIXED", "AC", "NN2", "THREE"])
def test_extracted_strategies_equal_mirror(name, episodes):
    import torch
    mb, tabs, pol, given, start = _case(name, episodes)
    before = [mb.q.clone(), mb.counter.clone(), mb.state.clone(), given.clone()] + [rb.params.clone() for rb in mb.nn.values()]
    w = np.random.RandomState(40 + episodes).uniform(0.0, 1.0, tabs["T"])
    out = mb.greedy_attractors(start=start, weights=w, policies=True, tuple_policy=given)
    ref = AM.analyse(tabs, pol, start, start_w=w, policies=True)
    for f in ALL:
        _bits_equal(out[f], ref[f], "%s %s" % (name, f))
    for a, b in zip(before, [mb.q, mb.counter, mb.state, given] + [rb.params for rb in mb.nn.values()]):
        assert torch.equal(a, b)                                         # nothing of the batch is written
    print("%s after %d episodes: games with n_attr >= 2: %.3f, largest n_attr %d, mu_max up to %d"
          % (name, episodes, np.mean(ref["n_attr"] >= 2), ref["n_attr"].max(), ref["mu_max"].max()))


# ------------------------------------------------------------------------------------------------ against the device
@pytest.mark.parametrize("name", ["MIXED", "THREE"])
def test_against_the_tuple_walk(name):
    from th_rl_amd import tuple_play as tp
    mb, tabs, pol, given, start = _case(name, 20)
    T = tabs["T"]
    out = mb.greedy_attractors(start=start, policies=True, tuple_policy=given)
    # (a) a walk started at a kept slot's rep is on the cycle and reports the slot's numbers
    for k in range(KEEP):
        rep = out["rep"][k]
        walk = tp.run(mb, start=rep, tuple_policy=given, tabs=tabs)
        kept = rep >= 0
        assert kept.any() or k > 0
        assert not walk["mu"][kept].any() and (walk["mu"][~kept] == -1).all()
        _bits_equal(walk["lam"][kept], out["lam"][k][kept], "lam of slot %d" % k)
        _bits_equal(walk["cycle_start"][kept], rep[kept], "cycle_start of slot %d" % k)
        for f in ("cycle_reward", "cycle_action"):
            _bits_equal(walk[f][:, kept], out[f][k][:, kept], "%s of slot %d" % (f, k))
    # (b) the walk from the training tuple ends in rep_x0's attractor after mu_x0 steps
    walk = tp.run(mb, start=start, horizon=T + 1, tuple_policy=given, tabs=tabs)
    ok = (start >= 0) & (start < T)
    assert ok.sum() >= G // 2
    _bits_equal(walk["mu"][ok], out["mu_x0"][ok], "mu_x0")
    lam_of = np.array([np.sum((out["tuple_rep"][g] == out["rep_x0"][g]) & (out["tuple_mu"][g] == 0)) for g in range(G)])
    _bits_equal(walk["lam"][ok], lam_of[ok], "lam of rep_x0's attractor")
    gi = np.flatnonzero(ok)
    assert np.array_equal(out["tuple_rep"][gi, walk["cycle_start"][gi]], out["rep_x0"][gi])
    kept = ok & (out["slot_x0"] >= 0)
    assert np.array_equal(out["lam"][out["slot_x0"][kept], np.flatnonzero(kept)], walk["lam"][kept])
    assert (out["rep_x0"][~ok] == -1).all() and (walk["mu"][~ok] == -1).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_all_qtable_batch_against_the_row_kernel(dtype):
    from th_rl_amd import tuple_play as tp
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(TWO, n_games=G, dtype=dtype, seed=11).init_tables()
    gb.run(40, logs=False)
    tabs = tp.tables(TWO)
    t = gb.greedy_attractors(weights=None)
    r = gb.attractors(reset=False)
    _bits_equal(t["n_attr"], r["n_attr"], "n_attr")
    _bits_equal(t["n_cycle_states"], r["n_cycle_states"], "n_cycle_states")
    assert (t["start"] >= 0).all() and (t["rep_x0"] >= 0).all()
    rmax = np.abs(tabs["reward"]).max(axis=1)
    few = np.flatnonzero(r["n_attr"] <= KEEP)
    assert few.size >= G // 2
    for g in few:
        n = int(r["n_attr"][g])
        assert sorted(t["lam"][:n, g].tolist()) == sorted(r["lam"][:n, g].tolist()), g
        free = list(range(n))
        for k in range(n):                                               # match by lam and mean: the two calls add the
            lam = int(t["lam"][k, g])                                    # same terms from different rotations of the cycle
            bound = (lam + 1) * 2.0 ** -52 * rmax
            hit = [j for j in free if r["lam"][j, g] == lam
                   and (np.abs(r["cycle_reward"][j, :, g] - t["cycle_reward"][k, :, g]) <= bound).all()]
            assert hit, (g, k, lam, t["cycle_reward"][k, :, g], r["cycle_reward"][:n, :, g])
            free.remove(hit[0])
    print("%s: n_attr >= 2 %.2f, n_attr <= KEEP %.2f, lam > 1 somewhere %.2f"
          % (dtype, np.mean(r["n_attr"] >= 2), few.size / float(G), np.mean(r["lam"].max(axis=0) > 1)))


# ------------------------------------------------------------------------------------------------ refusals, trainer
def test_refusals_and_the_old_methods_still_raise():
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.mixed import MixedGameBatch
    wide = MixedGameBatch(WIDE, n_games=4).init_tables()
    cac = MixedGameBatch(CAC, n_games=4).init_tables()
    with pytest.raises(ValueError, match="4096"):
        wide.greedy_attractors(start=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="continuous"):
        cac.greedy_attractors(start=np.zeros(4, np.int32))
    mb = _mixed(MIXED, n_games=8)
    with pytest.raises(ThrlError, match="attractor analysis runs on QTable agents only.*follow-up on the mixed path's policy tables"):
        mb.attractors()
    with pytest.raises(ValueError):
        mb.greedy_attractors(weights=np.ones(440))
    out = mb.greedy_attractors()
    assert (out["n_attr"] >= 1).all() and out["start_mass"].shape == (KEEP, 8)


def test_train_one_artefacts(tmp_path):
    from th_rl_amd import launch, trainer, tuple_analysis as ta, utils
    from th_rl_amd.mixed import MixedGameBatch
    n = 64
    base = dict(MIXED, environment=dict(ENV, max_steps=20))
    cfg = dict(base, training={"epochs": 20, "print_freq": 500, "seed": 19, "n_games": n, "groups": [0] * 40 + [1] * 24,
                               "greedy_cycles": True, "greedy_attractors": {"policies": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "greedy_attractors.json"))
    assert desc["n_states"] == 441 and desc["keep"] == KEEP and desc["options"] == {"policies": True, "weights": "uniform"}
    assert "uniformly over action profiles" in desc["start_weights"]
    assert (exp / "greedy_cycles.json").exists()
    assert np.load(exp / "gattr_games.npy").shape == (6, n) and np.load(exp / "gattr_slots.npy").shape == (3, KEEP, n)
    assert np.load(exp / "gattr_cycle.npy").shape == (2, KEEP, 2, n) and np.load(exp / "gattr_start.npy").shape == (n,)
    assert np.load(exp / "gattr_start_mass.npy").shape == (KEEP + 1, n) and np.load(exp / "gattr_start_reward.npy").shape == (2, n)
    assert np.load(exp / "gattr_state.npy").shape == (2, n, 441)
    summ = utils.greedy_attractor_summary(str(exp))
    games = utils.greedy_attractor_games(str(exp))
    assert len(summ) == len(desc["summary"]) == 2 and summ["games"].tolist() == [40, 24] and summ["n_states"][0] == 441
    assert summ["no_start"].sum() == int((games["start"] < 0).sum()) and (summ["no_start"] <= summ["games"]).all()
    assert "delta_start_mean" in summ and "delta_reset_mean" not in summ
    # equal to the batch method on the saved batch
    mb = MixedGameBatch(base, n_games=n).load(str(exp / "batch.pt"))
    direct = mb.greedy_attractors(policies=True)
    saved = ta.load_attractor_games(str(exp))
    for f in ALL + ("start",):
        _bits_equal(saved[f], direct[f], f)
    assert games.index.tolist() == list(range(n))
    for f in GAME + ("start",):
        assert games[f].tolist() == direct[f].tolist(), f
    for k in range(KEEP):
        assert games["rep_%d" % k].tolist() == direct["rep"][k].tolist()
        _bits_equal(games["mass_%d" % k].to_numpy(), direct["start_mass"][k], "mass")
    _bits_equal(games["mass_other"].to_numpy(), direct["start_mass_other"], "mass_other")
    # the walk of greedy_cycles ends in the training attractor
    cyc = np.load(exp / "gcyc_cycle.npy")[0]
    has = direct["start"] >= 0
    assert np.array_equal(cyc[0][has], direct["mu_x0"][has])
    assert np.array_equal(direct["tuple_rep"][np.flatnonzero(has), cyc[2][has]], direct["rep_x0"][has])
    with pytest.raises(KeyError):
        utils.greedy_attractor_games(str(tmp_path))
    with pytest.raises(ValueError, match="greedy_attractors is not available under th_rl_amd.launch"):
        launch.check_launch_config(dict(base, training={"n_games": n, "greedy_attractors": {"policies": True}}))
    with pytest.raises(ValueError, match="is not available under th_rl_amd.launch"):
        launch.check_launch_config(cfg)                                  # beside greedy_cycles: refused all the same
    (tmp_path / "cac.json").write_text(json.dumps(dict(CAC, training={"epochs": 1, "n_games": 4, "greedy_attractors": True})))
    with pytest.raises(ValueError, match="continuous"):
        trainer.train_one(str(tmp_path / "cac"), str(tmp_path / "cac.json"))
