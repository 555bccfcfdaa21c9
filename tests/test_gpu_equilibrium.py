"""Equilibrium check on the device (thrl_equilibrium, GameBatch.equilibrium, training.equilibrium): every output
bit-equal to the numpy mirror (tests/equilibrium_mirror.py) on fresh and trained tables, f32 and f64, individual grids
(S = 87: several states per lane, on f32 tables and on f64 ones), 64 x 64 action tuples (the reward LUT in global memory), the 3,000-state config, a gamma sweep, an agents mask, given and default start
prices, a game count that is no multiple of anything; the known answers through set_tables; mu / lam against the
deviation analysis; and the invariances (learning state untouched, halves, MixedGameBatch, the trainer's artefacts at
convergence, a sharded launch, error codes)."""
import ctypes
import json

import numpy as np
import pytest

import deviation_mirror as M
import equilibrium_mirror as E

pytestmark = pytest.mark.gpu

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
SYM = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
WIDE2 = {"agents": [dict(AG, actions=64, states=200), dict(AG, actions=64, states=200, gamma=0.9)], "environment": dict(ENV)}
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}
GAME_FIELDS = ("mu", "lam", "iters", "n_diff_all", "n_diff_on", "loss_all", "loss_on", "loss_all_mean", "loss_on_mean",
               "v_on")
STATE_FIELDS = ("br_policy", "v_opt", "v_pi")


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _check(gb, config, state0=None, gamma=None, agents=None):
    out = gb.equilibrium(agents=agents, state0=state0, policies=True)
    s0 = gb.states_numpy() if state0 is None else state0
    ref = E.analyse(config, gb.tables_numpy(), s0, agents=agents, gamma=gamma)
    assert out["n_states"] == ref["n_states"]
    for f in GAME_FIELDS + STATE_FIELDS:
        _bits_equal(out[f], ref[f], f)
    return out


def _batch(config, G, dtype="float32", seed=3, episodes=0, sweep=None):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, seed=seed, sweep=sweep).init_tables()
    if episodes:
        gb.run(episodes, logs=False)
    return gb


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("episodes", [0, 300])
def test_headline_matches_mirror(dtype, episodes):
    gb = _batch(TWO, 203, dtype, seed=11, episodes=episodes)           # 203: no multiple of a wave or a block
    out = _check(gb, TWO)
    assert out["n_states"] == 41
    assert out["iters"].min() >= 0 and out["iters"].max() >= 1          # someone's strategy is no best response
    assert (out["loss_all"] >= out["loss_on"]).all() and (out["n_diff_all"] >= out["n_diff_on"]).all()
    _check(gb, TWO, state0=np.random.RandomState(2).uniform(0, 10, gb.G))


def test_three_agents_individual_grids_several_states_per_lane():
    gb = _batch(THREE, 96, seed=5, episodes=50)
    out = _check(gb, THREE)
    assert out["n_states"] == 87 and out["n_states"] > 64               # the LDS evaluation path
    _check(gb, THREE, state0=np.linspace(0.0, 10.0, 96), agents=[1])


def _random_batch(config, G, dtype, seed):
    """Random tables through set_tables, no training: the mirror reads the same numbers on any machine."""
    from oracle import oracle as O
    from th_rl_amd.batched import GameBatch
    cfg, _ = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    rs = np.random.RandomState(seed)
    q = rs.normal(0.0, 1.0, (G, O.table_stride(cfg))).astype(dtype)
    return GameBatch(config, n_games=G, dtype=dtype, seed=seed).set_tables(q, rs.uniform(0, 10, G))


def test_lds_evaluation_path_on_float64_tables():
    gb = _random_batch(THREE, 96, "float64", seed=21)                   # k_equilibrium<double, S > 64, reward LUT in LDS>
    out = _check(gb, THREE)
    assert out["n_states"] == 87 and out["iters"].min() >= 0 and out["iters"].max() >= 2


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_reward_lut_in_global_memory_with_the_lds_evaluation_path(dtype):
    # 64 x 64 = 4,096 tuples: the reward LUT alone is the 64 KiB budget, so it stays in global memory; S = 81 > 64
    gb = _random_batch(WIDE2, 12, dtype, seed=22)
    out = _check(gb, WIDE2)
    assert out["n_states"] == 81 and out["iters"].min() >= 0 and out["iters"].max() >= 2


def test_3000_state_config_matches_mirror():
    gb = _batch(BIG, 64, seed=6, episodes=20)
    out = _check(gb, BIG)
    assert out["n_states"] == 41
    _check(gb, BIG, state0=np.linspace(0.5, 9.5, 64))


def test_gamma_sweep_solves_with_the_games_gamma():
    G = 128
    gam = np.array([[0.35, 0.9, 0.95, 0.0, 0.99][g % 5] for g in range(G)])
    gb = _batch(TWO, G, seed=8, episodes=100, sweep={"gamma": gam})
    _check(gb, TWO, gamma=np.stack([gam, gam]))


def test_agents_mask_leaves_the_others_alone():
    gb = _batch(TWO, 70, seed=9, episodes=30)
    both = gb.equilibrium(policies=True)
    one = _check(gb, TWO, agents=[1])
    assert one["agents"] == [1]
    for f in GAME_FIELDS[2:] + STATE_FIELDS:
        _bits_equal(one[f][1], both[f][1], f)
        assert not np.asarray(one[f][0]).any(), f                       # never written: the zeros they were made with
    assert not one["br_on"][0].any() and np.array_equal(one["nash"], one["br_on"][1])


def test_cycle_equals_the_deviation_analysis():
    for cfg, G, ep in ((TWO, 150, 0), (TWO, 150, 200), (THREE, 64, 30)):
        gb = _batch(cfg, G, seed=21, episodes=ep)
        s0 = np.random.RandomState(4).uniform(0, 10, G)
        for st in (None, s0):
            e, d = gb.equilibrium(state0=st), gb.deviation(state0=st, steps=2)
            _bits_equal(e["mu"], d["mu"], "mu")
            _bits_equal(e["lam"], d["lam"], "lam")


# ------------------------------------------------------------------------------------------------ known answers
def _known(config, strategies, state0, dtype="float64"):
    from th_rl_amd.batched import GameBatch
    G = len(state0)
    gb = GameBatch(config, n_games=G, dtype=dtype).set_tables(E.strategy_tables(config, strategies, G), state0)
    return gb.equilibrium(policies=True)


def test_known_static_nash_pair_is_an_equilibrium():
    pairs = E.static_best_responses(E.plan(SYM))
    assert pairs == [(13, 14), (14, 13)]
    for dtype in ("float32", "float64"):
        for a0, a1 in pairs:
            o = _known(SYM, [a0, a1], [3.0, 7.5], dtype)
            assert o["iters"].tolist() == [[0, 0]] * 2 and not o["n_diff_all"].any()
            for f in ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean"):
                assert (o[f] == 0.0).all(), f
            _bits_equal(o["v_opt"], o["v_pi"], "v")
            assert o["nash"].all() and o["perfect"].all()


def test_known_cartel_without_punishment_is_none():
    pl = E.plan(SYM)
    o = _known(SYM, [5, 5], [3.0])
    assert o["n_states"] == 41 and o["n_diff_all"][:, 0].tolist() == [41, 41] and o["n_diff_on"][:, 0].tolist() == [1, 1]
    R = pl["rew"][0].reshape(21, 21)
    want = 1.0 - R[5, 5] / R[:, 5].max()
    assert abs(want - 0.110953) < 1e-6
    assert abs(o["loss_all"][0, 0] - want) <= 4 * 2 * E.doublings(0.95) * 2.0 ** -53 * want
    assert not o["nash"].any() and not o["perfect"].any()


def test_known_grim_trigger():
    pl = E.plan(SYM)
    row = int(M.encode(M.env_step([M.scale(5, pl["ag"][0]), M.scale(5, pl["ag"][1])], 10.0, 1.0)[0], pl["ag"][0]))
    assert row == 50
    s0, s1 = np.full(101, 13), np.full(101, 14)
    s0[row] = s1[row] = 5
    start = [5.0]                                   # row 50: the cartel state
    patient = {"agents": [dict(AG, gamma=0.95), dict(AG, gamma=0.95)], "environment": dict(ENV)}
    o = _known(patient, [s0, s1], start)
    assert (o["mu"][0], o["lam"][0]) == (0, 1) and o["nash"].all() and o["perfect"].all()
    assert o["iters"][:, 0].tolist() == [0, 0]
    hasty = {"agents": [dict(AG, gamma=0.3), dict(AG, gamma=0.3)], "environment": dict(ENV)}
    o = _known(hasty, [s0, s1], start)
    assert o["n_diff_on"][:, 0].tolist() == [1, 1] and o["n_diff_all"][:, 0].tolist() == [1, 1]   # only at the cartel state
    assert (o["loss_on"] > 0).all() and abs(o["loss_on"][0, 0] - 0.0465) < 1e-3
    assert not o["nash"].any()
    ref = E.analyse(hasty, E.strategy_tables(hasty, [s0, s1], 1), start)
    for f in GAME_FIELDS + STATE_FIELDS:
        _bits_equal(o[f], ref[f], f)


# ------------------------------------------------------------------------------------------------ invariances
def test_learning_state_untouched_and_halves_equal_full():
    from th_rl_amd.batched import GameBatch
    G = 180
    gb = _batch(TWO, G, seed=12, episodes=40)
    before = (gb.tables_numpy().copy(), gb.counters_numpy().copy(), gb.states_numpy().copy(), list(gb.eps), gb.episode)
    full = gb.equilibrium(policies=True)
    after = (gb.tables_numpy(), gb.counters_numpy(), gb.states_numpy(), list(gb.eps), gb.episode)
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    q, s = before[0], before[2]
    for lo, hi in ((0, 77), (77, G)):
        h = GameBatch(TWO, n_games=hi - lo, seed=12, game_offset=lo).set_tables(q[lo:hi], s[lo:hi])
        part = h.equilibrium(policies=True)
        for f in GAME_FIELDS:
            _bits_equal(part[f], full[f][..., lo:hi], f)
        for f in STATE_FIELDS:
            _bits_equal(part[f], full[f][:, lo:hi], f)


def test_mixed_batch_equals_game_batch():
    from th_rl_amd.mixed import MixedGameBatch
    from th_rl_amd._lib import ThrlError
    G = 96
    for dtype in ("float32", "float64"):
        gb = _batch(TWO, G, dtype, seed=14, episodes=30)
        mb = MixedGameBatch(TWO, n_games=G, dtype=dtype).set_tables(gb.tables_numpy(), gb.states_numpy())
        a, b = gb.equilibrium(policies=True), mb.equilibrium(policies=True)
        for f in GAME_FIELDS + STATE_FIELDS:
            _bits_equal(b[f], a[f], f)
    mx = MixedGameBatch(MIXED, n_games=8).init_tables()
    with pytest.raises(ThrlError, match="follow-up"):
        mx.equilibrium()


def test_error_codes_never_fault():
    from th_rl_amd import _lib
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.batched import GameBatch
    gb = _batch(TWO, 16, seed=1)
    with pytest.raises(ThrlError, match="subset"):
        gb.equilibrium(agents=[2])
    # more than 4,096 action tuples / a gamma of 1
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}
    wb = GameBatch(wide, n_games=4, kernel="generic").init_tables()
    with pytest.raises(ThrlError) as e:
        wb.equilibrium()
    assert e.value.code == _lib.ERR_UNSUPPORTED
    one = {"agents": [dict(AG, gamma=1.0), dict(AG)], "environment": dict(ENV)}
    ob = GameBatch(one, n_games=4).init_tables()
    with pytest.raises(ThrlError) as e:
        ob.equilibrium()
    assert e.value.code == -1
    assert ob.equilibrium(agents=[1])["iters"].shape == (2, 4)         # the other agent's gamma is fine
    # a missing required output
    a = _lib.EquilibriumArgs()
    a.n_games, a.agents = 16, 3
    assert gb.L.thrl_equilibrium(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(a), None) == -2
    # a per-game gamma outside [0, 1) is refused by the batch before the call
    sw = _batch(TWO, 8, seed=2, sweep={"gamma": np.array([0.5] * 7 + [1.0])})
    with pytest.raises(ThrlError, match="sweep gamma"):
        sw.equilibrium()


# ------------------------------------------------------------------------------------------------ trainer, launch
def test_train_one_equilibrium_artefacts_at_convergence(tmp_path):
    from th_rl_amd import trainer, utils, equilibrium as eq
    G = 256
    sw = {"gamma": [[0.5, 0.9, 0.95, 0.35][g % 4] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 60, "print_freq": 500, "seed": 21, "n_games": G, "sweep": sw,
                              "convergence": {"window": 10, "every": 5, "snapshot": True},
                              "deviation": {"steps": 6, "tables": "converged"},
                              "equilibrium": {"tables": "converged", "policies": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "equilibrium.json"))
    assert desc["options"]["agents"] == [0, 1] and desc["options"]["tables"] == "converged" and desc["n_states"] == 41
    assert [(r["group"], r["agent"]) for r in desc["summary"]] == [(k, a) for k in range(4) for a in (0, 1, None)]
    games = eq.load_games(str(exp))
    assert games["br_policy"].shape == (2, G, 41) and games["br_policy"].dtype == np.uint16
    # the artefacts are the mirror's on each converged game's snapshot and the final tables of the others
    import torch
    from th_rl_amd.batched import GameBatch
    ca = np.load(exp / "conv_episode.npy")
    sd = torch.load(exp / "convergence.pt", weights_only=True)
    gb = GameBatch(TWO, n_games=G, sweep=sw).load(str(exp / "batch.pt"))
    m = torch.from_numpy(ca >= 0)
    q = torch.where(m[:, None], sd["q_conv"], gb.q.cpu()).numpy()
    s0 = torch.where(m, sd["state_conv"], gb.state.cpu()).numpy()
    gam = np.asarray(sw["gamma"])
    ref = E.analyse(TWO, q, s0, gamma=np.stack([gam, gam]))
    for f in GAME_FIELDS + STATE_FIELDS:
        _bits_equal(games[f], ref[f], f)
    # mu / lam are the deviation analysis' on the same tables
    dv = utils.deviation_games(str(exp), 0)
    e0 = utils.equilibrium_games(str(exp), 0)
    assert e0["mu"].tolist() == dv["mu"].tolist() and e0["lam"].tolist() == dv["lam"].tolist()
    df = utils.equilibrium_summary(str(exp))
    assert len(df) == 12 and df["games"].tolist() == [G // 4] * 12
    assert all(r["collusive"] is not None for r in desc["summary"] if r["agent"] is None)


def test_sharded_launch_equilibrium_equal_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 101
    sw = {"gamma": [[0.35, 0.9, 0.95][g % 3] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "sweep": sw,
                              "deviation": {"steps": 4}, "equilibrium": True})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    assert json.load(open(tmp_path / "one" / "equilibrium.json")) == json.load(open(tmp_path / "two" / "equilibrium.json"))
    for f in ("cycle", "iters", "diff", "loss", "value"):
        x, y = np.load(tmp_path / "one" / ("eq_%s.npy" % f)), np.load(tmp_path / "two" / ("eq_%s.npy" % f))
        _bits_equal(x, y, f)
    for i in (0, 1):
        a, b = utils.equilibrium_games(str(tmp_path / "one"), i), utils.equilibrium_games(str(tmp_path / "two"), i)
        assert a.index.tolist() == b.index.tolist() == list(range(G))
        for c in a.columns:
            _bits_equal(a[c].to_numpy(), b[c].to_numpy(), c)
