"""Attractor analysis on the device (thrl_attractors, GameBatch.attractors, training.attractors): every output,
state_rep and state_mu included, bit-equal to the numpy mirror (tests/attractors_mirror.py, which walks every state
where the kernel doubles pointers) on fresh and trained headline tables in f32 and f64, individual grids (S = 87:
several states per lane), the 3,000-state config (3,001 reset starts), a given policy with no tables, a convergence
tracker's policy and a game count below the batch's; the known answers through set_tables; the training state's cycle
against the deviation analysis; the accounting identities; and the invariances (training state, game order, shard
split, MixedGameBatch, the trainer's artefacts, a sharded launch)."""
import ctypes
import json

import numpy as np
import pytest

import attractors_mirror as A
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
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}
GAME_FIELDS = ("n_attr", "mu_max", "n_cycle_states", "rep_x0", "mu_x0", "slot_x0")
SLOT_FIELDS = ("rep", "lam", "basin", "cycle_reward", "cycle_action")
RESET_FIELDS = ("reset_mass", "reset_mass_other", "reset_reward")
STATE_FIELDS = ("state_rep", "state_mu")
ALL_FIELDS = GAME_FIELDS + SLOT_FIELDS + RESET_FIELDS + STATE_FIELDS
X0_FIELDS = ("rep_x0", "mu_x0", "slot_x0")


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _batch(config, G, dtype="float32", seed=3, episodes=0):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, seed=seed).init_tables()
    if episodes:
        gb.run(episodes, logs=False)
    return gb


def _check(gb, config, state0=None, n_games=None, **kw):
    from th_rl_amd import attractors as at
    out = gb.attractors(state0=state0, policies=True, n_games=n_games, **kw)
    s0 = gb.states_numpy() if state0 is None else state0
    ref = A.analyse(config, gb.tables_numpy(), s0, reset=at.starts(config), n_games=n_games)
    assert out["n_states"] == ref["n_states"]
    for f in ALL_FIELDS:
        _bits_equal(out[f], ref[f], f)
    _identities(out)
    return out


def _identities(out):
    """What holds for every game whatever the tables: the basins partition the states, the masses the reset
    distribution."""
    S = out["n_states"]
    kept = out["basin"].sum(axis=0)
    assert (kept <= S).all() and ((kept == S) == (out["n_attr"] <= A.KEEP)).all()
    assert (out["lam"].sum(axis=0) <= out["n_cycle_states"]).all() and (out["n_cycle_states"] <= S).all()
    assert (out["n_attr"] >= 1).all() and ((out["rep"] >= 0).sum(axis=0) == np.minimum(out["n_attr"], A.KEEP)).all()
    assert (np.diff(out["basin"], axis=0) <= 0).all()
    if "reset_mass" in out:
        total = out["reset_mass"].sum(axis=0) + out["reset_mass_other"]
        print("max |sum of reset masses - 1| = %.3e (J = %d)" % (np.abs(total - 1.0).max(), out["n_starts"]))
        assert np.all(np.abs(total - 1.0) <= out["n_starts"] * 2.0 ** -52)          # J ulp
        assert ((out["reset_mass_other"] == 0) | (out["n_attr"] > A.KEEP)).all()


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("episodes", [0, 200, 1600])
def test_headline_matches_mirror(dtype, episodes):
    gb = _batch(TWO, 139, dtype, seed=11, episodes=episodes)           # 139: no multiple of a wave or a block
    out = _check(gb, TWO)
    assert out["n_states"] == 41 and out["n_starts"] == 101
    if episodes == 0:
        # the condition the other cases rest on, on the device's own fresh tables
        assert np.mean(out["n_attr"] >= 2) >= 0.5 and out["n_attr"].max() <= A.KEEP
    _check(gb, TWO, state0=np.random.RandomState(2).uniform(0, 10, gb.G))


def test_three_agents_individual_grids_several_states_per_lane():
    gb = _batch(THREE, 96, seed=5, episodes=50)
    out = _check(gb, THREE)
    assert out["n_states"] == 87 and out["n_states"] > 64
    _check(gb, THREE, state0=np.linspace(0.0, 10.0, 96))


def test_3000_state_config_matches_mirror():
    from th_rl_amd import attractors as at
    assert at.starts(BIG)[1].size == 3001                               # 47 chunks of starts per game
    gb = _batch(BIG, 48, seed=6, episodes=20)
    out = _check(gb, BIG)
    assert out["n_states"] == 41


def test_policy_given_plays_the_policy_and_reads_no_table():
    import torch
    from th_rl_amd import _lib, attractors as at, crossplay as xp
    G = 77
    gb = _batch(TWO, G, seed=8, episodes=100)
    want = gb.attractors(policies=True)
    pol = xp.extract(gb)
    got = gb.attractors(policies=True, policy=pol)
    for f in ALL_FIELDS:
        _bits_equal(got[f], want[f], f)
    # the extraction of this call is the one of cross-play
    assert np.array_equal(pol.cpu().numpy().view(np.uint16), A.policies(TWO, gb.tables_numpy()))
    # q = NULL through the library itself
    a = _lib.AttractorsArgs()
    a.n_games, a.flags = G, _lib.ATTR_POLICY_GIVEN
    dev = gb.device
    keep = {f: torch.zeros((G,), dtype=torch.int32, device=dev) for f in GAME_FIELDS}
    keep.update({f: torch.zeros((A.KEEP, G), dtype=torch.int32, device=dev) for f in ("rep", "lam", "basin")})
    keep.update({f: torch.zeros((A.KEEP, 2, G), dtype=torch.float64, device=dev) for f in ("cycle_reward", "cycle_action")})
    for f, t in keep.items():
        setattr(a, f, t.data_ptr())
    a.state0, a.policy = gb.state.data_ptr(), pol.data_ptr()
    assert gb.L.thrl_attractors(ctypes.byref(gb.cfg), None, ctypes.byref(a), gb._stream()) == 0
    torch.cuda.synchronize(dev)
    for f, t in keep.items():
        _bits_equal(t.cpu().numpy(), want[f], f)
    # entries that are no action are clamped to the last action, as in cross-play
    bad = pol.clone()
    bad[:, ::3] = 999
    ref = A.analyse(TWO, None, gb.states_numpy(), policy=bad.cpu().numpy().view(np.uint16), reset=at.starts(TWO))
    got = gb.attractors(policies=True, policy=bad)
    for f in ALL_FIELDS:
        _bits_equal(got[f], ref[f], f)


def test_a_convergence_trackers_policy_serves_this_call():
    gb = _batch(TWO, 90, seed=13, episodes=40)
    tr = gb.track_convergence(window=10, every=5)
    gb.run(20, logs=False)
    tr.check()
    got = gb.attractors(policies=True, policy=tr.policy)
    want = gb.attractors(policies=True)
    for f in ALL_FIELDS:
        _bits_equal(got[f], want[f], f)
    _check(gb, TWO)


def test_fewer_games_than_the_batch_holds():
    gb = _batch(TWO, 150, seed=9, episodes=30)
    part = _check(gb, TWO, n_games=67)
    full = gb.attractors(policies=True)
    for f in GAME_FIELDS + SLOT_FIELDS + RESET_FIELDS:
        assert part[f].shape[-1] == 67
        _bits_equal(part[f], full[f][..., :67], f)
    for f in STATE_FIELDS:
        _bits_equal(part[f], full[f][:67], f)


def test_more_games_than_resident_blocks():
    """Every block loops over several games (at most 16 one-wave blocks per CU are launched): the first, a middle and
    the last stretch of 6,000 games against the mirror, and the fresh-table condition on all of them."""
    from th_rl_amd import attractors as at
    G = 6000
    gb = _batch(SYM, G, seed=1)
    out = gb.attractors(policies=True)
    _identities(out)
    q, s0, reset = gb.tables_numpy(), gb.states_numpy(), at.starts(SYM)
    for lo, hi in ((0, 40), (4090, 4130), (G - 40, G)):
        ref = A.analyse(SYM, q[lo:hi], s0[lo:hi], reset=reset)
        for f in GAME_FIELDS + SLOT_FIELDS + RESET_FIELDS:
            _bits_equal(out[f][..., lo:hi], ref[f], f)
        for f in STATE_FIELDS:
            _bits_equal(out[f][lo:hi], ref[f], f)
    print("fresh games with two or more attractors: %.3f, most: %d" % (np.mean(out["n_attr"] >= 2), out["n_attr"].max()))
    assert np.mean(out["n_attr"] >= 2) >= 0.5


# ------------------------------------------------------------------------------------------------ known answers
def _known(config, tables, state0, dtype="float64"):
    from th_rl_amd.batched import GameBatch
    G = len(state0)
    gb = GameBatch(config, n_games=G, dtype=dtype).set_tables(tables, state0)
    return gb.attractors(policies=True)


def test_known_constant_policies_have_one_fixed_point():
    pl = E.plan(SYM)
    for dtype in ("float32", "float64"):
        o = _known(SYM, E.strategy_tables(SYM, [5, 5], 2), [3.0, 7.5], dtype)
        fixed = int(pl["sid"][5 * 21 + 5])
        assert o["n_attr"].tolist() == [1, 1] and o["mu_max"].tolist() == [1, 1] and o["n_cycle_states"].tolist() == [1, 1]
        assert o["rep"][0].tolist() == [fixed] * 2 and o["lam"][0].tolist() == [1, 1] and o["basin"][0].tolist() == [41, 41]
        assert (o["rep"][1:] == -1).all() and not o["basin"][1:].any() and not o["cycle_reward"][1:].any()
        assert (o["state_rep"] == fixed).all() and (o["state_mu"].sum(axis=1) == 40).all()
        assert o["slot_x0"].tolist() == [0, 0] and o["rep_x0"].tolist() == [fixed] * 2 and o["mu_x0"].tolist() == [1, 1]
        _bits_equal(o["cycle_reward"][0, 0], np.full(2, pl["rew"][0][5 * 21 + 5]), "cycle_reward")
        r1 = pl["rew"][1][5 * 21 + 5]
        assert np.all(np.abs(o["reset_reward"][1] - r1) <= 2 * 101 * 2.0 ** -52 * r1)
        assert np.all(np.abs(o["reset_mass"][0] - 1.0) <= 101 * 2.0 ** -52) and not o["reset_mass"][1:].any()


def test_known_every_state_a_fixed_point():
    pl = E.plan(SYM)
    o = _known(SYM, A.fixed_point_tables(SYM, 2), [3.0, 5.0])
    assert o["n_attr"].tolist() == [41, 41] and o["n_cycle_states"].tolist() == [41, 41] and not o["mu_max"].any()
    for g in range(2):
        assert o["rep"][:, g].tolist() == list(range(8)) and o["lam"][:, g].tolist() == [1] * 8
        assert o["basin"][:, g].tolist() == [1] * 8 and o["state_rep"][g].tolist() == list(range(41))
    # states 0 .. 7 are rows 60 .. 53; the rows no state has play action 0 and land in state 0 (row 60)
    assert [int(pl["srow"][0][s]) for s in range(8)] == list(range(60, 52, -1))
    assert np.all(np.abs(o["reset_mass_other"] - 0.33) <= 1e-12) and np.all(np.abs(o["reset_mass"][1:].sum(axis=0) - 0.07) <= 1e-12)
    # price 5.0 is row 50, the state of the tuple (5, 5): wherever that state is numbered, it is its own attractor
    s = int(pl["sid"][5 * 21 + 5])
    assert o["rep_x0"][1] == s and o["mu_x0"][1] == 0 and o["slot_x0"][1] == (s if s < 8 else -1)


def test_known_planted_two_cycle_and_fixed_point():
    """Rows up to 30 play 20 (price 2, row 20: a fixed point), the rows above play 5 (price 5, row 50), row 50 plays 13
    (price 3.4, row 34) and row 34 plays 5 again: the 2-cycle 50 <-> 34 draws the 30 states with rows above 30, the
    fixed point the 11 states with rows 20 .. 30."""
    from th_rl_amd import attractors as at
    pl = E.plan(SYM)
    strat = np.where(np.arange(101) <= 30, 20, 5)
    strat[50] = 13
    assert sorted(pl["srow"][0].tolist()) == list(range(20, 61))
    x, y, z = (int(pl["sid"][a * 21 + a]) for a in (5, 13, 20))
    assert [int(pl["srow"][0][s]) for s in (x, y, z)] == [50, 34, 20]
    o = _known(SYM, E.strategy_tables(SYM, [strat, strat], 3), [5.0, 2.9, 9.9])
    assert o["n_attr"].tolist() == [2] * 3 and o["n_cycle_states"].tolist() == [3] * 3 and o["mu_max"].tolist() == [1] * 3
    for g in range(3):
        assert o["rep"][:2, g].tolist() == [min(x, y), z] and o["lam"][:2, g].tolist() == [2, 1]
        assert o["basin"][:2, g].tolist() == [30, 11]
    R = pl["rew"][0]
    _bits_equal(o["cycle_reward"][0, 0], np.full(3, (R[5 * 21 + 5] + R[13 * 21 + 13]) / 2.0), "two-cycle reward")
    _bits_equal(o["cycle_reward"][1, 0], np.full(3, R[20 * 21 + 20]), "fixed-point reward")
    assert o["slot_x0"].tolist() == [0, 1, 0] and o["mu_x0"].tolist() == [0, 1, 1]
    # rows 0 .. 30 of the reset distribution end in the fixed point: prices below 3.05
    assert np.all(np.abs(o["reset_mass"][1] - 0.305) <= 101 * 2.0 ** -52)
    ref = A.analyse(SYM, E.strategy_tables(SYM, [strat, strat], 3), [5.0, 2.9, 9.9], reset=at.starts(SYM))
    for f in ALL_FIELDS:
        _bits_equal(o[f], ref[f], f)


# ------------------------------------------------------------------------------------------------ cross-checks
def test_training_state_equals_the_deviation_analysis():
    for cfg, G, ep in ((TWO, 150, 0), (TWO, 150, 200), (THREE, 64, 30)):
        gb = _batch(cfg, G, seed=21, episodes=ep)
        s0 = np.random.RandomState(4).uniform(0, 10, G)
        for st in (None, s0):
            o, d = gb.attractors(state0=st), gb.deviation(state0=st, steps=2)
            _identities(o)
            kept = o["slot_x0"] >= 0
            assert kept.all() or o["n_attr"][~kept].min() > A.KEEP
            _bits_equal(o["mu_x0"], d["mu"], "mu")
            g = np.flatnonzero(kept)
            slot = o["slot_x0"][g]
            _bits_equal(o["lam"][slot, g], d["lam"][g], "lam")
            _bits_equal(o["rep"][slot, g], o["rep_x0"][g], "rep")
            for i in range(gb.N):
                got, want = o["cycle_reward"][slot, i, g], d["cycle_reward"][i][g]
                tol = 4 * d["lam"][g] * np.spacing(np.abs(want))
                print("agent %d: max |cycle_reward - deviation's| / (4 ulp lam) = %.3f" % (i, (np.abs(got - want) / tol).max()))
                assert np.all(np.abs(got - want) <= tol)


# ------------------------------------------------------------------------------------------------ invariances
def test_only_the_x0_outputs_depend_on_the_training_state():
    gb = _batch(TWO, 120, seed=12, episodes=40)
    before = (gb.tables_numpy().copy(), gb.counters_numpy().copy(), gb.states_numpy().copy(), list(gb.eps), gb.episode)
    a = gb.attractors(policies=True)
    b = gb.attractors(policies=True, state0=np.random.RandomState(1).uniform(0, 10, gb.G))
    after = (gb.tables_numpy(), gb.counters_numpy(), gb.states_numpy(), list(gb.eps), gb.episode)
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    for f in ALL_FIELDS:
        if f not in X0_FIELDS:
            _bits_equal(a[f], b[f], f)
    assert any(not np.array_equal(a[f], b[f]) for f in X0_FIELDS)


def test_game_order_and_shard_split():
    from th_rl_amd.batched import GameBatch
    G = 180
    gb = _batch(TWO, G, seed=12, episodes=40)
    full = gb.attractors(policies=True)
    q, s = gb.tables_numpy(), gb.states_numpy()
    perm = np.random.RandomState(3).permutation(G)
    sh = GameBatch(TWO, n_games=G, seed=12).set_tables(q[perm], s[perm]).attractors(policies=True)
    for f in GAME_FIELDS + SLOT_FIELDS + RESET_FIELDS:
        _bits_equal(sh[f], full[f][..., perm], f)
    for f in STATE_FIELDS:
        _bits_equal(sh[f], full[f][perm], f)
    for lo, hi in ((0, 77), (77, G)):
        h = GameBatch(TWO, n_games=hi - lo, seed=12, game_offset=lo).set_tables(q[lo:hi], s[lo:hi])
        part = h.attractors(policies=True)
        for f in GAME_FIELDS + SLOT_FIELDS + RESET_FIELDS:
            _bits_equal(part[f], full[f][..., lo:hi], f)
        for f in STATE_FIELDS:
            _bits_equal(part[f], full[f][lo:hi], f)


def test_mixed_batch_equals_game_batch():
    from th_rl_amd.mixed import MixedGameBatch
    from th_rl_amd._lib import ThrlError
    G = 96
    for dtype in ("float32", "float64"):
        gb = _batch(TWO, G, dtype, seed=14, episodes=30)
        mb = MixedGameBatch(TWO, n_games=G, dtype=dtype).set_tables(gb.tables_numpy(), gb.states_numpy())
        a, b = gb.attractors(policies=True), mb.attractors(policies=True)
        for f in ALL_FIELDS:
            _bits_equal(b[f], a[f], f)
    mx = MixedGameBatch(MIXED, n_games=8).init_tables()
    with pytest.raises(ThrlError, match="follow-up"):
        mx.attractors()


def test_reset_is_optional_and_error_codes_never_fault():
    from th_rl_amd import _lib
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.batched import GameBatch
    gb = _batch(TWO, 16, seed=1)
    o = gb.attractors(reset=False)
    assert "reset_mass" not in o and o["n_attr"].shape == (16,)
    full = gb.attractors()
    for f in GAME_FIELDS + SLOT_FIELDS:
        _bits_equal(o[f], full[f], f)
    with pytest.raises(ThrlError, match="n_games"):
        gb.attractors(n_games=17)
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}
    wb = GameBatch(wide, n_games=4, kernel="generic").init_tables()
    with pytest.raises(ThrlError) as e:
        wb.attractors()
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a = _lib.AttractorsArgs()
    a.n_games = 16
    assert gb.L.thrl_attractors(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(a), None) == -2


# ------------------------------------------------------------------------------------------------ trainer, launch
def test_train_one_attractor_artefacts_at_convergence(tmp_path):
    from th_rl_amd import trainer, utils, attractors as at
    G = 192
    cfg = dict(TWO, training={"epochs": 60, "print_freq": 500, "seed": 21, "n_games": G, "n_groups": 3,
                              "groups": [g % 3 for g in range(G)],
                              "convergence": {"window": 10, "every": 5, "snapshot": True},
                              "deviation": {"steps": 4, "tables": "converged"},
                              "attractors": {"tables": "converged", "policies": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "attractors.json"))
    assert desc["options"] == {"policies": True, "tables": "converged"} and desc["n_states"] == 41 and desc["n_starts"] == 101
    assert [r["group"] for r in desc["summary"]] == [0, 1, 2] and [r["games"] for r in desc["summary"]] == [G // 3] * 3
    games = at.load_games(str(exp))
    assert games["state_rep"].shape == (G, 41) and games["state_rep"].dtype == np.uint16
    # the artefacts are the mirror's on each converged game's snapshot and the final tables of the others
    import torch
    from th_rl_amd.batched import GameBatch
    ca = np.load(exp / "conv_episode.npy")
    sd = torch.load(exp / "convergence.pt", weights_only=True)
    gb = GameBatch(TWO, n_games=G).load(str(exp / "batch.pt"))
    m = torch.from_numpy(ca >= 0)
    q = torch.where(m[:, None], sd["q_conv"], gb.q.cpu()).numpy()
    s0 = torch.where(m, sd["state_conv"], gb.state.cpu()).numpy()
    ref = A.analyse(TWO, q, s0, reset=at.starts(TWO))
    for f in ALL_FIELDS:
        _bits_equal(games[f], ref[f], f)
    nash, cartel = at.optimal(TWO)
    assert desc["summary"] == json.loads(json.dumps(at.summarize(ref, np.arange(G) % 3, 3, nash, cartel)))
    # the training attractor is the deviation analysis' cycle on the same tables
    dv = utils.deviation_games(str(exp), 0)
    ag = utils.attractor_games(str(exp))
    assert ag["mu_x0"].tolist() == dv["mu"].tolist() and len(utils.attractor_summary(str(exp))) == 3
    assert np.all(np.abs(ag["delta_train"].to_numpy() - dv["delta"].to_numpy()) <= 1e-12)


def test_sharded_launch_attractors_equal_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 101
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "n_groups": 2,
                              "groups": [g % 2 for g in range(G)], "attractors": {"policies": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    assert json.load(open(tmp_path / "one" / "attractors.json")) == json.load(open(tmp_path / "two" / "attractors.json"))
    for f in ("games", "slots", "cycle", "reset_mass", "reset_reward", "state"):
        x, y = np.load(tmp_path / "one" / ("attr_%s.npy" % f)), np.load(tmp_path / "two" / ("attr_%s.npy" % f))
        _bits_equal(x, y, f)
    a, b = utils.attractor_games(str(tmp_path / "one")), utils.attractor_games(str(tmp_path / "two"))
    assert a.index.tolist() == b.index.tolist() == list(range(G))
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
