"""Cross-play on the device (thrl_crossplay, GameBatch.crossplay, training.crossplay): every output and row bit-equal
to the numpy mirror (tests/crossplay_mirror.py) on fresh and trained tables, f32 and f64, individual grids, the
3,000-state config (direct extraction and gathered walk), explicit random seats with repeats, M != G, given and default
start prices, a game count that is no multiple of anything; identity seats against the deviation analysis; the route
through set_tables + deviation; the policies against thrl_policy_track; known answers; and the invariances (learning
state untouched, halves, the sentinel of a seat out of range, MixedGameBatch, the trainer's artefacts, a sharded
launch, rows through group_stats).

In every mirror-compared case at least half of the matches must differ, in (mu, lam, s*), from the self-play of seat
0's game as the mirror computes it: the comparisons must not be satisfiable by self-play."""
import ctypes
import json

import numpy as np
import pytest

import crossplay_mirror as X
import deviation_mirror as M

pytestmark = pytest.mark.gpu

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}
OUT = ("mu", "lam", "cycle_reward", "cycle_action")
ROWS = ("reward_rows", "action_rows")


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


def _check(gb, config, seats, state0=None, steps=6, horizon=None, strangers=True):
    """One round against the mirror, outputs and rows; returns the device result."""
    seats = np.asarray(seats)
    out = gb.crossplay(seats, steps=steps, rows=True, state0=state0, horizon=horizon)
    s0 = gb.states_numpy()[seats[0]] if state0 is None else np.asarray(state0, np.float64)
    q = gb.tables_numpy()
    ref = X.analyse(config, q, seats, s0, steps=steps, horizon=horizon)
    if strangers:
        share = X.differs_from_self_play(config, q, seats, s0, ref, horizon=horizon).mean()
        print("matches that differ from seat 0's self-play: %.3f" % share)
        assert share >= 0.5, share
    for f in OUT + (ROWS if steps else ()):
        _bits_equal(out[f], ref[f], f)
    assert out["horizon"] == ref["horizon"]
    return out


def _rotate(G, k, n_agents=2):
    from th_rl_amd.crossplay import pairings
    return pairings(np.zeros(G, int), 1, "rotate", k, n_agents=n_agents)[-1]


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("episodes", [0, 300])
def test_headline_matches_mirror(dtype, episodes):
    G = 203                                                             # no multiple of a wave or a block
    gb = _batch(TWO, G, dtype, seed=11, episodes=episodes)
    for k in (1, 7):
        out = _check(gb, TWO, _rotate(G, k))
        assert out["mu"].min() >= 0 and out["lam"].min() >= 1           # the default horizon always finds the cycle
    _check(gb, TWO, _rotate(G, 3), state0=np.random.RandomState(2).uniform(0, 10, G))


def test_explicit_seats_with_repeats_and_other_match_counts():
    G = 203
    gb = _batch(TWO, G, seed=12, episodes=40)
    rs = np.random.RandomState(5)
    for Mn in (57, 203, 700):                                           # M < G, = G, > G
        seats = rs.randint(0, G, size=(2, Mn))                          # games repeat, seat 0 is no identity
        _check(gb, TWO, seats)
        _check(gb, TWO, seats, state0=rs.uniform(0, 10, Mn), steps=3)
    # a short horizon: matches whose cycle lies past it report lam = 0, mu = H, as the mirror does
    out = _check(gb, TWO, rs.randint(0, G, size=(2, 300)), horizon=3, steps=0)
    assert (out["lam"] == 0).any() and (out["mu"][out["lam"] == 0] == 3).all()


def test_three_agents_individual_grids():
    G = 96
    gb = _batch(THREE, G, seed=5, episodes=50)
    _check(gb, THREE, _rotate(G, 1, 3))
    _check(gb, THREE, np.random.RandomState(7).randint(0, G, size=(3, 150)), state0=np.linspace(0.0, 10.0, 150))


def test_3000_state_config_direct_extraction_and_gathered_walk():
    G = 64
    gb = _batch(BIG, G, seed=6, episodes=20)
    _check(gb, BIG, _rotate(G, 5))
    _check(gb, BIG, _rotate(G, 9), state0=np.linspace(0.5, 9.5, G), steps=4)


def test_three_agents_gathered_walk():
    """Three agents of 1,000 states each: the policy windows are past the walk's LDS budget (k_xplay_walk<gathered, 8>)."""
    config = {"agents": [dict(a, states=1000) for a in THREE["agents"]], "environment": THREE["environment"]}
    G = 300                                                             # a full block of 256 lanes and a partial one
    gb = _batch(config, G, seed=8)
    _check(gb, config, _rotate(G, 1, 3), strangers=False)
    rs = np.random.RandomState(8)
    out = _check(gb, config, rs.randint(0, G, size=(3, G)), state0=rs.uniform(0, 10, G), steps=3, horizon=3, strangers=False)
    assert (out["lam"] == 0).any() and (out["mu"][out["lam"] == 0] == 3).all()


def test_unaligned_tables_take_the_direct_extraction_path():
    import torch
    from th_rl_amd import crossplay as xp
    G = 70
    gb = _batch(TWO, G, seed=8, episodes=20)
    flat = torch.empty((G * gb.stride + 1,), dtype=gb.q.dtype, device=gb.q.device)
    shifted = flat[1:].view(G, gb.stride)                               # 4 bytes off a 16-byte boundary
    shifted.copy_(gb.q)
    assert shifted.data_ptr() % 16 != 0 and gb.q.data_ptr() % 16 == 0
    a, b = xp.extract(gb), xp.extract(gb, q=shifted)
    assert torch.equal(a, b)
    _bits_equal(a.cpu().numpy().view(np.uint16), X.policies(TWO, gb.tables_numpy()), "policy")
    seats = _rotate(G, 2)
    x, y = gb.crossplay(seats), gb.crossplay(seats, q=shifted)
    for f in OUT:
        _bits_equal(x[f], y[f], f)


# ------------------------------------------------------------------------------------------------ other routes
def test_identity_seats_equal_the_deviation_analysis():
    from th_rl_amd.crossplay import identity
    for cfg, G, ep in ((TWO, 150, 0), (TWO, 150, 200), (THREE, 64, 30)):
        gb = _batch(cfg, G, seed=21, episodes=ep)
        s0 = np.random.RandomState(4).uniform(0, 10, G)
        for st in (None, s0):
            x, d = gb.crossplay(identity(gb.N, G), state0=st), gb.deviation(state0=st, steps=2)
            for f in OUT:
                _bits_equal(x[f], d[f], f)


def test_equals_set_tables_on_a_second_batch_then_deviation():
    from th_rl_amd.batched import GameBatch
    G = 180
    for dtype in ("float32", "float64"):
        gb = _batch(TWO, G, dtype, seed=31, episodes=60)
        seats = np.random.RandomState(3).randint(0, G, size=(2, G))
        s0 = gb.states_numpy()[seats[0]]
        other = GameBatch(TWO, n_games=G, dtype=dtype).set_tables(X.cross_tables(TWO, gb.tables_numpy(), seats), s0)
        d = other.deviation(steps=2)
        x = gb.crossplay(seats)
        for f in OUT:
            _bits_equal(x[f], d[f], f)


def test_policy_is_the_trackers_baseline_and_can_be_given():
    from th_rl_amd import crossplay as xp
    for cfg, G, dtype in ((TWO, 203, "float32"), (TWO, 90, "float64"), (THREE, 64, "float32"), (BIG, 16, "float32")):
        gb = _batch(cfg, G, dtype, seed=41, episodes=20)
        tr = gb.track_convergence(window=5)                             # the baseline pass of thrl_policy_track
        pol = xp.extract(gb)
        assert pol.shape == tr.policy.shape and bool((pol == tr.policy).all())
        seats = np.random.RandomState(9).randint(0, G, size=(gb.N, 2 * G))
        a = gb.crossplay(seats, steps=4, rows=True)                     # extracts, then plays
        b = gb.crossplay(seats, steps=4, rows=True, policy=tr.policy)   # THRL_XPLAY_POLICY_GIVEN, q = NULL
        for f in OUT + ROWS:
            _bits_equal(a[f], b[f], f)


# ------------------------------------------------------------------------------------------------ known answers
def _known(tables, seats, state0, dtype="float64"):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(M.KNOWN, n_games=tables.shape[0], dtype=dtype).set_tables(tables, np.full(tables.shape[0], 5.0))
    return gb.crossplay(np.asarray(seats), state0=state0, steps=4, rows=True)


def test_known_tit_for_tat_meets_always_undercut():
    """KNOWN's grid: action k produces 2.5 k, price 10 - 2.5 (k_0 + k_1), row 4 - (k_0 + k_1).  Tit for tat answers the
    rival's last output: from row r it plays 2 when the total was at least 3 (someone produced 2), else 1.  Always
    undercut plays 2.  Together: (1, 2) -> row 1 -> (2, 2) -> row 0 -> (2, 2): the punishment fixed point, price 0."""
    tft, cut = [2, 2, 1, 1, 1], [2, 2, 2, 2, 2]
    q = np.concatenate([M.one_hot_tables(tft), M.one_hot_tables(cut)])  # game 0 = two tit-for-tats, game 1 = two undercutters
    for dtype in ("float32", "float64"):
        o = _known(q, [[0, 1, 0], [1, 0, 0]], [7.5, 7.5, 7.5], dtype)   # tft vs cut, cut vs tft, tft vs tft; start row 3
        assert o["lam"].tolist() == [1, 1, 1] and o["mu"].tolist() == [2, 2, 1]
        assert o["cycle_reward"][:, :2].tolist() == [[0.0, 0.0], [0.0, 0.0]]        # price 0: nobody earns
        assert o["cycle_action"][:, :2].tolist() == [[0.5, 0.5], [0.5, 0.5]]
        # two tit-for-tats stay at (1, 1): price 5, each sells 2.5
        assert o["cycle_reward"][:, 2].tolist() == [12.5, 12.5] and o["cycle_action"][:, 2].tolist() == [0.25, 0.25]
        # the path of match 0: (1, 2) at price 2.5, then (2, 2) at price 0
        assert o["reward_rows"][:, :, 0].tolist() == [[6.25, 12.5], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
        assert o["action_rows"][:2, :, 0].tolist() == [[0.25, 0.5], [0.5, 0.5]]


def test_known_two_fixed_points_form_a_two_cycle_together():
    """Table a sits at row 2 in self-play (both play 1: 4 - 2 = 2), table b at row 4 (both play 0).  Agent 0 of the a
    game with agent 1 of the b game: row 2 -> (a[2], b[2]) = (1, 0) -> row 3 -> (a[3], b[3]) = (0, 2) -> row 2."""
    a, b = [1, 1, 1, 0, 1], [0, 0, 0, 2, 0]
    q = np.concatenate([M.one_hot_tables(a), M.one_hot_tables(b)])
    seats, s0 = [[0, 1, 0], [0, 1, 1]], [5.0, 10.0, 5.0]               # a & a from row 2, b & b from row 4, a & b from row 2
    for dtype in ("float32", "float64"):
        o = _known(q, seats, s0, dtype)
        assert o["lam"].tolist() == [1, 1, 2] and o["mu"].tolist() == [0, 0, 0]
        # (1, 0): price 7.5, agent 0 sells 2.5; (0, 2): price 5, agent 1 sells 5
        assert o["cycle_reward"][:, 2].tolist() == [(18.75 + 0.0) / 2, (0.0 + 25.0) / 2]
        assert o["cycle_action"][:, 2].tolist() == [0.125, 0.25]
        assert o["reward_rows"][:, :, 2].tolist() == [[18.75, 0.0], [0.0, 25.0]] * 2
        assert o["cycle_reward"][:, 0].tolist() == [12.5, 12.5] and o["cycle_reward"][:, 1].tolist() == [0.0, 0.0]
        ref = X.analyse(M.KNOWN, q, np.array(seats), s0, steps=4)
        for f in OUT + ROWS:
            _bits_equal(o[f], ref[f], f)


# ------------------------------------------------------------------------------------------------ invariances
def test_learning_state_untouched_and_halves_equal_whole():
    G = 180
    gb = _batch(TWO, G, seed=12, episodes=40)
    seats = np.random.RandomState(1).randint(0, G, size=(2, 333))
    before = (gb.tables_numpy().copy(), gb.counters_numpy().copy(), gb.states_numpy().copy(), list(gb.eps), gb.episode)
    full = gb.crossplay(seats, steps=5, rows=True)
    after = (gb.tables_numpy(), gb.counters_numpy(), gb.states_numpy(), list(gb.eps), gb.episode)
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    for lo, hi in ((0, 130), (130, 333)):
        part = gb.crossplay(seats[:, lo:hi], steps=5, rows=True)
        for f in OUT + ROWS:
            _bits_equal(part[f], full[f][..., lo:hi], f)
    # a list of rounds = the rounds one by one
    both = gb.crossplay([seats[:, :100], seats[:, 100:200]])
    for r, (lo, hi) in enumerate(((0, 100), (100, 200))):
        for f in OUT:
            _bits_equal(both[f][r], full[f][..., lo:hi], f)


def test_seat_out_of_range_gets_the_sentinel_and_disturbs_nobody():
    import torch
    from th_rl_amd import _lib, crossplay as xp
    from th_rl_amd._lib import ThrlError
    G, Mn = 100, 300
    gb = _batch(TWO, G, seed=13, episodes=30)
    seats = np.random.RandomState(2).randint(0, G, size=(2, Mn)).astype(np.int32)
    good = gb.crossplay(seats, steps=3, rows=True)
    bad = seats.copy()
    where = {5: (0, G), 77: (1, -1), 256: (1, 1 << 30), 299: (0, -(1 << 31))}
    for m, (i, v) in where.items():
        bad[i, m] = v
    with pytest.raises(ThrlError, match="seats must lie"):
        gb.crossplay(bad)                                               # the Python layer sees host arrays
    dev = gb.device
    with torch.cuda.device(dev):
        t = {"seat": torch.from_numpy(bad).to(dev), "state0": gb.state.index_select(0, torch.from_numpy(seats[0]).long().to(dev)),
             "policy": xp.extract(gb), "mu": torch.full((Mn,), 9, dtype=torch.int32, device=dev),
             "lam": torch.full((Mn,), 9, dtype=torch.int32, device=dev),
             "cycle_reward": torch.full((2, Mn), 9.0, dtype=torch.float64, device=dev),
             "cycle_action": torch.full((2, Mn), 9.0, dtype=torch.float64, device=dev),
             "reward_rows": torch.full((3, 2, Mn), 9.0, dtype=torch.float64, device=dev),
             "action_rows": torch.full((3, 2, Mn), 9.0, dtype=torch.float64, device=dev)}
        a = _lib.CrossplayArgs()
        a.n_games, a.n_matches, a.n_steps, a.horizon, a.row_count, a.flags = G, Mn, 3, good["horizon"], 3, 1
        for f, x in t.items():
            setattr(a, f, x.data_ptr())
        _lib.check(gb.L.thrl_crossplay(ctypes.byref(gb.cfg), None, ctypes.byref(a), gb._stream()), "thrl_crossplay")
        torch.cuda.synchronize(dev)
    got = {f: t[f].cpu().numpy() for f in OUT + ROWS}
    ok = np.ones(Mn, bool)
    ok[list(where)] = False
    for f in OUT + ROWS:
        _bits_equal(got[f][..., ok], good[f][..., ok], f)
    assert got["mu"][~ok].tolist() == [-1] * 4 and got["lam"][~ok].tolist() == [0] * 4
    for f in OUT[2:] + ROWS:
        assert not got[f][..., ~ok].any(), f


def test_mixed_batch_equals_game_batch():
    from th_rl_amd.mixed import MixedGameBatch
    from th_rl_amd._lib import ThrlError
    G = 96
    seats = np.random.RandomState(6).randint(0, G, size=(2, 150))
    for dtype in ("float32", "float64"):
        gb = _batch(TWO, G, dtype, seed=14, episodes=30)
        mb = MixedGameBatch(TWO, n_games=G, dtype=dtype).set_tables(gb.tables_numpy(), gb.states_numpy())
        a, b = gb.crossplay(seats, steps=3, rows=True), mb.crossplay(seats, steps=3, rows=True)
        for f in OUT + ROWS:
            _bits_equal(b[f], a[f], f)
    mx = MixedGameBatch(MIXED, n_games=8).init_tables()
    with pytest.raises(ThrlError, match="follow-up"):
        mx.crossplay(np.zeros((2, 4), int))


def test_rows_through_group_stats_equal_group_stats_of_the_rows():
    from th_rl_amd.crossplay import pairings
    from th_rl_amd.group_stats import GroupSpec, reduce_host
    G, K = 150, 7
    gb = _batch(TWO, G, seed=15, episodes=40)
    ids = np.arange(G) % 3
    spec = GroupSpec.from_config(TWO, G, True, groups=ids.tolist(), n_groups=3)
    rounds = pairings(ids, 3, "rotate", 2, "own")
    out = gb.crossplay(rounds, steps=K, rows=True, group_stats=spec, budget=8 * 2 * G * 3)    # three rows per chunk
    assert out["reward_rows"].shape == (2, K, 2, G)
    want = None
    for r in range(2):
        part = reduce_host(out["reward_rows"][r], out["action_rows"][r], ids, 3, spec.describe())
        if want is None:
            want = {f: np.array(v) for f, v in part.items()}
        else:
            want["hist"] += part["hist"]
            want["sums"] += part["sums"]
            want["minmax"] = np.maximum(want["minmax"].view(np.uint64), np.asarray(part["minmax"]).view(np.uint64))
    for f in ("hist", "sums", "minmax"):
        assert np.array_equal(np.asarray(out["group_stats"][f]).astype(np.uint64).ravel(),
                              np.asarray(want[f]).astype(np.uint64).ravel()), f


# ------------------------------------------------------------------------------------------------ trainer, launch
def test_train_one_crossplay_artefacts(tmp_path):
    from th_rl_amd import trainer, utils, crossplay as xp
    from th_rl_amd.batched import GameBatch
    G = 256
    sw = {"gamma": [[0.5, 0.9, 0.95, 0.35][g % 4] for g in range(G)]}
    opt = {"rounds": 3, "scheme": "random", "against": "all", "steps": 5, "seed": 2}
    cfg = dict(TWO, training={"epochs": 40, "print_freq": 500, "seed": 21, "n_games": G, "sweep": sw,
                              "group_stats": True, "crossplay": opt})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "crossplay.json"))
    assert desc["options"]["rounds_played"] == 12 and desc["options"]["against"] == "all"
    assert [(r["group"], r["partner_group"]) for r in desc["summary"]] == [(a, b) for a in range(4) for b in range(4)]
    games, self_play = xp.load_games(str(exp))
    assert games["seats"].shape == (12, 2, G) and np.load(exp / "xplay_cycle.npy").shape == (12, 2, G)
    # equal to the batch method on the final tables, and to the mirror
    gb = GameBatch(TWO, n_games=G, sweep=sw).load(str(exp / "batch.pt"))
    ids = np.arange(G) % 4
    rounds = xp.pairings(ids, 4, "random", 3, "all", seed=2)
    assert np.array_equal(np.stack(rounds), games["seats"])
    out = gb.crossplay(rounds)
    for f in OUT:
        _bits_equal(games[f], out[f], f)
    for r in (0, 7):
        ref = X.analyse(TWO, gb.tables_numpy(), rounds[r], gb.states_numpy())
        for f in OUT:
            _bits_equal(games[f][r], ref[f], f)
    own = gb.deviation(steps=2)
    _bits_equal(self_play["lam"], own["lam"], "self lam")
    _bits_equal(self_play["cycle_reward"], own["cycle_reward"], "self reward")
    nash, cartel = xp.optimal(TWO)
    assert desc["summary"] == json.loads(json.dumps(xp.summarize(games, self_play, ids, 4, nash, cartel)))
    assert np.load(exp / "xplay_mean.npy").shape[0] == 5                # the pooled path rows, one per step
    df = utils.crossplay_games(str(exp), 4)
    assert df.index.tolist() == list(range(G)) and df["seat_1"].tolist() == rounds[4][1].tolist()
    assert len(utils.crossplay_summary(str(exp))) == 16


def test_train_one_crossplay_on_converged_tables(tmp_path):
    import torch
    from th_rl_amd import trainer, crossplay as xp
    from th_rl_amd.batched import GameBatch
    G = 128
    cfg = dict(TWO, training={"epochs": 60, "print_freq": 500, "seed": 23, "n_games": G,
                              "convergence": {"window": 10, "every": 5, "snapshot": True},
                              "crossplay": {"rounds": 2, "tables": "converged"}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    assert json.load(open(exp / "crossplay.json"))["options"]["tables"] == "converged"
    games, _ = xp.load_games(str(exp))
    ca = np.load(exp / "conv_episode.npy")
    sd = torch.load(exp / "convergence.pt", weights_only=True)
    gb = GameBatch(TWO, n_games=G).load(str(exp / "batch.pt"))
    m = torch.from_numpy(ca >= 0)
    q = torch.where(m[:, None], sd["q_conv"], gb.q.cpu()).numpy()
    s0 = torch.where(m, sd["state_conv"], gb.state.cpu()).numpy()
    for r in (0, 1):
        ref = X.analyse(TWO, q, games["seats"][r], s0)
        for f in OUT:
            _bits_equal(games[f][r], ref[f], f)


def test_sharded_launch_merges_to_the_concatenation(tmp_path):
    from th_rl_amd import crossplay as xp
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.launch import launch
    from th_rl_amd.sharding import shard_range
    G = 101
    sw = {"gamma": [[0.35, 0.9, 0.95][g % 3] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "sweep": sw,
                              "crossplay": {"rounds": 2, "against": "all"}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    out = tmp_path / "two"
    launch(str(tmp_path / "c.json"), str(out), gpus=2)
    merged, merged_self = xp.load_games(str(out))
    parts = [xp.load_games(str(out / ("shard%d" % r))) for r in (0, 1)]
    for f in merged:
        _bits_equal(merged[f], np.concatenate([p[0][f] for p in parts], axis=-1), f)
    assert merged["seats"].shape == (6, 2, G) and merged["seats"][:, 0].tolist() == [list(range(G))] * 6
    # the seats, replayed by the mirror on each shard's tables, give the merged outputs; partners stay in the shard
    for r in (0, 1):
        lo, n = shard_range(G, r, 2)
        gb = GameBatch(TWO, n_games=n, sweep={"gamma": sw["gamma"][lo:lo + n]}).load(str(out / ("shard%d" % r) / "batch.pt"))
        seats = merged["seats"][:, :, lo:lo + n] - lo
        assert seats.min() >= 0 and seats.max() < n
        for k in (0, 3):
            ref = X.analyse(TWO, gb.tables_numpy(), seats[k], gb.states_numpy())
            for f in OUT:
                _bits_equal(merged[f][k][..., lo:lo + n], ref[f], f)
    desc = json.load(open(out / "crossplay.json"))
    nash, cartel = xp.optimal(TWO)
    ids = np.arange(G) % 3
    assert desc["summary"] == json.loads(json.dumps(xp.summarize(merged, merged_self, ids, 3, nash, cartel)))
