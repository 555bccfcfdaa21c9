"""The tuple form of greedy play on the device (thrl_tuple_policy, thrl_tuple_walk, MixedGameBatch.greedy_cycles,
training.greedy_cycles): the extracted strategies against thrl_nn_act / thrl_ac_act called once per tuple price (no
tolerance) and against crossplay's extraction at the rows of the tuple prices; the walk bit-equal to the numpy mirror
(tests/tuple_play_mirror.py) fed the device's strategies; against thrl_crossplay on an all-QTable batch; against
play_greedy; sentinels, invariances and the trainer's artefacts.

Fresh networks are nearly constant in the price, so the networks here get weights with kinks inside the price range:
every extraction test asserts on the device result that the neural rows are not constant, and every random-seat case
that at least half of the matches differ from seat 0's self-play."""
import json

import numpy as np
import pytest

import tuple_play_mirror as TM

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
CONFIGS = {"MIXED": (MIXED, 441), "AC": (AC, 105), "NN2": (NN2, 672), "THREE": (THREE, 385)}
OUT = ("mu", "lam", "cycle_start", "cycle_reward", "cycle_action")
ROWS = ("reward_rows", "action_rows")
G = 203                                                                 # no multiple of the 4 games per block or of a wave


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


def _policy(mb):
    from th_rl_amd import tuple_play as tp
    return tp.extract(mb).cpu().numpy().view(np.uint16)


def _check_neural_rows(mb, config, pol, share):
    """Every neural entry equals the act kernel called once per tuple price; the rows are not constant."""
    import torch
    from th_rl_amd import tuple_play as tp
    price = tp.tables(config)["price"]
    varied = np.zeros(mb.G, bool)
    for i, rb in mb.nn.items():
        want = np.stack([rb.act(torch.full((mb.G,), float(p), dtype=torch.float64)).cpu().numpy() for p in price], axis=1)
        _bits_equal(pol[:, i, :], want, "agent %d" % i)
        assert pol[:, i, :].max() < rb.A
        varied |= np.array([np.unique(r).size >= 2 for r in pol[:, i, :]])
    print("games with a neural row of >= 2 distinct actions: %.3f" % varied.mean())
    assert varied.mean() >= share, varied.mean()


@pytest.fixture(scope="module")
def trained():
    """MIXED with kinked networks after 20 training episodes: the batch, its tables, its strategies."""
    from th_rl_amd import tuple_play as tp
    mb = _mixed(MIXED, seed=7, weights_seed=4)
    mb.run(20, per_game_logs=False)
    return mb, tp.tables(MIXED), _policy(mb)


# ------------------------------------------------------------------------------------------------ extraction
@pytest.mark.parametrize("name", ["MIXED", "AC", "NN2", "THREE"])
def test_neural_entries_equal_the_act_kernel(name):
    config, T = CONFIGS[name]
    mb = _mixed(config, seed=5)
    pol = _policy(mb)
    assert pol.shape == (G, len(config["agents"]), T)
    _check_neural_rows(mb, config, pol, 0.25 if name == "AC" else 0.5)


def test_neural_entries_after_training_and_one_game(trained):
    mb, _, pol = trained
    _check_neural_rows(mb, MIXED, pol, 0.5)
    one = _mixed(MIXED, n_games=1, seed=9, weights_seed=8)
    _check_neural_rows(one, MIXED, _policy(one), 0.0)


@pytest.mark.parametrize("kind", ["Reinforce", "ActorCritic"])
@pytest.mark.parametrize("A", [2, 8, 9, 24, 25, 32])
def test_neural_strategy_and_price_probs_against_the_float64_mirror(A, kind):
    """k_tp_neural and k_tp_probs against tests/policy_reference.py, not against the act kernel: every strategy entry
    of the neural agent lies in the mirror's argmax set at that tuple's price, every probability of price_probs within
    the derived bound.  Action counts at both dispatch edges and at 2 and 32; ActorCritic with a value head that is
    far from zero behind the policy's parameters."""
    import policy_reference as PR
    from th_rl_amd import sampled_play as sp, tuple_play as tp
    n = 5
    config = {"agents": [dict(AG, actions=5, states=30), dict(RF, name=kind, actions=A)], "environment": dict(ENV)}
    mb = _mixed(config, n_games=n, seed=17 + A, weights_seed=A)
    vh = kind == "ActorCritic"
    Pp = PR.n_policy_params(A)
    w = mb.nn[1].params.cpu().numpy().copy()
    if vh:
        w[:, Pp:] = np.random.RandomState(A).uniform(-1, 1, (n, 257)) * 1e3
        mb.nn[1].set_params(w)
    tabs = tp.tables(config)
    price, T = tabs["price"], int(tabs["T"])
    assert T == 5 * A and mb.nn[1].P == Pp + (257 if vh else 0)
    pol = _policy(mb)
    probs = sp.price_probs(mb, price)[1].cpu().numpy()
    assert pol.shape == (n, 2, T) and probs.shape == (n, T, A)
    worst, decided = 0.0, []
    for g in range(n):
        p64, S = PR.probs64(w[g], A, price, value_head=vh)
        bound = PR.prob_bound(p64, S)
        am = PR.argmax_set(p64, bound)
        decided.append(am.sum(axis=1) == 1)
        assert pol[g, 1].max() < A
        bad = np.flatnonzero(~am[np.arange(T), pol[g, 1].astype(np.int64)])
        assert bad.size == 0, (g, bad[:5], pol[g, 1][bad[:5]], [np.flatnonzero(am[t]) for t in bad[:5]])
        ratio = np.abs(probs[g].astype(np.float64) - p64) / bound
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (g, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        assert np.abs(probs[g].astype(np.float64).sum(axis=1) - 1.0).max() <= A * 2 * PR.U
    decided = np.concatenate(decided)
    print("A=%d %s: worst |dp| / bound %.4f, entries with one admissible action %.3f" % (A, kind, worst, decided.mean()))
    assert decided.mean() >= 0.9, decided.mean()                       # (of the mirror: the check above decides the entry)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("episodes", [0, 40])
def test_qtable_entries_equal_crossplay_extraction(dtype, episodes):
    from th_rl_amd import crossplay as xp, tuple_play as tp
    from th_rl_amd.batched import GameBatch
    mb = _mixed(MIXED, dtype=dtype, seed=11)
    if episodes:
        mb.run(episodes, per_game_logs=False)
    pol = _policy(mb)
    # an all-QTable batch holding the same agent-0 tables
    gb = GameBatch(TWO, n_games=G, dtype=dtype, seed=2).init_tables()
    q = gb.tables_numpy().copy()
    n0 = 101 * 21
    q[:, :n0] = mb.tables_numpy()[:, mb.offsets[0]:mb.offsets[0] + n0]
    gb.set_tables(q, gb.states_numpy())
    rows_pol = xp.extract(gb).cpu().numpy().view(np.uint16)
    price = tp.tables(MIXED)["price"]
    row = np.clip(np.rint(price / 10.0 * 100.0), 0, 100).astype(np.int64)       # encode64, half-even
    assert np.unique(row).size > 20
    _bits_equal(pol[:, 0, :], rows_pol[:, row], "agent 0")
    assert np.mean([np.unique(r).size >= 2 for r in pol[:, 0, :]]) >= 0.5


# ------------------------------------------------------------------------------------------------ walk vs mirror
def _check(mb, tabs, pol, seats, start, steps=6, horizon=None, strangers=True, budget=None):
    seats = np.asarray(seats)
    kw = {} if budget is None else {"budget": budget}
    out = mb.greedy_cycles(seats=seats, start=start, steps=steps, rows=True, horizon=horizon, **kw)
    ref = TM.analyse(tabs, pol, seats, start, steps=steps, horizon=horizon)
    if strangers:
        share = TM.differs_from_self_play(tabs, pol, seats, start, ref, horizon=horizon).mean()
        print("matches that differ from seat 0's self-play: %.3f" % share)
        assert share >= 0.5, share
    for f in OUT + (ROWS if steps else ()):
        _bits_equal(out[f], ref[f], f)
    assert out["horizon"] == ref["horizon"] and np.array_equal(out["start"], np.asarray(start))
    return out


def test_identity_seats_match_mirror(trained):
    mb, tabs, pol = trained
    from th_rl_amd import tuple_play as tp
    start = tp.start_tuples(mb, tabs).cpu().numpy()
    assert (start >= 0).all()                                           # a noise-free trained state is a tuple's price
    ident = tp.identity(2, G)
    out = _check(mb, tabs, pol, ident, start, strangers=False)
    assert out["mu"].min() >= 0 and out["lam"].min() >= 1               # the default horizon always finds the cycle
    dflt = mb.greedy_cycles()                                           # default seats and start
    for f in OUT:
        _bits_equal(dflt[f], out[f], f)
    assert np.array_equal(dflt["start"], start) and np.array_equal(dflt["seats"], ident)


@pytest.mark.parametrize("M", [57, 203, 700])
@pytest.mark.parametrize("steps", [0, 6])
def test_random_seats_and_starts_match_mirror(trained, M, steps):
    mb, tabs, pol = trained
    rs = np.random.RandomState(M + steps)
    seats = rs.randint(0, G, size=(2, M))                               # games repeat, seat 0 is no identity
    _check(mb, tabs, pol, seats, rs.randint(0, 441, size=M), steps=steps)


def test_short_horizon_and_chunked_rows(trained):
    mb, tabs, pol = trained
    rs = np.random.RandomState(21)
    seats, start = rs.randint(0, G, size=(2, 300)), rs.randint(0, 441, size=300)
    # Under horizon 3 a match and seat 0's self-play that both run past three steps report the same (3, 0, -1), so the
    # triple cannot tell them apart there; that these seats are strangers is asserted at the default horizon below.
    out = _check(mb, tabs, pol, seats, start, horizon=3, steps=0, strangers=False)
    assert (out["lam"] == 0).any() and (out["mu"][out["lam"] == 0] == 3).all()
    assert (out["cycle_start"][out["lam"] == 0] == -1).all() and (out["lam"] > 0).any()
    whole = _check(mb, tabs, pol, seats, start, steps=7)
    parts = _check(mb, tabs, pol, seats, start, steps=7, budget=8 * 2 * 300 * 2)    # two rows per chunk
    for f in ROWS:
        _bits_equal(parts[f], whole[f], f)


@pytest.mark.parametrize("name", ["NN2", "THREE"])
def test_other_configs_match_mirror(name):
    from th_rl_amd import tuple_play as tp
    config, T = CONFIGS[name]
    N = len(config["agents"])
    mb = _mixed(config, n_games=96, seed=13, weights_seed=6)
    tabs, pol = tp.tables(config), _policy(mb)
    rs = np.random.RandomState(3)
    _check(mb, tabs, pol, rs.randint(0, 96, size=(N, 150)), rs.randint(0, T, size=150), steps=4)


# reward and scaled tables past the LDS budget (2 N T doubles > 64 KiB): k_tp_walk reads them from global memory
GLOBAL_TABLES = {"TWO": ({"agents": [dict(AG, actions=128), dict(RF, actions=32)], "environment": dict(ENV)}, 4096),
                 "THREE": ({"agents": [dict(THREE["agents"][0], actions=16), THREE["agents"][1], dict(THREE["agents"][2], actions=8)],
                            "environment": THREE["environment"]}, 1408)}


@pytest.mark.parametrize("name", list(GLOBAL_TABLES))
def test_tables_in_global_memory_match_mirror(name):
    from th_rl_amd import tuple_play as tp
    config, T = GLOBAL_TABLES[name]
    N = len(config["agents"])
    assert 2 * N * T * 8 > 64 * 1024
    mb = _mixed(config, n_games=40, seed=17, weights_seed=8)
    tabs, pol = tp.tables(config), _policy(mb)
    assert tabs["T"] == T
    rs = np.random.RandomState(5)
    seats, start = rs.randint(0, 40, size=(N, 300)), rs.randint(0, T, size=300)     # a full block of 256 lanes and a partial one
    _check(mb, tabs, pol, seats, start, steps=4, strangers=False)
    out = _check(mb, tabs, pol, seats, start, horizon=2, steps=0, strangers=False)
    assert (out["lam"] == 0).any() and (out["mu"][out["lam"] == 0] == 2).all()


# ------------------------------------------------------------------------------------------------ existing analyses
def test_all_qtable_batch_against_crossplay():
    from th_rl_amd import crossplay as xp, tuple_play as tp
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(TWO, n_games=G, seed=11).init_tables()
    gb.run(300, logs=False)
    tabs = tp.tables(TWO)
    start = tp.start_tuples(gb, tabs).cpu().numpy()
    assert (start >= 0).all()
    ident = xp.identity(2, G)
    t = tp.run(gb, ident, start=start)
    r = gb.crossplay(ident)
    _bits_equal(t["lam"], r["lam"], "lam")
    d = t["mu"] - r["mu"]                                               # rows are coarser than prices: one step earlier at most
    assert set(np.unique(d).tolist()) <= {0, 1}, np.unique(d)
    same = d == 0
    assert same.any()
    print("matches whose row walk closes at the same step: %.3f" % same.mean())
    for f in ("cycle_reward", "cycle_action"):
        _bits_equal(t[f][:, same], r[f][:, same], f)


def test_rows_against_play_greedy(trained):
    mb, tabs, _ = trained
    states = mb.states_numpy()
    mr, ma = mb.play_greedy(iters=1, state0=states[None])
    out = mb.greedy_cycles(steps=mb.T, rows=True)
    for got, rows in ((mr[0], out["reward_rows"]), (ma[0], out["action_rows"])):
        want = rows[:mb.T].mean(axis=0)
        err = np.abs(got - want).max() / np.abs(want).max()
        print("play_greedy vs mean of the rows: %.3e" % err)
        assert np.allclose(got, want, rtol=1e-12, atol=0.0), err


# ------------------------------------------------------------------------------------------------ sentinels, invariances
def test_sentinels_touch_only_their_own_match(trained):
    mb, tabs, pol = trained
    rs = np.random.RandomState(31)
    M = 130
    seats, start = rs.randint(0, G, size=(2, M)), rs.randint(0, 441, size=M)
    clean = mb.greedy_cycles(seats=seats, start=start, steps=3, rows=True)
    bad_seats, bad_start = seats.copy(), start.copy()
    bad_seats[1, 5], bad_seats[0, 64], bad_start[17], bad_start[129] = G, -1, -1, 441
    hit = np.zeros(M, bool)
    hit[[5, 64, 17, 129]] = True
    out = _check(mb, tabs, pol, bad_seats, bad_start, steps=3, strangers=False)
    assert (out["mu"][hit] == -1).all() and (out["lam"][hit] == 0).all() and (out["cycle_start"][hit] == -1).all()
    assert not out["cycle_reward"][:, hit].any() and not out["reward_rows"][:, :, hit].any()
    for f in OUT + ROWS:
        _bits_equal(out[f][..., ~hit], clean[f][..., ~hit], f)


def test_nothing_of_the_batch_is_written_and_halves_and_given_policy(trained):
    import torch
    from th_rl_amd import tuple_play as tp
    mb, tabs, pol = trained
    before = [mb.q.clone(), mb.counter.clone(), mb.state.clone(), mb.nn[1].params.clone()]
    rs = np.random.RandomState(41)
    seats, start = rs.randint(0, G, size=(2, 210)), rs.randint(0, 441, size=210)
    given = tp.extract(mb)
    whole = mb.greedy_cycles(seats=seats, start=start, steps=3, rows=True)
    again = mb.greedy_cycles(seats=seats, start=start, steps=3, rows=True, tuple_policy=given)
    halves = [mb.greedy_cycles(seats=seats[:, s], start=start[s], steps=3, rows=True, tuple_policy=given)
              for s in (slice(0, 105), slice(105, 210))]
    for f in OUT + ROWS:
        _bits_equal(again[f], whole[f], f)
        _bits_equal(np.concatenate([h[f] for h in halves], axis=-1), whole[f], f)
    assert np.array_equal(given.cpu().numpy().view(np.uint16), pol)
    for a, b in zip(before, [mb.q, mb.counter, mb.state, mb.nn[1].params]):
        assert torch.equal(a, b)
    both = mb.greedy_cycles(seats=[seats, seats[::-1].copy()], start=start)       # a list of rounds
    assert both["mu"].shape == (2, 210) and np.array_equal(both["mu"][0], whole["mu"])


# ------------------------------------------------------------------------------------------------ trainer
def test_train_one_greedy_cycles_artefacts(tmp_path):
    from th_rl_amd import trainer, tuple_play as tp, utils
    from th_rl_amd.crossplay import pairings
    from th_rl_amd.mixed import MixedGameBatch
    n = 64
    cfg = dict(MIXED, environment=dict(ENV, max_steps=20),
               training={"epochs": 30, "print_freq": 500, "seed": 19, "n_games": n,
                         "greedy_cycles": {"rounds": 2, "steps": 4}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "greedy_cycles.json"))
    assert desc["T"] == 441 and desc["options"]["rounds_played"] == 3 and desc["options"]["horizon_used"] == 442
    assert len(desc["self_play"]) == 1 and desc["self_play"][0]["matches"] + desc["self_play"][0]["no_start"] == n
    assert desc["self_play"][0]["no_start"] == 0 and desc["self_play"][0]["cycles"] == n
    assert len(desc["summary"]) == 1 and "retained" in desc["summary"][0] and len(desc["summary"][0]["seat_gain"]) == 2
    games = tp.load_games(str(exp))
    assert games["seats"].shape == (3, 2, n) and np.load(exp / "gcyc_cycle.npy").shape == (3, 3, n)
    # equal to the batch method on the saved batch
    mb = MixedGameBatch(dict(MIXED, environment=dict(ENV, max_steps=20)), n_games=n).load(str(exp / "batch.pt"))
    rounds = [tp.identity(2, n)] + pairings(np.zeros(n, int), 1, "rotate", 2, "own", 0, 2)
    direct = mb.greedy_cycles(seats=rounds)
    for f in OUT + ("start",):
        _bits_equal(games[f], direct[f], f)
    assert np.array_equal(games["seats"], np.stack(rounds))
    for r in range(3):
        df = utils.greedy_cycle_games(str(exp), r)
        assert df.index.tolist() == list(range(n)) and df["seat_1"].tolist() == rounds[r][1].tolist()
        assert df["lam"].tolist() == direct["lam"][r].tolist() and df["mu"].tolist() == direct["mu"][r].tolist()
        _bits_equal(df["cycle_reward_1"].to_numpy(), direct["cycle_reward"][r, 1], "cycle_reward")
    own, cross = utils.greedy_cycle_summary(str(exp))
    assert len(own) == 1 and len(cross) == 1 and own["matches"][0] == n and "seat_gain_1" in cross
    with pytest.raises(KeyError):
        utils.greedy_cycle_games(str(exp), 3)


def test_refusals_before_training_and_the_old_methods_still_raise(tmp_path):
    from th_rl_amd import launch, trainer
    from th_rl_amd._lib import ThrlError
    (tmp_path / "cac.json").write_text(json.dumps(dict(CAC, training={"epochs": 2, "n_games": 4, "greedy_cycles": True})))
    with pytest.raises(ValueError, match="continuous"):
        trainer.train_one(str(tmp_path / "run"), str(tmp_path / "cac.json"))
    assert not (tmp_path / "run" / "log.csv").exists()
    (tmp_path / "l.json").write_text(json.dumps(dict(MIXED, training={"epochs": 2, "n_games": 8, "greedy_cycles": True})))
    with pytest.raises(ValueError, match="greedy_cycles"):
        launch.launch(str(tmp_path / "l.json"), str(tmp_path / "out"), gpus=2)
    assert not (tmp_path / "out").exists()
    mb = _mixed(MIXED, n_games=8)
    seats = np.zeros((2, 8), np.int32)
    for call in (lambda: mb.deviation(), lambda: mb.equilibrium(), lambda: mb.crossplay(seats),
                 lambda: mb.attractors(), lambda: mb.stationary()):
        with pytest.raises(ThrlError, match="follow-up"):
            call()
    mb.greedy_cycles(start=np.zeros(8, np.int32))                       # the new name runs
