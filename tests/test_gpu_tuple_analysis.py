"""The deviation test and the equilibrium check in tuple form on the device (thrl_tuple_deviation,
thrl_tuple_equilibrium, MixedGameBatch.greedy_deviation / greedy_equilibrium, training.greedy_deviation /
greedy_equilibrium): bit-equal to the numpy mirrors (tests/tuple_deviation_mirror.py, tests/tuple_equilibrium_mirror.py)
fed the device's extracted strategies; bit-equal to thrl_deviation / thrl_equilibrium on an all-QTable batch started on
its cycle, with no mirror in between; the edges of the tuple count and of the launch shape; the trainer's artefacts.

The networks get weights with kinks inside the price range (fresh ones are nearly constant in the price), the start
tuples are random, with -1 mixed in, and every game has its own gamma, one of them 0.  Every mirror test asserts that
its input is not degenerate: at least half of the games have a neural row with >= 2 distinct actions, at least a
quarter have a path with lam >= 1 and mu + lam > 1, and at least a quarter of the (game, agent) pairs need an
improvement round (iters >= 1).  The shares are printed by each test."""
import json

import numpy as np
import pytest

import tuple_deviation_mirror as DM
import tuple_equilibrium_mirror as EM

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
BIG = {"agents": [dict(AG, actions=128), dict(RF, actions=32)], "environment": dict(ENV)}          # T = 4096 exactly
WIDE = {"agents": [dict(AG, actions=129), dict(RF, actions=32)], "environment": dict(ENV)}         # 4128 tuples
CONFIGS = {"MIXED": (MIXED, 441), "AC": (AC, 105), "NN2": (NN2, 672), "THREE": (THREE, 385)}
G = 203                                                                 # no multiple of a wave or of the 256 games per block
DEV_INT = ("mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev")
DEV_OUT = DEV_INT + ("cycle_reward", "cycle_action", "gain")
ROWS = ("reward_rows", "action_rows")
EQ_OUT = ("mu", "lam", "iters", "n_diff_all", "n_diff_on", "loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on")
EQ_POL = ("br_policy", "v_opt", "v_pi")


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


def _gammas(n_agents, n_games, seed):
    """[N, G] in [0.5, 0.99], game 1 at gamma = 0 for every agent."""
    gam = np.random.RandomState(seed).uniform(0.5, 0.99, (n_agents, n_games))
    if n_games > 1:
        gam[:, 1] = 0.0
    return gam


def _mixed(config, n_games=G, dtype="float32", seed=3, weights_seed=1, sweep=True):
    from th_rl_amd import tuple_play as tp
    from th_rl_amd.mixed import MixedGameBatch
    gam = _gammas(len(config["agents"]), n_games, seed) if sweep else None
    mb = MixedGameBatch(config, n_games=n_games, dtype=dtype, seed=seed,
                        sweep={"gamma": gam} if sweep else None).init_tables()
    price = tp.tables(config)["price"]
    rs = np.random.RandomState(weights_seed)
    for i, rb in mb.nn.items():
        rb.set_params(_kinked_weights(rs, n_games, rb.A, rb.P, price.min(), price.max()))
    return mb, gam


def _starts(T, n_games, seed):
    """Random start tuples with -1 (and one T) mixed in."""
    rs = np.random.RandomState(seed)
    start = rs.randint(0, T, size=n_games).astype(np.int32)
    if n_games > 8:
        start[rs.choice(n_games, n_games // 8, replace=False)] = -1
        start[0], start[5] = 0, T
    return start


_CACHE = {}


def _case(name, episodes):
    """(batch, gammas, tables, strategies as numpy, as the device tensor, start tuples) of one config, built once."""
    from th_rl_amd import tuple_play as tp
    key = (name, episodes)
    if key not in _CACHE:
        config, T = CONFIGS[name]
        mb, gam = _mixed(config, seed=5 + episodes, weights_seed=2 + episodes)
        if episodes:
            mb.run(episodes, per_game_logs=False)
        given = tp.extract(mb)
        pol = given.cpu().numpy().view(np.uint16)
        assert pol.shape == (G, len(config["agents"]), T)
        varied = np.zeros(G, bool)
        for i in mb.nn:
            varied |= np.array([np.unique(r).size >= 2 for r in pol[:, i, :]])
        print("%s after %d episodes: games with a neural row of >= 2 distinct actions: %.3f" % (name, episodes, varied.mean()))
        assert varied.mean() >= 0.5, varied.mean()
        _CACHE[key] = (mb, gam, tp.tables(config), pol, given, _starts(T, G, 17 + episodes))
    return _CACHE[key]


def _path_share(ref, what):
    share = np.mean((ref["lam"] >= 1) & (ref["mu"] + ref["lam"] > 1))
    print("%s: games with lam >= 1 and mu + lam > 1: %.3f" % (what, share))
    assert share >= 0.25, share


# ------------------------------------------------------------------------------------------------ against the mirrors
@pytest.mark.parametrize("episodes", [0, 20])
@pytest.mark.parametrize("name", ["MIXED", "AC", "NN2", "THREE"])
def test_deviation_equals_mirror(name, episodes):
    mb, gam, tabs, pol, given, start = _case(name, episodes)
    N = mb.N
    for d, action, L in ((0, "best_response", 1), (N - 1, 1, 3), (N - 1, "best_response", 3)):
        out = mb.greedy_deviation(deviator=d, steps=7, dev_len=L, action=action, start=start, rows=True, tuple_policy=given)
        ref = DM.analyse(tabs, pol, start, deviator=d, steps=7, dev_len=L, action=-1 if action == "best_response" else action,
                         gamma=gam[d])
        _path_share(ref, "%s d=%d" % (name, d))
        for f in DEV_OUT + ROWS:
            _bits_equal(out[f], ref[f], "%s d=%d L=%d %s" % (name, d, L, f))
        assert out["horizon"] == ref["horizon"] and np.array_equal(out["start"], start)
        refused = (start < 0) | (start >= tabs["T"])
        assert refused.sum() >= G // 8 and (out["mu"][refused] == -1).all() and (out["act_dev"][refused] == -1).all()
        assert not out["reward_rows"][:, :, refused].any() and (out["mu"][~refused] >= 0).all()
        assert (out["ret_step"] >= 0).any() or (out["ret_step"][~refused] == -1).all()
    # the rows in two chunks with an uneven boundary (4 + 3), and with the strategies extracted by the call itself
    parts = mb.greedy_deviation(deviator=N - 1, steps=7, dev_len=3, start=start, rows=True, budget=8 * N * G * 4)
    for f in DEV_OUT + ROWS:
        _bits_equal(parts[f], out[f], f)
    # a short horizon: lam = 0 where the cycle closes later
    short = mb.greedy_deviation(deviator=0, steps=3, horizon=2, start=start, tuple_policy=given)
    ref = DM.analyse(tabs, pol, start, deviator=0, steps=3, horizon=2, gamma=gam[0])
    for f in DEV_OUT:
        _bits_equal(short[f], ref[f], "horizon 2 " + f)


@pytest.mark.parametrize("episodes", [0, 20])
@pytest.mark.parametrize("name", ["MIXED", "AC", "NN2", "THREE"])
def test_equilibrium_equals_mirror(name, episodes):
    mb, gam, tabs, pol, given, start = _case(name, episodes)
    out = mb.greedy_equilibrium(start=start, policies=True, tuple_policy=given)
    ref = EM.analyse(tabs, pol, start, gamma=gam, policies=True)
    _path_share(ref, name)
    share = np.mean(ref["iters"] >= 1)
    print("%s: (game, agent) pairs with iters >= 1: %.3f, largest iters %d" % (name, share, ref["iters"].max()))
    assert share >= 0.25, share
    for f in EQ_OUT + EQ_POL:
        _bits_equal(out[f], ref[f], "%s %s" % (name, f))
    assert out["n_states"] == tabs["T"] and out["agents"] == list(range(mb.N)) and np.array_equal(out["start"], start)
    refused = (start < 0) | (start >= tabs["T"])
    assert (out["mu"][refused] == -1).all() and np.isnan(out["loss_on"][:, refused]).all()
    assert not np.isnan(out["loss_all"]).any() and not out["nash"][refused].any()
    # gamma = 0 (game 1): one-period values, no doubling
    assert np.array_equal(out["v_pi"][0, 1], tabs["reward"][0][DM.greedy_map(tabs, pol[1])])
    # one agent alone leaves the other's outputs untouched (zeros of the runner's buffers)
    solo = mb.greedy_equilibrium(agents=[mb.N - 1], start=start, tuple_policy=given)
    for f in EQ_OUT[2:]:
        _bits_equal(solo[f][mb.N - 1], out[f][mb.N - 1], f)
        assert not solo[f][0].any()


# ------------------------------------------------------------------------------------------------ against the QTable kernels
def _row_states(config, price):
    """state(t) of thrl_equilibrium for a config whose agents share one grid: distinct rows in order of first occurrence."""
    a = config["agents"][0]
    row = np.clip(np.rint(price / float(a.get("max_state", 10)) * a["states"]), 0, a["states"]).astype(np.int64)
    ids, out = {}, np.zeros(row.size, np.int64)
    for t, r in enumerate(row):
        out[t] = ids.setdefault(int(r), len(ids))
    return out, len(ids)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_all_qtable_batch_against_the_row_kernels(dtype):
    from th_rl_amd import tuple_play as tp
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(TWO, n_games=G, dtype=dtype, seed=11).init_tables()
    gb.run(40, logs=False)
    tabs = tp.tables(TWO)
    given = tp.extract(gb)
    c = tp.run(gb, tuple_policy=given)["cycle_start"]
    assert (c >= 0).all()
    state0 = tabs["price"][c]
    for d, action, L in ((0, "best_response", 1), (1, 3, 3)):
        t = gb.greedy_deviation(deviator=d, steps=9, dev_len=L, action=action, start=c, rows=True, tuple_policy=given)
        r = gb.deviation(deviator=d, steps=9, dev_len=L, action=action, state0=state0, rows=True)
        assert not t["mu"].any() and not r["mu"].any()                  # both paths start on the cycle
        for f in ("lam", "cycle_reward", "cycle_action", "act_dev", "gain", "lam_post") + ROWS:
            _bits_equal(t[f], r[f], "d=%d %s" % (d, f))
        assert np.array_equal(t["ret_step"] < 0, r["ret_step"] < 0)
        diff = (t["ret_step"] - r["ret_step"])[r["ret_step"] >= 0]
        assert set(np.unique(diff).tolist()) <= {0, 1}, np.unique(diff)   # two tuples can share a row tuple
        print("d=%d: returned %.3f, of those one step later in tuple form %.3f, lam > 1: %.3f"
              % (d, np.mean(r["ret_step"] >= 0), diff.mean() if diff.size else 0.0, np.mean(r["lam"] > 1)))
    t = gb.greedy_equilibrium(start=c, policies=True, tuple_policy=given)
    r = gb.equilibrium(state0=state0, policies=True)
    assert not t["mu"].any() and not r["mu"].any()
    for f in ("lam", "iters", "n_diff_on", "loss_on", "loss_on_mean", "v_on", "loss_all"):
        _bits_equal(t[f], r[f], f)
    sid, S = _row_states(TWO, tabs["price"])
    assert S == r["n_states"] and t["n_states"] == 441
    for f in EQ_POL:
        _bits_equal(t[f], r[f][:, :, sid], f)
    print("pairs with iters >= 1: %.3f" % np.mean(r["iters"] >= 1))
    assert np.mean(r["iters"] >= 1) >= 0.25


# ------------------------------------------------------------------------------------------------ edges
def test_4096_tuples_exactly():
    from th_rl_amd import tuple_play as tp
    mb, gam = _mixed(BIG, n_games=5, seed=23, weights_seed=9)
    tabs = tp.tables(BIG)
    assert tabs["T"] == 4096
    given = tp.extract(mb)
    pol = given.cpu().numpy().view(np.uint16)
    start = np.array([0, 4095, 1234, -1, 4096], np.int32)
    out = mb.greedy_equilibrium(start=start, policies=True, tuple_policy=given)
    ref = EM.analyse(tabs, pol, start, gamma=gam, policies=True)
    print("T = 4096: iters %s" % ref["iters"].tolist())
    assert (ref["iters"] >= 1).any()
    for f in EQ_OUT + EQ_POL:
        _bits_equal(out[f], ref[f], f)
    dev = mb.greedy_deviation(deviator=0, steps=5, dev_len=2, start=start, rows=True, tuple_policy=given)
    ref = DM.analyse(tabs, pol, start, deviator=0, steps=5, dev_len=2, gamma=gam[0])
    for f in DEV_OUT + ROWS:
        _bits_equal(dev[f], ref[f], f)


def test_three_agents_with_tables_in_global_memory():
    """16 x 11 x 8 = 1,408 tuples of three agents: 2 N T doubles are past the deviation's LDS budget, so
    k_ta_deviation<global, 8> reads the reward and scaled tables from global memory."""
    from th_rl_amd import tuple_play as tp
    config = {"agents": [dict(THREE["agents"][0], actions=16), THREE["agents"][1], dict(THREE["agents"][2], actions=8)],
              "environment": THREE["environment"]}
    n = 300                                                             # a full block of 256 lanes and a partial one
    mb, gam = _mixed(config, n_games=n, seed=29, weights_seed=11)
    tabs = tp.tables(config)
    assert tabs["T"] == 1408 and 2 * 3 * tabs["T"] * 8 > 64 * 1024
    given = tp.extract(mb)
    pol = given.cpu().numpy().view(np.uint16)
    start = _starts(tabs["T"], n, 31)
    for d, horizon in ((0, None), (2, 2)):                              # horizon 2: lam = 0 where the cycle closes later
        kw = {} if horizon is None else {"horizon": horizon}
        dev = mb.greedy_deviation(deviator=d, steps=5, dev_len=2, start=start, rows=True, tuple_policy=given, **kw)
        ref = DM.analyse(tabs, pol, start, deviator=d, steps=5, dev_len=2, gamma=gam[d], **kw)
        for f in DEV_OUT + ROWS:
            _bits_equal(dev[f], ref[f], "d=%d %s" % (d, f))
    assert ((dev["lam"] == 0) & (dev["mu"] == 2)).any()


def test_one_game_halves_and_nothing_written():
    import torch
    from th_rl_amd import tuple_play as tp
    mb, gam, tabs, pol, given, start = _case("MIXED", 20)
    before = [mb.q.clone(), mb.counter.clone(), mb.state.clone(), mb.nn[1].params.clone(), given.clone()]
    whole_d = mb.greedy_deviation(deviator=1, steps=5, dev_len=2, start=start, rows=True, tuple_policy=given)
    whole_e = mb.greedy_equilibrium(start=start, policies=True, tuple_policy=given)
    for a, b in zip(before, [mb.q, mb.counter, mb.state, mb.nn[1].params, given]):
        assert torch.equal(a, b)
    # the same games launched in two halves of 101 and 102, and one game alone: a batch of their own each
    for lo, hi in ((0, 101), (101, 203), (7, 8)):
        part, _ = _mixed(MIXED, n_games=hi - lo, sweep=False)
        part.set_sweep({"gamma": gam[:, lo:hi]})
        sub = given[lo:hi].contiguous()
        d = part.greedy_deviation(deviator=1, steps=5, dev_len=2, start=start[lo:hi], rows=True, tuple_policy=sub)
        e = part.greedy_equilibrium(start=start[lo:hi], policies=True, tuple_policy=sub)
        for f in DEV_OUT + ROWS:
            _bits_equal(d[f], whole_d[f][..., lo:hi], f)
        for f in EQ_OUT:
            _bits_equal(e[f], whole_e[f][..., lo:hi], f)
        for f in EQ_POL:
            _bits_equal(e[f], whole_e[f][:, lo:hi], f)
    # the default start is the tuple of the batch's state
    dflt = mb.greedy_equilibrium(agents=[0])
    assert np.array_equal(dflt["start"], tp.start_tuples(mb, tabs).cpu().numpy()) and (dflt["start"] >= 0).all()
    assert (dflt["lam"] >= 1).all()


def test_refusals_and_the_old_methods_still_raise():
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.mixed import MixedGameBatch
    wide = MixedGameBatch(WIDE, n_games=4).init_tables()
    cac = MixedGameBatch(CAC, n_games=4).init_tables()
    for call in (wide.greedy_deviation, wide.greedy_equilibrium):
        with pytest.raises(ValueError, match="4096"):
            call(start=np.zeros(4, np.int32))
    for call in (cac.greedy_deviation, cac.greedy_equilibrium):
        with pytest.raises(ValueError, match="continuous"):
            call(start=np.zeros(4, np.int32))
    mb, _ = _mixed(MIXED, n_games=8, sweep=False)
    with pytest.raises(ThrlError, match="deviation analysis runs on QTable agents only.*follow-up on the mixed path's policy tables"):
        mb.deviation()
    with pytest.raises(ThrlError, match="the equilibrium check runs on QTable agents only.*follow-up on the mixed path's policy tables"):
        mb.equilibrium()
    # without a sweep the network's own gamma (0.995) discounts, not the placeholder table slot's
    out = mb.greedy_deviation(deviator=1, steps=4, start=np.zeros(8, np.int32))
    from th_rl_amd import tuple_play as tp
    ref = DM.analyse(tp.tables(MIXED), tp.extract(mb).cpu().numpy(), np.zeros(8, np.int32), deviator=1, steps=4, gamma=0.995)
    _bits_equal(out["gain"], ref["gain"], "gain")
    assert mb.greedy_equilibrium(start=np.zeros(8, np.int32))["iters"].min() >= 0


# ------------------------------------------------------------------------------------------------ trainer
def test_train_one_artefacts(tmp_path):
    from th_rl_amd import launch, trainer, tuple_analysis as ta, utils
    from th_rl_amd.mixed import MixedGameBatch
    n = 12
    base = dict(MIXED, environment=dict(ENV, max_steps=20))
    cfg = dict(base, training={"epochs": 20, "print_freq": 500, "seed": 19, "n_games": n,
                               "sweep": {"gamma": [0.6] * 6 + [0.9] * 6},
                               "greedy_deviation": {"steps": 6, "dev_len": 2}, "greedy_equilibrium": {"policies": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    dd = json.load(open(exp / "greedy_deviation.json"))
    ed = json.load(open(exp / "greedy_equilibrium.json"))
    assert dd["T"] == 441 and dd["options"]["horizon_used"] == 442 and dd["options"]["agents"] == [0, 1]
    assert len(dd["summary"]) == 4 and all(r["no_start"] == 0 and r["games"] == n // 2 for r in dd["summary"])
    assert ed["n_states"] == 441 and len(ed["summary"]) == 6 and ed["summary"][2]["collusive"] is not None
    assert np.load(exp / "gdev_cycle.npy").shape == (3, n) and np.load(exp / "gdev_cycle_reward.npy").shape == (2, n)
    for d in (0, 1):
        assert np.load(exp / ("gdev%d_post.npy" % d)).shape == (4, n) and np.load(exp / ("gdev%d_gain.npy" % d)).shape == (n,)
    assert np.load(exp / "geq_cycle.npy").shape == (3, n) and np.load(exp / "geq_iters.npy").shape == (2, n)
    assert np.load(exp / "geq_diff.npy").shape == (2, 2, n) and np.load(exp / "geq_loss.npy").shape == (4, 2, n)
    assert np.load(exp / "geq_value.npy").shape == (2, n) and np.load(exp / "geq_policy.npy").shape == (2, n, 441)
    assert np.load(exp / "geq_v_opt.npy").shape == (2, n, 441) and np.load(exp / "geq_v_pi.npy").dtype == np.float64
    # equal to the batch methods on the saved batch (the sweep comes back with it)
    mb = MixedGameBatch(base, n_games=n).load(str(exp / "batch.pt"))
    assert mb.sweep["gamma"].cpu().numpy()[0].tolist() == [0.6] * 6 + [0.9] * 6
    for d in (0, 1):
        direct = mb.greedy_deviation(deviator=d, steps=6, dev_len=2)
        saved = ta.load_deviation_games(str(exp), d)
        for f in DEV_OUT + ("start",):
            _bits_equal(saved[f], direct[f], f)
        df = utils.greedy_deviation_games(str(exp), d)
        assert df.index.tolist() == list(range(n)) and df["ret_step"].tolist() == direct["ret_step"].tolist()
        _bits_equal(df["gain"].to_numpy(), direct["gain"], "gain")
    direct = mb.greedy_equilibrium(policies=True)
    saved = ta.load_equilibrium_games(str(exp))
    for f in EQ_OUT + EQ_POL + ("start",):
        _bits_equal(saved[f], direct[f], f)
    df = utils.greedy_equilibrium_games(str(exp), 1)
    assert df["iters"].tolist() == direct["iters"][1].tolist() and df["nash"].tolist() == direct["nash"].tolist()
    ds, es = utils.greedy_deviation_summary(str(exp)), utils.greedy_equilibrium_summary(str(exp))
    assert len(ds) == 4 and "lam_1" in ds and ds["T"][0] == 441 and len(es) == 6 and es["n_states"][0] == 441
    with pytest.raises(KeyError):
        utils.greedy_deviation_games(str(tmp_path), 0)
    with pytest.raises(ValueError, match="greedy_deviation is not available under th_rl_amd.launch"):
        launch.check_launch_config(cfg)
    with pytest.raises(ValueError, match="greedy_equilibrium is not available under th_rl_amd.launch"):
        launch.check_launch_config(dict(base, training={"greedy_equilibrium": True}))
