"""Deviation analysis on the device (thrl_deviation, GameBatch.deviation, training.deviation): every output bit-equal
to the numpy mirror (tests/deviation_mirror.py) on fresh and trained tables, f32 and f64, individual grids, the
direct path, a gamma sweep, both deviation modes, every deviator, given and default start prices; hand-built
known answers; and the invariances (learning state untouched, halves, tau-chunks, group statistics, MixedGameBatch,
the trainer's artefacts, a sharded launch)."""
import json
import os

import numpy as np
import pytest

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
# 3,001 rows: the window of reachable rows (about 1,200 per agent) does not fit the LDS budget -> direct path
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}
FIELDS = ("mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev", "cycle_reward", "cycle_action", "gain",
          "reward_rows", "action_rows")


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _check(gb, config, state0=None, gamma=None, **kw):
    out = gb.deviation(rows=True, state0=state0, **kw)
    s0 = gb.states_numpy() if state0 is None else state0
    ref = M.analyse(config, gb.tables_numpy(), s0, gamma=gamma, **kw)
    for f in FIELDS:
        _bits_equal(out[f], ref[f], f)
    assert out["horizon"] == ref["horizon"]
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
    gb = _batch(TWO, 384, dtype, seed=11, episodes=episodes)
    out = _check(gb, TWO, deviator=0, steps=12, dev_len=1)
    if episodes == 0:
        assert out["lam"].max() > 1                       # fresh tables: long cycles
    rs = np.random.RandomState(2)
    s0 = rs.uniform(0, 10, gb.G)
    for d in (0, 1):
        _check(gb, TWO, state0=s0, deviator=d, steps=10, dev_len=3)
        _check(gb, TWO, deviator=d, steps=6, dev_len=3, action=17)
        _check(gb, TWO, state0=s0, deviator=d, steps=5, dev_len=1, action=0)


def test_three_agents_individual_grids():
    gb = _batch(THREE, 256, seed=5, episodes=50)
    for d in range(3):
        _check(gb, THREE, deviator=d, steps=9, dev_len=2)
    _check(gb, THREE, state0=np.linspace(0.0, 10.0, 256), deviator=1, steps=4, action=3)


def test_direct_path_matches_mirror():
    gb = _batch(BIG, 128, seed=6, episodes=20)
    _check(gb, BIG, deviator=1, steps=8, dev_len=1)
    _check(gb, BIG, deviator=0, steps=8, dev_len=2, action=5, state0=np.linspace(0.5, 9.5, 128))


# Three agents on every path of the plan (k_deviation<.., 8>): the staged policy in one byte, in two bytes (257 actions
# on 12 states: the windows still fit the LDS budget), and the direct path (1,000 states each: they do not)
_A3 = [dict(AG, actions=7, states=30, action_range=[0.1, 0.5]), dict(AG, actions=11, states=30, action_range=[0.2, 0.4], gamma=0.9),
       dict(AG, actions=5, states=40, action_range=[0.0, 0.3])]
THREE_PATHS = {
    "one-byte": {"agents": _A3, "environment": dict(ENV, nplayers=3, max_steps=40)},
    "two-byte": {"agents": [dict(_A3[0], actions=257, states=12)] + _A3[1:], "environment": dict(ENV, nplayers=3, max_steps=40)},
    "direct": {"agents": [dict(a, states=1000) for a in _A3], "environment": dict(ENV, nplayers=3, max_steps=40)},
}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", list(THREE_PATHS))
def test_three_agents_on_every_path(name, dtype):
    config, G = THREE_PATHS[name], 300                      # a full block of 256 lanes and a partial one
    gb = _batch(config, G, dtype, seed=9)
    _check(gb, config, deviator=0, steps=6, dev_len=2)
    # a horizon of 3: games whose cycle closes later report mu = 3, lam = 0, before and after the deviation
    out = _check(gb, config, deviator=2, steps=5, dev_len=1, action=1, horizon=3, state0=np.linspace(0.0, 10.0, G))
    assert (out["lam"] == 0).any() and (out["mu"][out["lam"] == 0] == 3).all()


def test_gamma_sweep_discounts_with_the_games_gamma():
    G = 256
    gam = np.array([[0.35, 0.9, 0.95, 0.5][g % 4] for g in range(G)])
    gb = _batch(TWO, G, seed=8, episodes=100, sweep={"gamma": gam})
    for d in (0, 1):
        _check(gb, TWO, gamma=gam, deviator=d, steps=16, dev_len=2)


# ------------------------------------------------------------------------------------------------ known answers
def _known(policy, state0, **kw):
    from th_rl_amd.batched import GameBatch
    G = len(state0)
    gb = GameBatch(M.KNOWN, n_games=G, dtype="float64").set_tables(M.one_hot_tables(policy, G), state0)
    return gb.deviation(rows=True, **kw)


def test_known_punishment_returns():
    o = _known(M.PUNISH_2, [5.0], steps=5, dev_len=1, action=2)
    assert (o["mu"][0], o["lam"][0], o["mu_post"][0], o["lam_post"][0], o["ret_step"][0], o["act_dev"][0]) == (0, 1, 2, 1, 3, 2)
    assert o["gain"][0] == -6.25 and o["gain"][0] < 0
    assert o["cycle_reward"][:, 0].tolist() == [12.5, 12.5]
    assert o["reward_rows"][:, :, 0].tolist() == [[12.5, 6.25], [0, 0], [12.5, 12.5], [12.5, 12.5], [12.5, 12.5]]


def test_known_grim_trigger_never_returns():
    o = _known(M.GRIM, [5.0], steps=5, dev_len=1, action=2)
    assert (o["lam"][0], o["ret_step"][0], o["mu_post"][0], o["lam_post"][0]) == (1, -1, 1, 1)
    assert o["gain"][0] == -11.71875


def test_known_two_cycle_and_horizon():
    o = _known(M.CYCLE_2, [5.0, 10.0], steps=4, action=2)
    assert o["mu"].tolist() == [0, 1] and o["lam"].tolist() == [2, 2]
    assert o["cycle_reward"].tolist() == [[6.25, 6.25]] * 2 and o["cycle_action"].tolist() == [[0.375, 0.375]] * 2
    short = _known(M.CYCLE_2, [10.0], steps=4, action=2, horizon=2)
    assert (short["mu"][0], short["lam"][0], short["ret_step"][0]) == (2, 0, -1)
    enough = _known(M.CYCLE_2, [10.0], steps=4, action=2, horizon=3)
    assert (enough["mu"][0], enough["lam"][0]) == (1, 2)


# ------------------------------------------------------------------------------------------------ invariances
def test_learning_state_untouched_and_halves_equal_full():
    from th_rl_amd.batched import GameBatch
    G = 300
    gb = _batch(TWO, G, seed=12, episodes=40)
    before = (gb.tables_numpy().copy(), gb.counters_numpy().copy(), gb.states_numpy().copy(), list(gb.eps), gb.episode)
    full = gb.deviation(deviator=1, steps=10, dev_len=2, rows=True)
    after = (gb.tables_numpy(), gb.counters_numpy(), gb.states_numpy(), list(gb.eps), gb.episode)
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    q, s = before[0], before[2]
    for lo, hi in ((0, 137), (137, G)):
        h = GameBatch(TWO, n_games=hi - lo, seed=12, game_offset=lo).set_tables(q[lo:hi], s[lo:hi])
        part = h.deviation(deviator=1, steps=10, dev_len=2, rows=True)
        for f in FIELDS:
            _bits_equal(part[f], full[f][..., lo:hi], f)


def test_chunked_rows_and_group_stats():
    from th_rl_amd.group_stats import GroupSpec, reduce_host, resolve_ranges
    G = 256
    gb = _batch(TWO, G, seed=13, episodes=60)
    one = gb.deviation(deviator=0, steps=20, rows=True)
    chunked = gb.deviation(deviator=0, steps=20, rows=True, budget=8 * 2 * G * 3)       # 3 periods per chunk
    for f in FIELDS:
        _bits_equal(chunked[f], one[f], f)
    ids = np.arange(G) % 3
    spec = GroupSpec(2, ids, 3, resolve_ranges(TWO), bins=64)
    st = gb.deviation(deviator=0, steps=20, group_stats=spec, budget=8 * 2 * G * 7)
    assert "reward_rows" not in st
    raw = reduce_host(one["reward_rows"], one["action_rows"], ids, 3, spec.describe())
    for k in ("hist", "sums", "minmax"):
        assert np.array_equal(np.asarray(st["group_stats"][k]).view(np.uint8), np.asarray(raw[k]).view(np.uint8)), k


def test_mixed_batch_equals_game_batch():
    from th_rl_amd.mixed import MixedGameBatch
    from th_rl_amd._lib import ThrlError
    G = 128
    for dtype in ("float32", "float64"):
        gb = _batch(TWO, G, dtype, seed=14, episodes=30)
        mb = MixedGameBatch(TWO, n_games=G, dtype=dtype).set_tables(gb.tables_numpy(), gb.states_numpy())
        a = gb.deviation(deviator=1, steps=8, dev_len=2, rows=True)
        b = mb.deviation(deviator=1, steps=8, dev_len=2, rows=True)
        for f in FIELDS:
            _bits_equal(b[f], a[f], f)
    mx = MixedGameBatch(MIXED, n_games=8).init_tables()
    with pytest.raises(ThrlError, match="follow-up"):
        mx.deviation()


# ------------------------------------------------------------------------------------------------ trainer, launch
def test_train_one_deviation_artefacts(tmp_path):
    from th_rl_amd import trainer, utils
    G = 512
    sw = {"gamma": [[0.5, 0.9, 0.95, 0.35][g % 4] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 30, "print_freq": 500, "seed": 21, "n_games": G, "sweep": sw,
                              "group_stats": {"bins": 64, "histograms": True},
                              "deviation": {"steps": 12, "dev_len": 2}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "deviation.json"))
    assert desc["options"]["agents"] == [0, 1] and desc["options"]["horizon_used"] == 442
    assert [(r["group"], r["deviator"]) for r in desc["summary"]] == [(k, d) for d in (0, 1) for k in range(4)]
    assert np.load(exp / "dev_cycle.npy").shape == (2, G) and np.load(exp / "dev_cycle.npy").dtype == np.int32
    assert np.load(exp / "dev_cycle_reward.npy").shape == (2, G)
    # the artefacts are those of GameBatch.deviation on the trained batch
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(TWO, n_games=G, sweep=sw).load(str(exp / "batch.pt"))
    for d in (0, 1):
        o = gb.deviation(deviator=d, steps=12, dev_len=2, rows=True)
        post = np.load(exp / ("dev%d_post.npy" % d))
        assert post.shape == (4, G) and post.dtype == np.int32
        _bits_equal(post, np.stack([o["mu_post"], o["lam_post"], o["ret_step"], o["act_dev"]]), "post")
        _bits_equal(np.load(exp / ("dev%d_gain.npy" % d)), o["gain"], "gain")
        assert np.load(exp / ("dev%d_mean.npy" % d)).shape == (12, 4, 5)
        games = utils.deviation_games(str(exp), d)
        assert games["gain"].tolist() == o["gain"].tolist()
    _bits_equal(np.load(exp / "dev_cycle.npy"), np.stack([o["mu"], o["lam"]]), "cycle")
    df = utils.deviation_summary(str(exp))
    assert len(df) == 8 and df["games"].tolist() == [G // 4] * 8
    q = utils.group_quantiles(str(exp), 1, "total", prefix="dev0")
    assert len(q) == 12 and "Nash" in q.columns


def test_sharded_launch_deviation_equal_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 101
    sw = {"gamma": [[0.35, 0.9, 0.95][g % 3] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "sweep": sw,
                              "group_stats": {"bins": 32, "histograms": True},
                              "deviation": {"steps": 6, "dev_len": 1}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    assert json.load(open(tmp_path / "one" / "deviation.json")) == json.load(open(tmp_path / "two" / "deviation.json"))
    for d in (0, 1):
        a, b = utils.deviation_games(str(tmp_path / "one"), d), utils.deviation_games(str(tmp_path / "two"), d)
        assert a.index.tolist() == b.index.tolist() == list(range(G))
        for c in a.columns:
            _bits_equal(a[c].to_numpy(), b[c].to_numpy(), c)
        for f in ("sums", "hist", "min", "max", "quantiles"):
            x = np.load(tmp_path / "one" / ("dev%d_%s.npy" % (d, f)))
            y = np.load(tmp_path / "two" / ("dev%d_%s.npy" % (d, f)))
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (d, f)
