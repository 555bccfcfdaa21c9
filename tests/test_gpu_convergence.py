"""Convergence tracking on the device (thrl_policy_track, Tracker, training.convergence): every per-game array
bit-equal to the numpy mirror (tests/convergence_mirror.py) on planted tables and during training on every episode
kernel, f32 and f64, the staged and the direct path; the learning state untouched; shard invariance; the early stop;
resume; and the deviation analysis at convergence."""
import json
import os

import numpy as np
import pandas
import pytest

import convergence_mirror as M

pytestmark = pytest.mark.gpu

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
NOISE = dict(TWO, environment=dict(ENV, noise_prob=0.3))
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
# 3,001 rows x 21 actions x 2 agents: a game's block does not fit the LDS budget -> direct path
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
FIELDS = ("policy", "stable_since", "converged_at", "conv_since", "changes")


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.dtype.itemsize == b.dtype.itemsize, (what, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, np.flatnonzero(a.ravel() != b.ravel())[:5])


def _compare(tr, m, what=""):
    got, ref = tr.to_numpy(), m.arrays()
    for f in FIELDS + (("q_conv", "state_conv") if m.snapshot else ()):
        _bits_equal(got[f], ref[f], "%s %s" % (what, f))
    assert tr.converged() == m.n_converged, what


def _mirror(gb, window, snapshot=False):
    return M.Mirror(gb.tables_numpy(), gb.shapes, gb.offsets, gb.episode, window, state=gb.states_numpy(),
                    snapshot=snapshot)


def _batch(config, G, dtype="float32", seed=3, **kw):
    from th_rl_amd.batched import GameBatch
    return GameBatch(config, n_games=G, dtype=dtype, seed=seed, **kw).init_tables()


def _planted(rs, G, stride, dtype):
    return rs.randint(0, 4, (G, stride)).astype(dtype)          # four values: ties in most rows


# ------------------------------------------------------------------------------------------------ kernel vs mirror
@pytest.mark.parametrize("config,G,dtype", [(TWO, 5000, "float32"), (TWO, 3000, "float64"), (THREE, 700, "float32"),
                                            (BIG, 300, "float32"), (BIG, 200, "float64")])
def test_kernel_matches_mirror_on_planted_tables(config, G, dtype):
    import torch
    rs = np.random.RandomState(5)
    gb = _batch(config, G, dtype)
    q = _planted(rs, G, gb.stride, dtype)
    st = rs.rand(G) * 10
    gb.set_tables(q, st)
    gb.episode = 7
    tr = gb.track_convergence(window=3, every=1, snapshot=True)
    m = _mirror(gb, 3, snapshot=True)
    _compare(tr, m, "baseline")
    for k, e in enumerate((8, 9, 10, 11, 12, 13, 15, 16)):
        # plant changes: a few games get new maxima in one row of one agent, some of them reverted later
        games = rs.choice(G, size=max(1, G // (5 + k)), replace=False)
        for g in games:
            i = rs.randint(gb.N)
            r, a = gb.shapes[i]
            row = rs.randint(r)
            o = gb.offsets[i] + row * a
            q[g, o:o + a] = rs.randint(0, 4, a)
        for g in range(G // 10):        # restless games: a new greedy action at every check, never converge
            i = rs.randint(gb.N)
            r, a = gb.shapes[i]
            o = gb.offsets[i] + rs.randint(r) * a
            cur = int(np.argmax(q[g, o:o + a]))
            q[g, o:o + a] = 0
            q[g, o + (cur + 1) % a] = 5
        st = rs.rand(G) * 10
        gb.q.copy_(torch.from_numpy(q))
        gb.state.copy_(torch.from_numpy(st))
        gb.episode = e
        n = tr.check()
        assert n == m.check(q, e, state=st)
        _compare(tr, m, "check at %d" % e)
    assert 0 < m.n_converged < G
    assert np.array_equal(gb.tables_numpy().view(np.uint8), q.view(np.uint8))      # q is read only


def test_kernel_without_snapshot_or_count():
    from th_rl_amd import _lib
    import ctypes
    rs = np.random.RandomState(8)
    gb = _batch(TWO, 1000)
    q = _planted(rs, 1000, gb.stride, np.float32)
    gb.set_tables(q, np.zeros(1000))
    tr = gb.track_convergence(window=1, every=1)
    m = _mirror(gb, 1)
    gb.episode = 1
    a = _lib.PolicyTrackArgs()           # n_converged NULL: the arrays still update
    a.n_games, a.flags, a.episode, a.window = 1000, 0, 1, 1
    for f in FIELDS:
        setattr(a, f, getattr(tr, f).data_ptr())
    _lib.check(gb.L.thrl_policy_track(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(a), gb._stream()), "track")
    m.check(q, 1)
    got = tr.to_numpy()
    for f in FIELDS:
        _bits_equal(got[f], m.arrays()[f], f)
    assert tr.converged() == 0 and (got["converged_at"] == 1).all()


# ------------------------------------------------------------------------------------------------ during training
def _track_training(gb, every, window, checks):
    from th_rl_amd.batched import GameBatch
    tr = gb.track_convergence(window=window, every=every)
    m = _mirror(gb, window)
    for _ in range(checks):
        if isinstance(gb, GameBatch):
            gb.run(every, logs=False)
        else:
            gb.run(every, per_game_logs=False)
        assert tr.check() == m.check(gb.tables_numpy(), gb.episode)
        _compare(tr, m, "episode %d" % gb.episode)
    return tr, m


@pytest.mark.parametrize("every", [1, 5])
def test_training_wave_kernel_matches_mirror(every):
    gb = _batch(TWO, 4096, seed=21)
    tr, m = _track_training(gb, every, 2 * every, 24 // every)
    assert gb.last_kernel == "wave"
    assert m.changes.sum() > 0


@pytest.mark.parametrize("case", ["noise", "sweep", "tuple", "generic", "f64"])
def test_training_other_kernels_match_mirror(case):
    G = 2048
    if case == "noise":
        gb = _batch(NOISE, G, seed=4)
    elif case == "sweep":
        gb = _batch(TWO, G, seed=4, sweep={"gamma": [[0.35, 0.9, 0.95][g % 3] for g in range(G)],
                                           "alpha": np.linspace(0.05, 0.5, G)})
    elif case == "tuple":
        gb = _batch(THREE, G, seed=4)
    elif case == "generic":
        gb = _batch(TWO, 512, seed=4, kernel="generic")
    else:
        gb = _batch(TWO, 1024, dtype="float64", seed=4)
    _track_training(gb, 2, 4, 8)
    if case == "generic":
        assert gb.last_kernel == "generic"
    if case == "tuple":
        assert gb.last_kernel == "tuple"


def test_mixed_batch_one_game_f64_matches_mirror():
    from th_rl_amd.mixed import MixedGameBatch
    gb = MixedGameBatch(TWO, n_games=1, dtype="float64", seed=9).init_tables()
    tr, m = _track_training(gb, 1, 3, 30)
    assert m.changes[0] > 0


# ------------------------------------------------------------------------------------------------ invariances
def _state(gb):
    return (gb.tables_numpy().copy(), gb.counters_numpy().copy(), gb.states_numpy().copy(), list(gb.eps), gb.episode)


def test_learning_state_untouched():
    G, cuts = 2048, (4, 4, 4, 8)
    runs = {}
    for tracked in (True, False):
        gb = _batch(TWO, G, seed=31)
        tr = gb.track_convergence(window=4, every=4) if tracked else None
        logs = []
        for k in cuts:
            out = gb.run(k, per_game_logs=True)
            logs.append((out["reward_log"], out["action_log"], out["game_reward_log"], out["game_action_log"]))
            if tr is not None:
                tr.check()
        runs[tracked] = (_state(gb), logs)
    (sa, la), (sb, lb) = runs[True], runs[False]
    for x, y in zip(sa, sb):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    for a, b in zip(la, lb):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # against one uncut launch: tables, counters, state and epsilon identical, the mean logs to the split tolerance
    gb = _batch(TWO, G, seed=31)
    out = gb.run(sum(cuts), per_game_logs=True)
    sc = _state(gb)
    for x, y in zip(sa, sc):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        else:
            assert x == y
    np.testing.assert_allclose(np.concatenate([l[0] for l in la]), out["reward_log"], rtol=1e-12)
    np.testing.assert_allclose(np.concatenate([l[1] for l in la]), out["action_log"], rtol=1e-12)


def test_game_halves_equal_the_whole():
    from th_rl_amd.batched import GameBatch
    G = 1000
    whole = _batch(TWO, G, seed=41)
    parts = [GameBatch(TWO, n_games=hi - lo, seed=41, game_offset=lo).init_tables() for lo, hi in ((0, 371), (371, G))]
    trs = [b.track_convergence(window=3, every=3) for b in [whole] + parts]
    for _ in range(6):
        for b, t in zip([whole] + parts, trs):
            b.run(3, logs=False)
            t.check()
    w = trs[0].to_numpy()
    halves = [t.to_numpy() for t in trs[1:]]
    for f in FIELDS:
        _bits_equal(w[f], np.concatenate([h[f] for h in halves]), f)
    assert trs[0].converged() == trs[1].converged() + trs[2].converged()


def _train(tmp_path, name, config, **training):
    from th_rl_amd import trainer
    cfg = dict(config, training=training)
    d = tmp_path / name
    d.mkdir(parents=True, exist_ok=True)
    (d / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(d / "out"), str(d / "c.json"))
    return d / "out"


def _conv_arrays(d):
    return {f: np.load(os.path.join(str(d), f)) for f in ("conv_episode.npy", "conv_since.npy", "conv_stable_since.npy",
                                                         "conv_changes.npy")}


def test_early_stop_with_alpha_zero(tmp_path):
    frozen = {"agents": [dict(AG, alpha=0.0), dict(AG, alpha=0.0)], "environment": dict(ENV)}
    G = 300
    base = dict(epochs=40, print_freq=4, seed=5, n_games=G, game_logs=True, group_stats={"bins": 16})
    out = _train(tmp_path, "stop", frozen, convergence={"window": 10, "every": 4, "stop": 1.0}, **base)
    desc = json.load(open(out / "convergence.json"))
    assert desc["stopped_early"] and desc["episodes_run"] == 12 and desc["every_used"] == 4
    assert desc["summary"][0]["converged"] == G and desc["summary"][0]["converged_at_q50"] == 12
    a = _conv_arrays(out)
    assert (a["conv_episode.npy"] == 12).all() and (a["conv_since.npy"] == 0).all()
    assert (a["conv_changes.npy"] == 0).all()
    assert len(pandas.read_csv(out / "log.csv", header=[0, 1])) == 12
    assert np.load(out / "game_rewards.npy").shape == (12, 2, G)
    assert np.load(out / "game_actions.npy").shape == (12, 2, G)
    for f in ("mean", "std", "min", "max", "quantiles", "sums"):
        assert np.load(out / ("group_%s.npy" % f)).shape[0] == 12, f
    # with stop: null every epoch runs and the artefacts are the untracked run's (same launches: print_freq = every)
    full = _train(tmp_path, "full", frozen, convergence={"window": 10, "every": 4}, **base)
    plain = _train(tmp_path, "plain", frozen, **base)
    assert not json.load(open(full / "convergence.json"))["stopped_early"]
    for name in ("log.csv", "0.npy", "1.npy", "0_counter.npy", "game_rewards.npy", "group_mean.npy", "group_sums.npy"):
        assert (full / name).read_bytes() == (plain / name).read_bytes(), name
    import torch
    x, y = torch.load(full / "batch.pt", weights_only=True), torch.load(plain / "batch.pt", weights_only=True)
    for k in ("q", "counter", "state"):
        assert torch.equal(x[k], y[k]), k
    assert x["eps"] == y["eps"] and x["episode"] == y["episode"] == 40


def test_tracked_training_artefacts_equal_untracked(tmp_path):
    base = dict(epochs=30, print_freq=5, seed=6, n_games=512)
    a = _train(tmp_path, "a", TWO, convergence={"window": 10, "every": 5}, **base)
    b = _train(tmp_path, "b", TWO, **base)
    for name in ("log.csv", "0.npy", "1.npy", "0_counter.npy", "1_counter.npy"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert not os.path.exists(b / "convergence.json")


def test_resume_equals_uninterrupted(tmp_path):
    base = dict(print_freq=4, seed=8, n_games=700)
    conv = {"window": 8, "every": 4, "snapshot": True}
    whole = _train(tmp_path, "whole", TWO, epochs=32, convergence=conv, **base)
    first = _train(tmp_path, "first", TWO, epochs=16, convergence=conv, **base)
    second = _train(tmp_path, "second", TWO, epochs=16, convergence=conv, resume=str(first / "batch.pt"), **base)
    a, b = _conv_arrays(whole), _conv_arrays(second)
    for f in a:
        _bits_equal(a[f], b[f], f)
    import torch
    x, y = torch.load(whole / "convergence.pt", weights_only=True), torch.load(second / "convergence.pt", weights_only=True)
    for k in ("policy", "q_conv", "state_conv", "n_converged"):
        assert torch.equal(x[k], y[k]), k


def test_deviation_at_convergence(tmp_path):
    from th_rl_amd.batched import GameBatch
    import torch
    G = 400
    sw = {"alpha": [0.0 if g % 2 == 0 else 0.1 for g in range(G)]}      # the even games converge at episode 4
    out = _train(tmp_path, "dev", TWO, epochs=24, print_freq=4, seed=9, n_games=G, sweep=sw,
                 convergence={"window": 4, "every": 4, "snapshot": True},
                 deviation={"agents": [0], "steps": 6, "tables": "converged"})
    desc = json.load(open(out / "deviation.json"))
    assert desc["options"]["tables"] == "converged"
    ca = np.load(out / "conv_episode.npy")
    assert 0 < (ca >= 0).sum() < G
    sd = torch.load(out / "convergence.pt", weights_only=True)
    gb = GameBatch(TWO, n_games=G, seed=9).load(str(out / "batch.pt"))
    m = torch.from_numpy(ca >= 0)
    q = torch.where(m[:, None], sd["q_conv"], gb.q.cpu())
    s = torch.where(m, sd["state_conv"], gb.state.cpu())
    gb.set_tables(q.numpy(), s.numpy(), counter=gb.counters_numpy())
    r = gb.deviation(deviator=0, steps=6)
    cyc = np.load(out / "dev_cycle.npy")
    assert np.array_equal(cyc, np.stack([r["mu"], r["lam"]]).astype(np.int32))
    assert np.array_equal(np.load(out / "dev0_gain.npy").view(np.uint64), r["gain"].view(np.uint64))
    assert np.array_equal(np.load(out / "dev_cycle_reward.npy").view(np.uint64), r["cycle_reward"].view(np.uint64))
    post = np.load(out / "dev0_post.npy")
    assert np.array_equal(post, np.stack([r["mu_post"], r["lam_post"], r["ret_step"], r["act_dev"]]).astype(np.int32))
    # the analysed start prices are the converged games' states at episode 4, not the final ones
    fin = GameBatch(TWO, n_games=G, seed=9).load(str(out / "batch.pt"))
    assert (ca[::2] == 4).all() and not np.array_equal(fin.states_numpy()[::2], s.numpy()[::2])


def test_sharded_launch_with_stop_equals_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 101
    # the even games do not learn (alpha 0) and converge at the first check >= W: the stop at 0.2 comes there
    sw = {"alpha": [0.0 if g % 2 == 0 else 0.1 for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 40, "print_freq": 500, "seed": 17, "n_games": G, "sweep": sw,
                              "convergence": {"window": 6, "every": 2, "stop": 0.2}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    one = json.load(open(tmp_path / "one" / "convergence.json"))
    two = json.load(open(tmp_path / "two" / "convergence.json"))
    assert one == two
    assert one["stopped_early"] and one["episodes_run"] < 40
    a, b = _conv_arrays(tmp_path / "one"), _conv_arrays(tmp_path / "two")
    for f in a:
        _bits_equal(a[f], b[f], f)
    x, y = utils.convergence_games(str(tmp_path / "one")), utils.convergence_games(str(tmp_path / "two" / "shard0"))
    assert y.index.tolist() == list(range(len(y)))
    la = pandas.read_csv(tmp_path / "one" / "log.csv", header=[0, 1])
    lb = pandas.read_csv(tmp_path / "two" / "log.csv", header=[0, 1])
    assert len(la) == len(lb) == one["episodes_run"]
    np.testing.assert_allclose(la.to_numpy(), lb.to_numpy(), rtol=1e-12)
