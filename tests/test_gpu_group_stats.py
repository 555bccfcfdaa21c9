"""Per-group statistics on the device (thrl_group_stats, th_rl_amd.group_stats): the kernel against its numpy
restatement (group_stats.reduce_host, same float64 operations) bit for bit; every episode path's out["group_stats"]
against the reduction of the same run's per-game rows, with everything else identical to the run without it;
invariance to chunking and to sharding; the trainer's artefacts."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
NOISY = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV, noise_prob=0.05)}
CYCLE = {"agents": [dict(AG, min_memory=100), dict(AG, min_memory=100, alpha=0.3)], "environment": dict(ENV, max_steps=50)}
GRIDS = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=21, states=100, action_range=[0.2, 0.4], min_memory=10, alpha=0.3, gamma=0.9)],
         "environment": dict(ENV, max_steps=40)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}


def _eq(a, b):
    for k in ("hist", "sums", "minmax"):
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape, k
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k


def _spec(config, ids, n_groups, bins=64, n_max=None):
    from th_rl_amd.group_stats import GroupSpec, resolve_ranges
    return GroupSpec(len(config["agents"]), ids, n_groups, resolve_ranges(config), bins=bins, n_max=n_max)


# ------------------------------------------------------------------------------------------------ kernel alone
def _synthetic(E, N, G, B, rs, lo=0.0, hi=25.0):
    w = (hi - lo) / B
    r = rs.uniform(lo - 3.0, hi + 3.0, (E, N, G))
    a = rs.uniform(-0.1, 1.1, (E, N, G))
    edges = lo + rs.randint(0, B + 1, (E, N, G)) * w            # exactly on bin edges (and on hi)
    pick = rs.uniform(size=(E, N, G)) < 0.2
    r = np.where(pick, edges, r)
    if G > 3:
        r[0, 0, 0], r[0, 1, 1], r[-1, 0, 2] = np.nan, np.inf, -np.inf
        r[-1, -1, 3] = 1e6                                         # beyond the sums' clamp M
    return r, a


@pytest.mark.parametrize("G,n_groups", [(1, 1), (63, 7), (65537, 300), (1 << 20, 7)])
def test_kernel_matches_numpy_mirror(G, n_groups):
    import torch
    from th_rl_amd import _lib
    from th_rl_amd.group_stats import reduce_host, to_numpy
    rs = np.random.RandomState(G + n_groups)
    E, N, B = 3, 2, 64
    ids = rs.randint(0, n_groups, G).astype(np.int32)               # unsorted
    spec = _spec(TWO, ids, n_groups, bins=B)
    r, a = _synthetic(E, N, G, B, rs)
    L = _lib.load()
    rt, at = torch.from_numpy(r).cuda(), torch.from_numpy(a).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = to_numpy(spec.reduce(L, rt, at, E, spec.zeros(E, "cuda"), stream))
    want = reduce_host(r, a, ids, n_groups, spec.describe())
    _eq(got, want)
    # episodes cut into two calls: same bits
    st = spec.zeros(E, "cuda")
    spec.reduce(L, rt[:1], at[:1], 1, st, stream)
    spec.reduce(L, rt[1:], at[1:], E - 1, st, stream, at=1)
    _eq(to_numpy(st), want)


def test_kernel_one_bin_per_group_contention():
    """Every game of a group in one bin (a converged sweep): the wave-aggregated LDS path."""
    import torch
    from th_rl_amd import _lib
    from th_rl_amd.group_stats import reduce_host, to_numpy
    G, E, N, n_groups = 1 << 20, 2, 2, 8
    ids = (np.arange(G) % n_groups).astype(np.int32)
    spec = _spec(TWO, ids, n_groups, bins=256)
    r = np.broadcast_to((3.0 + 2.0 * ids)[None, None, :], (E, N, G)).copy()
    a = np.full((E, N, G), 0.3)
    L = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = to_numpy(spec.reduce(L, torch.from_numpy(r).cuda(), torch.from_numpy(a).cuda(), E, spec.zeros(E, "cuda"),
                               stream))
    want = reduce_host(r, a, ids, n_groups, spec.describe())
    _eq(got, want)
    assert (got["hist"].max(axis=-1) == G // n_groups).all()


def test_kernel_validation():
    import torch
    from th_rl_amd import _lib
    L = _lib.load()
    G, N = 16, 2
    ids = np.zeros(G, np.int32)
    spec = _spec(TWO, ids, 1, bins=8)
    rt = torch.zeros((1, N, G), dtype=torch.float64, device="cuda")
    st = spec.zeros(1, "cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def args(**kw):
        a = _lib.GroupStatsArgs()
        perm, seg = spec._device_index(rt.device)
        a.n_games, a.n_agents, a.n_episodes, a.n_groups, a.n_bins = G, N, 1, 1, 8
        a.game_reward_log = a.game_action_log = rt.data_ptr()
        a.group_of = ids.ctypes.data_as(ctypes.c_void_p)
        a.perm, a.seg_off = perm.data_ptr(), seg.data_ptr()
        for q in range(2 * N + 1):
            a.lo[q], a.hi[q], a.inv_w[q] = spec.lo[q], spec.hi[q], spec.inv_w[q]
            a.scale[q][0], a.scale[q][1] = spec.scale[q, 0], spec.scale[q, 1]
        a.hist, a.sums, a.minmax = st["hist"].data_ptr(), st["sums"].data_ptr(), st["minmax"].data_ptr()
        for k, v in kw.items():
            if k == "lo0":
                a.lo[0] = v
            elif k == "scale0":
                a.scale[0][0] = v
            else:
                setattr(a, k, v)
        return a

    assert L.thrl_group_stats(ctypes.byref(args()), stream) == 0
    assert L.thrl_group_stats(ctypes.byref(args(n_bins=0)), stream) == -3
    assert L.thrl_group_stats(ctypes.byref(args(n_bins=1025)), stream) == -3
    assert L.thrl_group_stats(ctypes.byref(args(lo0=25.0)), stream) == -1            # hi <= lo
    assert L.thrl_group_stats(ctypes.byref(args(scale0=3.0)), stream) == -1          # not a power of two
    assert L.thrl_group_stats(ctypes.byref(args(scale0=2.0 ** 62)), stream) == -1    # int64 bound
    bad = ids.copy()
    bad[5] = 1
    assert L.thrl_group_stats(ctypes.byref(args(group_of=bad.ctypes.data_as(ctypes.c_void_p))), stream) == -1
    assert b"group_of[5]" in L.thrl_last_error()
    assert L.thrl_group_stats(ctypes.byref(args(perm=None)), stream) == -2
    assert L.thrl_group_stats(None, stream) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ episode paths
def _sweep(N, G):
    rs = np.random.RandomState(7)
    return dict(gamma=rs.choice([0.35, 0.9, 0.95], (N, G)), alpha=rs.choice([0.05, 0.1, 0.5], (N, G)))


# label, config, G, kernel, sweep
PATHS = [
    ("wave_plain", TWO, 4096, "wave", False),
    ("wave_sweep", NOISY, 4096, "wave", True),
    ("wave_cycle", CYCLE, 4096, "wave", False),
    ("tuple", GRIDS, 4096, "tuple", False),
    ("generic", TWO, 1024, "generic", False),
]


def _gb(config, G, kernel, sweep, seed=11):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype="float32", kernel=kernel, seed=seed, sweep=_sweep(2, G) if sweep else None)
    return gb.init_tables()


@pytest.mark.parametrize("label,config,G,kernel,sweep", PATHS, ids=[p[0] for p in PATHS])
def test_gamebatch_group_stats_equal_reduction_of_rows(label, config, G, kernel, sweep):
    from th_rl_amd.group_stats import assign_groups, reduce_host
    E = 6
    ids, ng, _ = assign_groups(G, sweep=_sweep(2, G) if sweep else None)
    if not sweep:
        ids, ng = (np.arange(G) % 5).astype(np.int32), 5
    spec = _spec(config, ids, ng)
    a, b, c = _gb(config, G, kernel, sweep), _gb(config, G, kernel, sweep), _gb(config, G, kernel, sweep)
    oa = a.run(E, per_game_logs=True, group_stats=spec)
    ob = b.run(E)
    oc = c.run(E, group_stats=spec)
    assert oa["kernel"] == ob["kernel"] == oc["kernel"]
    _eq(oa["group_stats"], reduce_host(oa["game_reward_log"], oa["game_action_log"], ids, ng, spec.describe()))
    _eq(oc["group_stats"], oa["group_stats"])
    for x in (a, c):
        assert np.array_equal(x.tables_numpy(), b.tables_numpy())
        assert np.array_equal(x.counters_numpy(), b.counters_numpy())
        assert np.array_equal(x.states_numpy(), b.states_numpy())
        assert x.eps == b.eps
        for k, v in x.sweep.items():
            assert np.array_equal(v.cpu().numpy(), b.sweep[k].cpu().numpy())
    for o in (oa, oc):      # fixed-point mean logs on the wave kernel; float64 atomics elsewhere (1e-12, include/thrl.h)
        if kernel == "wave":
            assert np.array_equal(o["reward_log"], ob["reward_log"]) and np.array_equal(o["action_log"], ob["action_log"])
        else:
            np.testing.assert_allclose(o["reward_log"], ob["reward_log"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(o["action_log"], ob["action_log"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("fused", [True, False])
def test_mixed_group_stats_equal_reduction_of_rows(fused):
    from th_rl_amd.group_stats import reduce_host
    from th_rl_amd.mixed import MixedGameBatch
    G, E = 256 if fused else 64, 3
    ids = (np.arange(G) % 3).astype(np.int32)
    spec = _spec(MIXED, ids, 3)
    a = MixedGameBatch(MIXED, n_games=G, dtype="float32", seed=5).init_tables()
    b = MixedGameBatch(MIXED, n_games=G, dtype="float32", seed=5).init_tables()
    oa = a.run(E, fused=fused, group_stats=spec)
    ob = b.run(E, fused=fused)
    _eq(oa["group_stats"], reduce_host(oa["game_reward_log"], oa["game_action_log"], ids, 3, spec.describe()))
    assert np.array_equal(oa["game_reward_log"], ob["game_reward_log"])
    assert np.array_equal(oa["reward_log"], ob["reward_log"])
    assert np.array_equal(a.tables_numpy(), b.tables_numpy()) and np.array_equal(a.states_numpy(), b.states_numpy())
    assert np.array_equal(a.nn[1].params.cpu().numpy(), b.nn[1].params.cpu().numpy())
    if fused:           # the mean-log-only path (rows reused launch by launch) gives the same statistics
        c = MixedGameBatch(MIXED, n_games=G, dtype="float32", seed=5).init_tables()
        _eq(c.run(E, fused=True, per_game_logs=False, group_stats=spec)["group_stats"], oa["group_stats"])
    mr, ma, raw = a.play_greedy(iters=2, group_stats=spec)
    _eq(raw, reduce_host(mr, ma, ids, 3, spec.describe()))


# ------------------------------------------------------------------------------------------------ sharding
def test_two_shards_merged_equal_one_batch():
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import assign_groups, merge, GroupSpec, resolve_ranges
    G, E = 4096, 4
    sw = {"gamma": np.repeat([0.35, 0.9, 0.95, 0.5], G // 4)[np.random.RandomState(3).permutation(G)]}
    ids, ng, _ = assign_groups(G, sweep=sw)
    n_max = int(np.bincount(ids).max())
    rng = resolve_ranges(TWO)
    one = GameBatch(TWO, n_games=G, seed=9, sweep=sw).init_tables()
    full = one.run(E, group_stats=GroupSpec(2, ids, ng, rng, n_max=n_max))["group_stats"]
    parts = []
    for lo, hi in ((0, G // 2), (G // 2, G)):
        gb = GameBatch(TWO, n_games=hi - lo, seed=9, game_offset=lo, sweep={"gamma": sw["gamma"][lo:hi]}).init_tables()
        parts.append(gb.run(E, group_stats=GroupSpec(2, ids[lo:hi], ng, rng, n_max=n_max))["group_stats"])
    _eq(merge(parts), full)


def test_sharded_launch_group_stats_equal_single_process(tmp_path):
    from th_rl_amd import trainer
    from th_rl_amd.launch import launch
    G = 101
    sw = {"gamma": [[0.35, 0.9, 0.95][g % 3] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "sweep": sw,
                              "group_stats": {"bins": 32, "histograms": True, "greedy_iters": 2}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    for p in ("group", "greedy"):
        for f in ("sums", "hist", "min", "max", "quantiles", "mean"):
            x = np.load(tmp_path / "one" / ("%s_%s.npy" % (p, f)))
            y = np.load(tmp_path / "two" / ("%s_%s.npy" % (p, f)))
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (p, f)
    assert json.load(open(tmp_path / "one" / "groups.json")) == json.load(open(tmp_path / "two" / "groups.json"))


# ------------------------------------------------------------------------------------------------ trainer
def test_train_one_chunking_invariance(tmp_path, monkeypatch):
    from th_rl_amd import trainer
    G = 1024
    orig = trainer.game_log_chunk
    monkeypatch.setattr(trainer, "game_log_chunk", lambda n, g, c=1, budget=None: orig(n, g, c, budget=8 * n * g * 4))
    sw = {"gamma": [[0.35, 0.9, 0.95, 0.5][g % 4] for g in range(G)]}
    outs = []
    for pf in (3, 7):
        cfg = dict(TWO, training={"epochs": 20, "print_freq": pf, "seed": 4, "n_games": G, "sweep": sw,
                                  "group_stats": {"histograms": True}})
        (tmp_path / ("c%d.json" % pf)).write_text(json.dumps(cfg))
        trainer.train_one(str(tmp_path / ("r%d" % pf)), str(tmp_path / ("c%d.json" % pf)))
        outs.append(tmp_path / ("r%d" % pf))
    for f in ("group_sums", "group_hist", "group_quantiles"):
        assert np.array_equal(np.load(outs[0] / (f + ".npy")), np.load(outs[1] / (f + ".npy"))), f


def test_train_one_group_artefacts(tmp_path):
    import torch
    from th_rl_amd import trainer, utils
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import quantiles, reduce_host, min_max
    G, epochs, gammas = 4096, 12, [0.35, 0.5, 0.9, 0.95]
    sw = {"gamma": [gammas[g % 4] for g in range(G)]}
    cfg = dict(TWO, training={"epochs": epochs, "print_freq": 5, "seed": 8, "n_games": G, "sweep": sw,
                              "game_logs": True,
                              "group_stats": {"bins": 128, "histograms": True, "greedy_iters": 3}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "groups.json"))
    assert [g["values"] for g in desc["groups"]] == [{"gamma": x} for x in gammas]
    assert [g["games"] for g in desc["groups"]] == [G // 4] * 4
    rew, act = np.load(exp / "game_rewards.npy"), np.load(exp / "game_actions.npy")
    ids = np.arange(G) % 4
    mean = np.load(exp / "group_mean.npy")
    assert mean.shape == (epochs, 4, 5)
    for k in range(4):
        np.testing.assert_allclose(mean[:, k, :2], rew[:, :, ids == k].mean(axis=2), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(mean[:, k, 2:4], act[:, :, ids == k].mean(axis=2), rtol=1e-12, atol=1e-12)
    raw = reduce_host(rew, act, ids, 4, desc)
    assert np.array_equal(np.load(exp / "group_sums.npy"), raw["sums"])
    assert np.array_equal(np.load(exp / "group_hist.npy"), raw["hist"])
    vmin, vmax = min_max(raw["minmax"])
    lo, hi = [r[0] for r in desc["ranges"]], [r[1] for r in desc["ranges"]]
    qs = np.load(exp / "group_quantiles.npy")
    assert np.array_equal(qs, quantiles(raw["hist"], vmin, vmax, desc["quantiles"], lo, hi))
    tot = rew.sum(axis=1)
    w = (hi[4] - lo[4]) / desc["bins"]
    for k in range(4):
        ref = np.quantile(tot[:, ids == k], desc["quantiles"], axis=1, method="inverted_cdf").T
        assert (np.abs(qs[:, k, 4, :] - ref) <= w).all()
    df = utils.group_quantiles(str(exp), 2)
    assert list(df.columns) == ["25th", "median", "75th", "Nash", "Cartel"] and len(df) == epochs
    assert abs(df["Cartel"][0] - 25.0) < 1e-12
    gl = utils.group_log(str(exp), 1)
    assert np.array_equal(gl.to_numpy(), mean[:, 1, :4])
    # greedy: play_greedy's rows of the trained games, reduced the same way
    gb = GameBatch(TWO, n_games=G, seed=8, sweep=sw)
    gb.load(str(exp / "batch.pt"))
    mr, ma = gb.play_greedy(iters=3)
    graw = reduce_host(mr, ma, ids, 4, desc)
    assert np.array_equal(np.load(exp / "greedy_sums.npy"), graw["sums"])
    assert np.array_equal(np.load(exp / "greedy_hist.npy"), graw["hist"])
    del torch
