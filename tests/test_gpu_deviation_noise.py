"""The deviation test under demand noise on the device (thrl_deviation_noise, GameBatch.deviation_noise,
training.deviation with "noise"): every per-game output and every row bit-equal to the numpy mirror
(tests/deviation_noise_mirror.py: the same recurrence with an explicit ascending loop over the source cells) on fresh and
trained headline tables in f32 and f64 (J = 101: two cells per lane, one of them masked) with a best response and a
fixed action over one and three periods, a 20-state config (J = 21: most lanes idle), three agents on individual grids
with deviator 2, the 3,000-state config (indexing and the LDS limit), per-game noise probabilities with two bad entries,
a game count below the batch's, more games than resident blocks, a given policy with no tables, weights that are no
stationary distribution, chunked rows, the sweep's gamma; the identities (the baseline is stationary's reward, the mass,
D(0) = 0), the dense route, and the trainer's artefacts, a sharded launch and MixedGameBatch."""
import json

import numpy as np
import pytest

import deviation_noise_mirror as DN
import stationary_mirror as S
from test_gpu_stationary import AG, BIG, ENV, SMALL, THREE, TWO, _batch, _bits_equal, _tabs

pytestmark = pytest.mark.gpu

FIELDS = DN.AGENT_FIELDS + DN.FLOAT_FIELDS + DN.INT_FIELDS
ROWS = DN.ROW_FIELDS


def _gamma(gb, G):
    gam = gb.sweep.get("gamma") if getattr(gb, "sweep", None) else None
    return None if gam is None else gam.cpu().numpy()[:, :G]


def _check(gb, config, noise_prob=0.05, weights="stationary", n_games=None, policy=None, stat_kw=None, **kw):
    """deviation_noise against the mirror on the same weights (the device's own pi for "stationary": test_gpu_stationary
    holds that one to its mirror), and the identities."""
    from th_rl_amd import deviation as dv
    out = gb.deviation_noise(noise_prob=noise_prob, weights=weights, rows=True, n_games=n_games, policy=policy,
                             **dict(stat_kw or {}, **kw))
    G = out["gain"].shape[0]
    pol = S.policies(config, gb.tables_numpy()) if policy is None else policy.cpu().numpy().view(np.uint16)
    K = kw.get("steps", 32)
    w = weights.cpu().numpy() if hasattr(weights, "cpu") else weights
    if isinstance(weights, str):
        st = gb.stationary(noise_prob=noise_prob, pi=True, n_games=n_games, policy=policy, **(stat_kw or {}))
        w = st["pi"]
        _bits_equal(out["base_reward"], st["stat_reward"], "base_reward against stat_reward")
        _bits_equal(out["base_action"], st["stat_action"], "base_action against stat_action")
        _bits_equal(out["stat_iters"], st["iters"], "stat_iters")
        # |mass - 1|: _identity's bound for the start, iters * (J + 2) ulp, and (J + 2) ulp more for each of the K steps
        ok = st["iters"] > 0
        err = np.abs(out["mass"][ok] - 1.0)
        bound = (st["iters"][ok] + K) * (out["n_cells"] + 2) * 2.0 ** -52
        print("max |mass - 1| = %.3e (bound of that game %.3e)" % (err.max(), bound[err.argmax()]))
        assert (err <= bound).all() and (out["mass"][~ok] == 0).all()
    ref = DN.analyse(config, _tabs(config), pol, noise_prob, w, deviator=kw.get("deviator", 0), steps=K,
                     dev_len=kw.get("dev_len", 1), dev_action=dv.action_index(kw.get("action", "best_response")),
                     ret_tol=kw.get("ret_tol", 1e-6), gamma=_gamma(gb, G), n_games=n_games)
    for f in FIELDS + ROWS:
        _bits_equal(out[f], ref[f], f)
    assert (out["dist_rows"][0] == 0.0).all()                              # D(0) == 0
    return out, ref


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("episodes", [0, 200])
def test_headline_matches_mirror(dtype, episodes):
    gb = _batch(TWO, 139, dtype, seed=11, episodes=episodes)           # 139: no multiple of a wave or a block
    pi = gb.stationary(noise_prob=0.05, pi=True)["pi"]
    # ret_tol = 0.07: after a one-period shock D(32) of these games lies on both sides of it
    out, ref = _check(gb, TWO, ret_tol=0.07)
    assert out["n_cells"] == 101
    _check(gb, TWO, weights=pi, dev_len=3, ret_tol=0.07)
    _check(gb, TWO, weights=pi, action=4, deviator=1)
    _check(gb, TWO, weights=pi, action=17, dev_len=3, deviator=1)
    if episodes:
        # the test is not vacuous: from the mirror's outputs
        print("dev_share in [%.3f, %.3f], ret_step >= 0 in %d games, == -1 in %d, low < 0 in %d, D(K) quartiles %s"
              % (ref["dev_share"].min(), ref["dev_share"].max(), (ref["ret_step"] >= 0).sum(), (ref["ret_step"] == -1).sum(),
                 (ref["low"] < 0).sum(), np.quantile(ref["dist"], [0, 0.25, 0.5, 0.75, 1])))
        assert (ref["dev_share"] > 0).any()
        assert (ref["ret_step"] >= 0).any()
        assert ((ref["ret_step"] == -1) | (ref["low"] < 0)).any()


def test_20_state_config_most_lanes_idle():
    gb = _batch(SMALL, 70, seed=4, episodes=30)
    out, _ = _check(gb, SMALL)
    assert out["n_cells"] == 21
    _check(gb, SMALL, action=0, dev_len=2, steps=9, deviator=1)


def test_three_agents_individual_grids_clipped_prices():
    gb = _batch(THREE, 48, seed=5, episodes=50)
    out, _ = _check(gb, THREE, deviator=2, steps=16)
    assert out["n_cells"] > 64
    _check(gb, THREE, deviator=2, steps=16, dev_len=3, action=1, noise_prob=0.5)


def test_3000_state_config_indexing_and_lds_limit():
    gb = _batch(BIG, 4, seed=6, episodes=20)
    out, _ = _check(gb, BIG, steps=4, stat_kw=dict(max_iters=16))
    assert out["n_cells"] == 3001 and (out["stat_iters"] == 16).all()
    _check(gb, BIG, steps=4, dev_len=2, action=20, weights=np.tile(_tabs(BIG)["cell_w"], (4, 1)))


def test_per_game_noise_with_bad_entries():
    G = 12
    gb = _batch(TWO, G, seed=7, episodes=60)
    p = np.array([0.01, 0.05, 0.0, 0.5, 1.0, np.nan, 0.05, 0.01, 1.0, 0.5, 0.05, 0.2])
    out, _ = _check(gb, TWO, noise_prob=p, steps=12)
    bad = np.array([2, 5])
    for f in FIELDS + ROWS:
        assert (np.asarray(out[f])[..., bad] == (-1 if f in DN.INT_FIELDS else 0)).all(), f
    assert (out["stat_iters"][bad] == -1).all() and (np.delete(out["mass"], bad) > 0.99).all()
    # the neighbours are what a scalar call gives them
    one = gb.deviation_noise(noise_prob=0.05, steps=12, rows=True)
    for g in (1, 6, 10):
        for f in FIELDS + ROWS:
            _bits_equal(np.asarray(out[f])[..., g], np.asarray(one[f])[..., g], f)
    # the batch's own sweep array is the default
    gb.set_sweep({"noise_prob": np.where(np.isfinite(p) & (p > 0), p, 0.3)})
    own = gb.deviation_noise(steps=12)
    _bits_equal(own["noise_prob"], np.where(np.isfinite(p) & (p > 0), p, 0.3))
    _bits_equal(own["gain"][[0, 1, 3]], out["gain"][[0, 1, 3]])


def test_fewer_games_than_the_batch_and_more_than_resident_blocks():
    import torch
    gb = _batch(SMALL, 77, seed=10, episodes=20)
    whole = gb.deviation_noise(noise_prob=0.5, steps=8, rows=True)
    part, _ = _check(gb, SMALL, noise_prob=0.5, n_games=30, steps=8)
    for f in FIELDS + ROWS:
        _bits_equal(part[f], whole[f][..., :30], f)
    # more games than blocks the device keeps resident: every block loops over games
    cus = torch.cuda.get_device_properties(gb.device).multi_processor_count
    G = cus * 32 + 77
    big = _batch(SMALL, G, seed=12)
    w = np.tile(_tabs(SMALL)["cell_w"], (G, 1))
    out = big.deviation_noise(noise_prob=0.5, steps=6, weights=w, rows=True)
    pol = S.policies(SMALL, big.tables_numpy())
    tail = np.r_[0:40, G - 120:G]
    ref = DN.analyse(SMALL, _tabs(SMALL), pol[tail], 0.5, w[tail], steps=6)
    for f in FIELDS + ROWS:
        _bits_equal(np.asarray(out[f])[..., tail], ref[f], f)


def test_policy_given_reads_no_table_and_other_weights():
    from th_rl_amd import crossplay as xp
    from th_rl_amd._lib import ThrlError
    G = 40
    gb = _batch(TWO, G, seed=9, episodes=100)
    want = gb.deviation_noise(noise_prob=0.05, steps=10, rows=True)
    pol = xp.extract(gb)
    got, _ = _check(gb, TWO, policy=pol, steps=10)                     # q = NULL with THRL_STAT_POLICY_GIVEN
    for f in FIELDS + ROWS:
        _bits_equal(got[f], want[f], f)
    # weights that are no stationary distribution: the unit mass on one cell per game
    J = _tabs(TWO)["n_cells"]
    w = np.zeros((G, J))
    w[np.arange(G), (7 * np.arange(G)) % J] = 1.0
    out, _ = _check(gb, TWO, weights=w, steps=10, dev_len=2)
    assert (out["stat_iters"] == 0).all() and (np.abs(out["mass"] - 1.0) <= 10 * (J + 2) * 2.0 ** -52).all()
    import torch
    _check(gb, TWO, weights=torch.from_numpy(w).to(gb.device), steps=10, dev_len=2)
    with pytest.raises(ThrlError, match="weights must be shaped"):
        gb.deviation_noise(noise_prob=0.05, weights=w[:, :50])


def test_chunked_rows_group_stats_and_sweep_gamma():
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import GroupSpec, reduce_host, resolve_ranges
    G = 96
    sw = {"gamma": [[0.5, 0.9, 0.95, 0.35][g % 4] for g in range(G)]}
    gb = GameBatch(TWO, n_games=G, dtype="float32", seed=13, sweep=sw).init_tables()
    gb.run(60, logs=False)
    one, _ = _check(gb, TWO, steps=8)                                  # the mirror discounts with the sweep's gamma
    plain = GameBatch(TWO, n_games=G, dtype="float32", seed=13).set_tables(gb.tables_numpy(), np.full(G, 5.0))
    plain = plain.deviation_noise(noise_prob=0.05, steps=8)
    assert not np.array_equal(plain["gain"], one["gain"]) and np.array_equal(plain["gain_dev"], one["gain_dev"])
    chunked = gb.deviation_noise(noise_prob=0.05, steps=8, rows=True, budget=8 * 2 * G * 3)       # 3 + 3 + 2 periods
    for f in FIELDS + ROWS:
        _bits_equal(chunked[f], one[f], f)
    ids = np.arange(G) % 3
    spec = GroupSpec(2, ids, 3, resolve_ranges(TWO), bins=64)
    st = gb.deviation_noise(noise_prob=0.05, steps=8, group_stats=spec, budget=8 * 2 * G * 3)
    assert "reward_rows" not in st
    for f in FIELDS:
        _bits_equal(st[f], one[f], f)
    raw = reduce_host(one["reward_rows"], one["action_rows"], ids, 3, spec.describe())
    for k in ("hist", "sums", "minmax"):
        assert np.array_equal(np.asarray(st["group_stats"][k]).view(np.uint8), np.asarray(raw[k]).view(np.uint8)), k


def test_dense_route_within_its_bound():
    gb = _batch(TWO, 8, "float64", seed=11, episodes=100)
    K = 16
    out = gb.deviation_noise(noise_prob=0.05, steps=K, dev_len=2, rows=True)
    pi = gb.stationary(noise_prob=0.05, pi=True)["pi"]
    pol = S.policies(TWO, gb.tables_numpy())
    worst = 0.0
    for g in range(8):
        Ed, rmax = DN.dense(TWO, _tabs(TWO), pol, 0.05, pi, g, steps=K, dev_len=2)
        for tau in range(K):
            err = np.abs(Ed[tau] - out["reward_rows"][tau, :, g]).max()
            worst = max(worst, err / DN.dense_bound(tau, 101, rmax))
            assert err <= DN.dense_bound(tau, 101, rmax), (g, tau, err)
    print("max |E - dense| / bound = %.3f" % worst)


# ------------------------------------------------------------------------------------------------ invariances
def test_mixed_batch_equals_game_batch():
    from th_rl_amd.mixed import MixedGameBatch
    G = 64
    gb = _batch(TWO, G, seed=13, episodes=50)
    want = gb.deviation_noise(noise_prob=0.05, steps=8, rows=True)
    mb = MixedGameBatch(TWO, n_games=G, dtype="float32").set_tables(gb.tables_numpy(), np.full(G, 5.0))
    got = mb.deviation_noise(noise_prob=0.05, steps=8, rows=True)
    for f in FIELDS + ROWS:
        _bits_equal(got[f], want[f], f)


def test_train_one_noise_artefacts_beside_untouched_noise_free_ones(tmp_path):
    from th_rl_amd import trainer, utils, deviation as dv
    from th_rl_amd.batched import GameBatch
    G = 48
    runs = {}
    for name, opt in (("plain", {"steps": 8}), ("noise", {"steps": 8, "noise": {"noise_prob": 0.05}})):
        cfg = dict(TWO, training={"epochs": 10, "print_freq": 500, "seed": 21, "n_games": G, "n_groups": 2,
                                  "groups": [g % 2 for g in range(G)], "group_stats": {"bins": 64, "histograms": True},
                                  "deviation": opt})
        (tmp_path / (name + ".json")).write_text(json.dumps(cfg))
        runs[name] = tmp_path / name
        trainer.train_one(str(runs[name]), str(tmp_path / (name + ".json")))
    names = sorted(f.name for f in runs["plain"].iterdir() if f.name.startswith("dev"))
    assert {"deviation.json", "dev_cycle.npy", "dev0_gain.npy", "dev1_post.npy", "dev0_mean.npy"} <= set(names)
    assert not any(n.startswith("devn") or n == "deviation_noise.json" for n in names)
    for n in names:        # the noise-free artefacts are byte for byte those of a run without the option
        assert (runs["plain"] / n).read_bytes() == (runs["noise"] / n).read_bytes(), n
    exp = runs["noise"]
    desc = json.load(open(exp / "deviation_noise.json"))
    assert desc["options"]["noise"] == dict(dv.NOISE_DEFAULTS, noise_prob=0.05) and desc["n_cells"] == 101
    assert [(r["group"], r["deviator"]) for r in desc["summary"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert all(r["games"] == G // 2 and r["solved"] == G // 2 for r in desc["summary"])
    gb = GameBatch(TWO, n_games=G).load(str(exp / "batch.pt"))
    games = {}
    for d in (0, 1):
        games[d] = dv.load_noise_games(str(exp), d)
        direct = gb.deviation_noise(deviator=d, steps=8, noise_prob=0.05)
        for f in FIELDS + ("noise_prob", "stat_iters"):
            _bits_equal(games[d][f], direct[f], f)
        assert np.load(exp / ("devn%d_mean.npy" % d)).shape == (8, 2, 5)
    assert desc["summary"] == json.loads(json.dumps(dv.summarize_noise(games, np.arange(G) % 2, 2, [0, 1])))
    df = utils.deviation_noise_summary(str(exp))
    assert len(df) == 4 and df.loc[0, "n_cells"] == 101
    gm = utils.deviation_noise_games(str(exp), deviator=1)
    assert gm.index.tolist() == list(range(G)) and gm["solved"].all()
    _bits_equal(gm["gain"].to_numpy(), games[1]["gain"])
    q = utils.group_quantiles(str(exp), 1, "total", prefix="devn0")
    assert len(q) == 8
    with pytest.raises(KeyError, match="training.deviation.noise"):
        utils.deviation_noise_summary(str(runs["plain"]))


def test_sharded_launch_with_noise_equal_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 37
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "n_groups": 2,
                              "groups": [g % 2 for g in range(G)], "group_stats": {"bins": 32, "histograms": True},
                              "deviation": {"steps": 6, "noise": {"noise_prob": 0.2}}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    for name in ("deviation.json", "deviation_noise.json"):
        assert json.load(open(tmp_path / "one" / name)) == json.load(open(tmp_path / "two" / name)), name
    files = sorted(f.name for f in (tmp_path / "one").iterdir()
                   if f.name.startswith("devn") and f.name.split("_", 1)[1] in ("games.npy", "steps.npy", "base.npy", "prob.npy",
                                                                               "stat_iters.npy"))
    assert len(files) == 8
    for f in files:
        _bits_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f), f)
    for d in (0, 1):
        a, b = utils.deviation_noise_games(str(tmp_path / "one"), d), utils.deviation_noise_games(str(tmp_path / "two"), d)
        assert a.index.tolist() == b.index.tolist() == list(range(G))
        for c in a.columns:
            assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
        for f in ("sums", "hist", "min", "max", "quantiles"):
            x = np.load(tmp_path / "one" / ("devn%d_%s.npy" % (d, f)))
            y = np.load(tmp_path / "two" / ("devn%d_%s.npy" % (d, f)))
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (d, f)
