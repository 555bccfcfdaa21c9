"""The equilibrium check under demand noise on the device (thrl_equilibrium_noise, equilibrium_noise(), the option
"noise" of training.equilibrium): every output, the per-cell arrays included, bit-equal to the numpy mirror
(tests/equilibrium_noise_mirror.py: the same sweeps with an explicit ascending loop over the band) on a 20-state config
(J = 21: most lanes idle), fresh and trained headline tables in f32 and f64 (J = 101: two cells per lane, one of them
masked), three agents on individual grids with point cells and clipped prices (J = 128), and a 10-state config whose
agents have more actions than the game has cells (z per (cell, action) instead of per tuple); per-game noise
probabilities and discount factors with bad entries, the sweep cap, a given policy with no tables, a game count below the
batch's, more games than resident blocks, no weights and weights of the caller's; the known answers through set_tables;
the invariances; and the trainer's artefacts."""
import ctypes
import json

import numpy as np
import pytest

import equilibrium_mirror as E
import equilibrium_noise_mirror as EN
import stationary_mirror as S

pytestmark = pytest.mark.gpu

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
SMALL = {"agents": [dict(AG, states=20), dict(AG, states=20, gamma=0.9)], "environment": dict(ENV)}
TINY = {"agents": [dict(AG, states=10, gamma=0.9), dict(AG, states=10, gamma=0.9)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
INT = ("iters", "sweeps", "n_diff_all")
FLOAT = ("loss_all", "loss_all_mean")
WEIGHTED = ("loss_w", "diff_w", "v_w")
CELL = ("br_policy", "v_opt", "v_pi")
_TABS = {}


def _tabs(config):
    from th_rl_amd import stationary as sn
    key = json.dumps(config, sort_keys=True)
    if key not in _TABS:
        _TABS[key] = sn.tables(config)
    return _TABS[key]


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _same(got, want, fields, sel=None):
    for f in fields:
        w = np.asarray(want[f])
        if sel is not None:
            w = w[:, sel]
        _bits_equal(got[f], w, f)


def _batch(config, G, dtype="float32", seed=3, episodes=0):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, seed=seed).init_tables()
    if episodes:
        gb.run(episodes, logs=False)
    return gb


def _weights(G, J, seed=0):
    w = np.random.RandomState(seed).uniform(0.0, 1.0, (G, J))
    return w / w.sum(axis=1, keepdims=True)


def _check(gb, config, noise_prob=0.05, weights="random", policy=None, gamma=None, capped_on_purpose=False, tabs=None,
           **kw):
    """equilibrium_noise(policies=True, ...) against the mirror; returns the device's result."""
    tabs = _tabs(config) if tabs is None else tabs
    G = kw.get("n_games") or gb.G
    if isinstance(weights, str) and weights == "random":
        weights = _weights(G, tabs["n_cells"], seed=G)
    out = gb.equilibrium_noise(noise_prob=noise_prob, policies=True, weights=weights, policy=policy, tabs=tabs, **kw)
    pol = S.policies(config, gb.tables_numpy()) if policy is None else policy.cpu().numpy().view(np.uint16)
    ref = EN.analyse(config, tabs, pol, noise_prob, agents=kw.get("agents"), gamma=gamma, weights=weights,
                     eval_tol=kw.get("eval_tol", 1e-12), max_sweeps=kw.get("max_sweeps", 8192), n_games=kw.get("n_games"))
    fields = INT + FLOAT + CELL + (WEIGHTED if weights is not None else ())
    sel = out["agents"]
    for f in fields:
        _bits_equal(np.asarray(out[f])[sel], np.asarray(ref[f])[sel], f)
    assert (weights is not None) == ("loss_w" in out)
    if not capped_on_purpose:       # the cap is a condition of these tests, not a measurement: held on the mirror
        ok = (np.asarray(noise_prob) > 0) & (np.asarray(noise_prob) <= 1) & np.ones(G, bool)
        it = np.asarray(ref["iters"])[sel]
        if gamma is not None:
            ok = ok[None, :] & (np.asarray(gamma)[sel][:, :G] >= 0) & (np.asarray(gamma)[sel][:, :G] < 1)
        else:
            ok = np.broadcast_to(ok, it.shape)
        assert (it[ok] >= 0).all() and (it[~ok] == -1).all()
        print("rounds <= %d, sweeps <= %d" % (it.max(), np.asarray(ref["sweeps"])[sel].max()))
    return out


# ------------------------------------------------------------------------------------------------ mirror
def test_20_state_config_most_lanes_idle_defaults():
    gb = _batch(SMALL, 70, seed=4, episodes=30)
    out = _check(gb, SMALL)
    assert out["n_cells"] == 21 and out["eval_tol"] == 1e-12 and out["max_sweeps"] == 8192


@pytest.mark.parametrize("dtype,episodes,eval_tol", [("float32", 0, 1e-9), ("float64", 0, 1e-9), ("float32", 200, 1e-12),
                                                     ("float64", 200, 1e-9)])
def test_headline_matches_mirror(dtype, episodes, eval_tol):
    gb = _batch(TWO, 139, dtype, seed=11, episodes=episodes)           # 139: no multiple of a wave or a block
    out = _check(gb, TWO, eval_tol=eval_tol)
    assert out["n_cells"] == 101


def test_three_agents_individual_grids_point_cells_clipped_prices():
    gb = _batch(THREE, 48, seed=5, episodes=50)
    tabs = _tabs(THREE)
    assert tabs["n_cells"] == 128 and tabs["n_cells"] - tabs["n_intervals"] == 5 and tabs["band_w"] == 40
    _check(gb, THREE, eval_tol=1e-9)
    _check(gb, THREE, noise_prob=0.5, agents=[1, 2])


def test_more_actions_than_cells_z_per_cell_and_action():
    tabs = _tabs(TINY)
    assert 21 > tabs["n_cells"] == 11                                  # T = 441 > J * A = 231: z is not staged per tuple
    gb = _batch(TINY, 70, seed=6, episodes=20)
    _check(gb, TINY)


# ------------------------------------------------------------------------------------------------ edge cases
def test_per_game_noise_with_bad_entries():
    G = 12
    gb = _batch(SMALL, G, seed=7, episodes=60)
    p = np.array([0.01, 0.05, 0.0, 0.5, 1.0, np.nan, 0.05, 0.01, 1.0, 0.5, 0.05, 0.2])
    out = _check(gb, SMALL, noise_prob=p, eval_tol=1e-9)
    bad = np.array([2, 5])
    for f in INT + FLOAT + WEIGHTED + CELL:
        x = np.asarray(out[f])
        assert (x[:, bad] == (-1 if f == "iters" else 0)).all(), f
    assert (np.delete(out["iters"], bad, axis=1) >= 0).all()
    assert not out["br_all"][:, bad].any() and not out["br_w"][:, bad].any() and not out["perfect"][bad].any()
    # the neighbours are what a scalar call gives them
    one = gb.equilibrium_noise(noise_prob=0.05, eval_tol=1e-9, policies=True, weights=_weights(G, 21, seed=G))
    for g in (1, 6, 10):
        for f in INT + FLOAT + WEIGHTED + CELL:
            _bits_equal(np.asarray(out[f])[:, g], np.asarray(one[f])[:, g], f)
    # the batch's own sweep array is the default
    own_p = np.where(np.isfinite(p) & (p > 0), p, 0.3)
    gb.set_sweep({"noise_prob": own_p})
    own = gb.equilibrium_noise(eval_tol=1e-9, weights=None)
    _bits_equal(own["noise_prob"], own_p)
    _bits_equal(own["loss_all"][:, 0], out["loss_all"][:, 0])


def test_sweep_gamma_one_outside_and_one_zero():
    G = 10
    gb = _batch(SMALL, G, seed=8, episodes=40)
    gam = np.full((2, G), 0.9)
    gam[0, 3], gam[1, 3], gam[1, 6], gam[0, 8] = 1.0, 0.5, 0.0, np.nan
    gb.set_sweep({"gamma": gam})
    out = _check(gb, SMALL, gamma=gam, eval_tol=1e-9)
    for i, g in ((0, 3), (0, 8)):
        assert out["iters"][i, g] == -1 and out["sweeps"][i, g] == 0 and out["n_diff_all"][i, g] == 0
        assert all(np.isnan(out[f][i, g]) for f in FLOAT + WEIGHTED)
        assert np.isnan(out["v_opt"][i, g]).all() and np.isnan(out["v_pi"][i, g]).all()
    assert out["iters"][1, 3] >= 0 and not out["br_all"][0, 3]
    # gamma = 0: V = R exactly after 2 sweeps per evaluation, and sigma* is the one-period best response under noise
    pl, tabs = E.plan(SMALL), _tabs(SMALL)
    tup = S.cell_tuples(SMALL, S.policies(SMALL, gb.tables_numpy()), tabs, G)
    R, _, _ = EN.dense(pl, tabs, tup[6], 1, 0.05)
    assert out["sweeps"][1, 6] == 2 * (out["iters"][1, 6] + 1)
    _bits_equal(out["v_opt"][1, 6], R.max(axis=1))
    assert np.array_equal(out["br_policy"][1, 6], np.where(R.max(axis=1) > R[np.arange(21), tup[6] % 21],
                                                           R.argmax(axis=1), tup[6] % 21))


def test_max_sweeps_16_caps_every_game():
    gb = _batch(SMALL, 9, seed=9, episodes=20)
    out = _check(gb, SMALL, max_sweeps=16, capped_on_purpose=True)
    assert (out["iters"] == -1).all() and (out["sweeps"] == 16).all() and (out["n_diff_all"] == 0).all()
    assert np.isnan(out["loss_all"]).all() and np.isnan(out["loss_w"]).all() and not out["br_all"].any()
    pol = S.policies(SMALL, gb.tables_numpy())
    tup = S.cell_tuples(SMALL, pol, _tabs(SMALL), 9)
    assert np.array_equal(out["br_policy"][0], tup // 21) and np.array_equal(out["br_policy"][1], tup % 21)


def test_policy_given_reads_no_table_and_tracker_policy():
    import torch
    from th_rl_amd import _lib, crossplay as xp
    G = 40
    gb = _batch(SMALL, G, seed=10, episodes=60)
    w = _weights(G, 21, seed=G)
    want = gb.equilibrium_noise(noise_prob=0.05, policies=True, weights=w)
    pol = xp.extract(gb)
    got = _check(gb, SMALL, policy=pol, weights=w)
    _same(got, want, INT + FLOAT + WEIGHTED + CELL)
    # q = NULL through the library itself, and no weights: the three weighted outputs may be NULL
    tabs, dev = _tabs(SMALL), gb.device
    a = _lib.EquilibriumNoiseArgs()
    a.n_games, a.agents, a.flags, a.n_cells, a.band_w = G, 3, _lib.EQN_POLICY_GIVEN, tabs["n_cells"], tabs["band_w"]
    a.max_sweeps, a.eval_tol, a.noise_prob = 8192, 1e-12, 0.05
    keep = {f: torch.from_numpy(np.ascontiguousarray(tabs[f])).to(dev)
            for f in ("cell_rows", "det_cell", "band_lo", "band", "noise_reward")}
    outs = {f: torch.zeros((2, G), dtype=torch.int32, device=dev) for f in INT}
    outs.update({f: torch.zeros((2, G), dtype=torch.float64, device=dev) for f in FLOAT})
    for f, t in list(keep.items()) + list(outs.items()):
        setattr(a, f, t.data_ptr())
    a.policy = pol.data_ptr()
    assert gb.L.thrl_equilibrium_noise(ctypes.byref(gb.cfg), None, ctypes.byref(a), gb._stream()) == 0
    torch.cuda.synchronize(dev)
    for f, t in outs.items():
        _bits_equal(t.cpu().numpy(), want[f], f)
    # entries that are no action are clamped to the last action
    bad = pol.clone()
    bad[:, 5] = 30000
    _check(gb, SMALL, policy=bad, weights=None)
    # a convergence tracker's policy is analysed as it is
    tr = gb.track_convergence(window=5)
    got = gb.equilibrium_noise(noise_prob=0.05, policies=True, weights=w, policy=tr.policy)
    _same(got, want, INT + FLOAT + WEIGHTED + CELL)


def test_fewer_games_than_the_batch_more_than_resident_blocks_and_the_weights():
    import torch
    gb = _batch(SMALL, 77, seed=10, episodes=20)
    w = _weights(77, 21, seed=1)
    whole = gb.equilibrium_noise(noise_prob=0.5, policies=True, weights=w)
    part = _check(gb, SMALL, noise_prob=0.5, n_games=30, weights=w[:30])
    _same(part, {f: np.asarray(whole[f])[:, :30] for f in INT + FLOAT + WEIGHTED + CELL}, INT + FLOAT + WEIGHTED + CELL)
    # weights = None leaves the other outputs as they are; "stationary" is stationary()'s pi of the same noise
    none = _check(gb, SMALL, noise_prob=0.5, weights=None)
    _same(none, whole, INT + FLOAT + CELL)
    pi = gb.stationary(noise_prob=0.5, pi=True)["pi"]
    stat = gb.equilibrium_noise(noise_prob=0.5, policies=True)
    _same(stat, _check(gb, SMALL, noise_prob=0.5, weights=pi), INT + FLOAT + WEIGHTED + CELL)
    _same(stat, gb.equilibrium_noise(noise_prob=0.5, policies=True, weights=torch.from_numpy(pi)), WEIGHTED)
    # more games than blocks the device keeps resident: every block loops over games
    cus = torch.cuda.get_device_properties(gb.device).multi_processor_count
    G = cus * 32 + 77
    big = _batch(TINY, G, seed=12)
    out = big.equilibrium_noise(noise_prob=0.5, eval_tol=1e-9, policies=True, weights=None)
    pol = S.policies(TINY, big.tables_numpy())
    tail = np.r_[0:40, G - 120:G]
    ref = EN.analyse(TINY, _tabs(TINY), pol[tail], 0.5, eval_tol=1e-9)
    assert (ref["iters"] >= 0).all()
    _same({f: np.asarray(out[f])[:, tail] for f in INT + FLOAT + CELL}, ref, INT + FLOAT + CELL)


# ------------------------------------------------------------------------------------------------ known answers
def test_constant_rival_makes_the_problem_static():
    """A rival that plays one action in every row: the agent's continuation value does not depend on its action (the
    next cell's tuple holds the rival's action whatever the cell), so sigma*(k) = argmax_a R(k, a) in every cell, the
    same tuple everywhere, and V* = max_a R / (1 - gamma) within the evaluation's bound."""
    from th_rl_amd.batched import GameBatch
    pl, tabs = E.plan(TWO), _tabs(TWO)
    rival = 12
    q = np.concatenate([E.strategy_tables(TWO, [a0, rival]) for a0 in (3, 20, 0)])
    gb = GameBatch(TWO, n_games=3, dtype="float64", seed=1).set_tables(q, np.full(3, 5.0))
    out = _check(gb, TWO, agents=[0], weights=_tabs(TWO)["cell_w"][None, :].repeat(3, 0))
    R = 0.95 * pl["rew"][0].reshape(21, 21)[:, rival] + 0.05 * tabs["noise_reward"][0].reshape(21, 21)[:, rival]
    best = int(np.argmax(R))
    assert (out["br_policy"][0] == best).all()
    bound = EN.error_bound(0.95, 1e-12, tabs["band_w"], R.max() / 0.05)
    err = np.abs(out["v_opt"][0] - R.max() / (1.0 - 0.95)).max()
    print("best action %d, max |V* - max R / (1 - gamma)| = %.3e (bound %.3e)" % (best, err, bound))
    assert err <= bound
    assert (out["n_diff_all"][0] == 101).all() and (out["iters"][0] == 1).all() and (out["loss_all"][0] > 0).all()
    # an own policy already equal to sigma*: no round, no difference, no loss
    q = E.strategy_tables(TWO, [best, rival], n_games=2)
    gb = GameBatch(TWO, n_games=2, dtype="float64", seed=1).set_tables(q, np.full(2, 5.0))
    out = _check(gb, TWO, agents=[0])
    assert (out["iters"][0] == 0).all() and (out["n_diff_all"][0] == 0).all()
    for f in FLOAT + ("loss_w", "diff_w"):
        assert (out[f][0] == 0.0).all(), f
    assert out["br_all"][0].all() and out["br_w"][0].all() and out["perfect"].all()
    _bits_equal(out["v_opt"][0], out["v_pi"][0])


# ------------------------------------------------------------------------------------------------ invariances
def test_invariances_state_order_shards_mixed_own_noise():
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    from th_rl_amd import equilibrium as eq
    G = 64
    fields = INT + FLOAT + WEIGHTED + CELL
    gb = _batch(SMALL, G, seed=13, episodes=50)
    want = gb.equilibrium_noise(noise_prob=0.05, policies=True)
    q = gb.tables_numpy()
    # the training state does not matter
    gb.state.fill_(1.25)
    _same(gb.equilibrium_noise(noise_prob=0.05, policies=True), want, fields)
    # game order
    perm = np.random.RandomState(1).permutation(G)
    gp = GameBatch(SMALL, n_games=G, dtype="float32", seed=1).set_tables(q[perm], np.full(G, 5.0))
    _same(gp.equilibrium_noise(noise_prob=0.05, policies=True), want, fields, sel=perm)
    # two half batches equal the whole
    parts = []
    for lo, hi in ((0, 23), (23, 64)):
        gs = GameBatch(SMALL, n_games=hi - lo, dtype="float32", seed=1, game_offset=lo).set_tables(q[lo:hi], np.full(hi - lo, 5.0))
        parts.append(gs.equilibrium_noise(noise_prob=0.05, policies=True))
    _same(eq.combine_noise(parts), want, fields)
    # MixedGameBatch, all QTable
    mb = MixedGameBatch(SMALL, n_games=G, dtype="float32").set_tables(q, np.full(G, 5.0))
    _same(mb.equilibrium_noise(noise_prob=0.05, policies=True), want, fields)
    # the run's own noise probability, when it is the same number
    noisy = dict(SMALL, environment=dict(ENV, noise_prob=0.05))
    gn = GameBatch(noisy, n_games=G, dtype="float32", seed=1).set_tables(q, np.full(G, 5.0))
    own = gn.equilibrium_noise(policies=True)
    assert (own["noise_prob"] == 0.05).all()
    _same(own, want, fields)
    with pytest.raises(eq.ThrlError, match="without env noise"):
        gb.equilibrium_noise()


def test_train_one_noise_artefacts_beside_untouched_noise_free_ones(tmp_path):
    from th_rl_amd import trainer, utils, equilibrium as eq
    from th_rl_amd.batched import GameBatch
    G = 24
    noisy = dict(SMALL, environment=dict(ENV, noise_prob=0.05))
    runs = {}
    for name, opt in (("plain", {"policies": True}), ("noise", {"policies": True, "noise": True})):
        cfg = dict(noisy, training={"epochs": 10, "print_freq": 500, "seed": 21, "n_games": G, "n_groups": 2,
                                    "groups": [g % 2 for g in range(G)], "equilibrium": opt})
        (tmp_path / (name + ".json")).write_text(json.dumps(cfg))
        runs[name] = tmp_path / name
        trainer.train_one(str(runs[name]), str(tmp_path / (name + ".json")))
    names = sorted(f.name for f in runs["plain"].iterdir() if f.name.startswith("eq"))
    assert "equilibrium.json" in names and not any(n.startswith("eqn_") or n == "equilibrium_noise.json" for n in names)
    for n in names:        # the noise-free artefacts are byte for byte those of a run without the option
        assert (runs["plain"] / n).read_bytes() == (runs["noise"] / n).read_bytes(), n
    exp = runs["noise"]
    desc = json.load(open(exp / "equilibrium_noise.json"))
    assert desc["options"]["noise"] == eq.NOISE_DEFAULTS and desc["n_cells"] == 21
    assert [(r["group"], r["agent"]) for r in desc["summary"]] == [(0, 0), (0, 1), (0, None), (1, 0), (1, 1), (1, None)]
    assert all(r["games"] == G // 2 for r in desc["summary"]) and all(r["capped"] == 0 for r in desc["summary"] if r["agent"] is not None)
    g = eq.load_noise_games(str(exp))
    gb = GameBatch(noisy, n_games=G).load(str(exp / "batch.pt"))
    direct = gb.equilibrium_noise(policies=True)
    _same(g, direct, INT + FLOAT + WEIGHTED + CELL + ("noise_prob",))
    again = eq.summarize_noise(g, np.arange(G) % 2, 2, [0, 1], 0.0)
    assert desc["summary"] == json.loads(json.dumps(again))
    df = utils.equilibrium_noise_summary(str(exp))
    assert len(df) == 6 and df.loc[0, "n_cells"] == 21
    gm = utils.equilibrium_noise_games(str(exp), agent=1)
    assert gm.index.tolist() == list(range(G))
    _bits_equal(gm["loss_w"].to_numpy(), g["loss_w"][1])


def test_sharded_launch_with_noise_equal_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 21
    noisy = dict(SMALL, environment=dict(ENV, noise_prob=0.05))
    cfg = dict(noisy, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "n_groups": 2,
                                "groups": [g % 2 for g in range(G)], "equilibrium": {"policies": True, "noise": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    for name in ("equilibrium.json", "equilibrium_noise.json"):
        assert json.load(open(tmp_path / "one" / name)) == json.load(open(tmp_path / "two" / name)), name
    files = sorted(f.name for f in (tmp_path / "one").iterdir() if f.name.startswith(("eq_", "eqn_")))
    assert {"eqn_iters.npy", "eqn_loss.npy", "eqn_prob.npy", "eqn_weighted.npy", "eqn_policy.npy"} <= set(files)
    for f in files:
        _bits_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f), f)
    a, b = utils.equilibrium_noise_games(str(tmp_path / "one")), utils.equilibrium_noise_games(str(tmp_path / "two"))
    assert a.index.tolist() == b.index.tolist() == list(range(G))
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
