"""Greedy play under demand noise on the device (thrl_stationary, GameBatch.stationary, training.stationary): iters,
change, mass, stat_reward, stat_action, stat_price and pi bit-equal to the numpy mirror (tests/stationary_mirror.py:
the same recurrence with an explicit ascending loop over the source cells) on fresh and trained headline tables in f32
and f64 (J = 101: two cells per lane, one of them masked), a 20-state config (J = 21: most lanes idle), individual
grids with a max_state below a, the 3,000-state config (indexing; 16 steps), per-game noise probabilities with two bad
entries, the start from the training state, a given policy with no tables, a convergence tracker's policy, a game
count below the batch's and more games than resident blocks; the known answers through set_tables; the mass identity;
and the invariances (training state, game order, shard split, MixedGameBatch, the trainer's artefacts, a sharded
launch)."""
import ctypes
import json

import numpy as np
import pytest

import deviation_mirror as M
import stationary_mirror as S

pytestmark = pytest.mark.gpu

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
SMALL = {"agents": [dict(AG, states=20), dict(AG, states=20, gamma=0.9)], "environment": dict(ENV)}
THREE = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=11, states=60, action_range=[0.2, 0.4], min_memory=10, gamma=0.9),
                    dict(AG, actions=5, states=40, action_range=[0.0, 0.3], min_memory=10, max_state=8)],
         "environment": dict(ENV, nplayers=3, max_steps=40)}
BIG = {"agents": [dict(AG, states=3000), dict(AG, states=3000)], "environment": dict(ENV)}
FIELDS = ("iters", "change", "mass", "stat_reward", "stat_action", "stat_price", "pi")
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


def _batch(config, G, dtype="float32", seed=3, episodes=0):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, seed=seed).init_tables()
    if episodes:
        gb.run(episodes, logs=False)
    return gb


def _identity(out):
    """|mass - 1| <= iters * (J + 2) ulp: a step adds J products per cell and halves twice, the mass sums J cells."""
    ok = out["iters"] > 0
    err = np.abs(out["mass"][ok] - 1.0)
    bound = out["iters"][ok] * (out["n_cells"] + 2) * 2.0 ** -52
    print("max |mass - 1| = %.3e (bound of that game %.3e)" % (err.max(), bound[err.argmax()]))
    assert (err <= bound).all()
    assert (out["mass"][~ok] == 0).all()


def _check(gb, config, noise_prob=0.05, n_games=None, policy=None, start="reset", state0=None, **kw):
    out = gb.stationary(noise_prob=noise_prob, pi=True, n_games=n_games, policy=policy, start=start, state0=state0, **kw)
    pol = S.policies(config, gb.tables_numpy()) if policy is None else policy.cpu().numpy().view(np.uint16)
    s0 = None if start == "reset" else (gb.states_numpy() if state0 is None else state0)
    ref = S.iterate(config, _tabs(config), pol, noise_prob, state0=s0, n_games=n_games,
                    tol=kw.get("tol", 1e-12), max_iters=kw.get("max_iters", 8192))
    for f in FIELDS:
        _bits_equal(out[f], ref[f], f)
    _identity(out)
    return out


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("episodes", [0, 200])
def test_headline_matches_mirror(dtype, episodes):
    gb = _batch(TWO, 139, dtype, seed=11, episodes=episodes)           # 139: no multiple of a wave or a block
    out = _check(gb, TWO)
    assert out["n_cells"] == 101
    assert (out["iters"] > 0).all() and (out["iters"] < 8192).all()   # all converged: what test_stationary_host holds


def test_20_state_config_most_lanes_idle():
    gb = _batch(SMALL, 70, seed=4, episodes=30)
    out = _check(gb, SMALL)
    assert out["n_cells"] == 21


def test_three_agents_individual_grids_clipped_prices():
    gb = _batch(THREE, 48, seed=5, episodes=50)
    out = _check(gb, THREE)
    assert out["n_cells"] > 64
    _check(gb, THREE, noise_prob=0.5, start="state", state0=np.linspace(0.0, 9.99, 48))


def test_3000_state_config_indexing():
    gb = _batch(BIG, 4, seed=6, episodes=20)
    out = _check(gb, BIG, max_iters=16)
    assert out["n_cells"] == 3001 and (out["iters"] == 16).all()


def test_per_game_noise_with_bad_entries():
    G = 12
    gb = _batch(TWO, G, seed=7, episodes=60)
    p = np.array([0.01, 0.05, 0.0, 0.5, 1.0, np.nan, 0.05, 0.01, 1.0, 0.5, 0.05, 0.2])
    out = _check(gb, TWO, noise_prob=p)
    bad = np.array([2, 5])
    assert (out["iters"][bad] == -1).all() and (np.delete(out["iters"], bad) > 0).all()
    for f in ("change", "mass", "stat_price"):
        assert (out[f][bad] == 0).all()
    assert (out["stat_reward"][:, bad] == 0).all() and (out["stat_action"][:, bad] == 0).all() and (out["pi"][bad] == 0).all()
    # the neighbours are what a scalar call gives them
    one = gb.stationary(noise_prob=0.05, pi=True)
    for g in (1, 6, 10):
        for f in FIELDS:
            _bits_equal(np.asarray(out[f])[..., g] if f != "pi" else out[f][g],
                        np.asarray(one[f])[..., g] if f != "pi" else one[f][g], f)
    # the batch's own sweep array is the default
    gb.set_sweep({"noise_prob": np.where(np.isfinite(p) & (p > 0), p, 0.3)})
    own = gb.stationary(pi=True)
    _bits_equal(own["noise_prob"], np.where(np.isfinite(p) & (p > 0), p, 0.3))
    _bits_equal(own["pi"][0], out["pi"][0])


def test_start_state():
    gb = _batch(TWO, 70, seed=8, episodes=100)
    out = _check(gb, TWO, start="state")
    s0 = np.random.RandomState(2).uniform(0, 10, gb.G)
    s0[3] = 10.5                                                       # past a: the rows clamp to the last cell's
    out = _check(gb, TWO, start="state", state0=s0)
    assert (out["iters"] > 0).all()


def test_policy_given_reads_no_table_and_tracker_policy():
    import torch
    from th_rl_amd import _lib, crossplay as xp
    G = 40
    gb = _batch(TWO, G, seed=9, episodes=100)
    want = gb.stationary(noise_prob=0.05, pi=True)
    pol = xp.extract(gb)
    got = _check(gb, TWO, policy=pol)
    for f in FIELDS:
        _bits_equal(got[f], want[f], f)
    # q = NULL through the library itself
    from th_rl_amd import stationary as sn
    tabs = _tabs(TWO)
    dev = gb.device
    a = _lib.StationaryArgs()
    a.n_games, a.flags, a.n_cells, a.band_w = G, _lib.STAT_POLICY_GIVEN, tabs["n_cells"], tabs["band_w"]
    a.max_iters, a.tol, a.noise_prob = 8192, 1e-12, 0.05
    keep = {f: torch.from_numpy(np.ascontiguousarray(tabs[f])).to(dev)
            for f in ("cell_rows", "cell_w", "det_cell", "band_lo", "band", "noise_reward", "noise_price")}
    outs = {"iters": torch.zeros(G, dtype=torch.int32, device=dev)}
    outs.update({f: torch.zeros(G, dtype=torch.float64, device=dev) for f in ("change", "mass", "stat_price")})
    outs.update({f: torch.zeros((2, G), dtype=torch.float64, device=dev) for f in ("stat_reward", "stat_action")})
    for f, t in list(keep.items()) + list(outs.items()):
        setattr(a, f, t.data_ptr())
    a.policy = pol.data_ptr()
    assert gb.L.thrl_stationary(ctypes.byref(gb.cfg), None, ctypes.byref(a), gb._stream()) == 0
    torch.cuda.synchronize(dev)
    for f, t in outs.items():
        _bits_equal(t.cpu().numpy(), want[f], f)
    # entries that are no action are clamped to the last action
    bad = pol.clone()
    bad[:, 5] = 30000
    _check(gb, TWO, policy=bad)
    # a convergence tracker's policy is analysed as it is
    tr = gb.track_convergence(window=5)
    got = gb.stationary(noise_prob=0.05, pi=True, policy=tr.policy)
    for f in FIELDS:
        _bits_equal(got[f], want[f], f)


def test_fewer_games_than_the_batch_and_more_than_resident_blocks():
    import torch
    gb = _batch(SMALL, 77, seed=10, episodes=20)
    whole = gb.stationary(noise_prob=0.5, pi=True)
    part = _check(gb, SMALL, noise_prob=0.5, n_games=30)
    for f in FIELDS:
        _bits_equal(part[f], whole[f][..., :30] if f != "pi" else whole[f][:30], f)
    # more games than blocks the device keeps resident: every block loops over games
    cus = torch.cuda.get_device_properties(gb.device).multi_processor_count
    G = cus * 32 + 77
    big = _batch(SMALL, G, seed=12)
    out = big.stationary(noise_prob=0.5, max_iters=64)
    pol = S.policies(SMALL, big.tables_numpy())
    tail = np.r_[0:40, G - 120:G]
    ref = S.iterate(SMALL, _tabs(SMALL), pol[tail], 0.5, max_iters=64)
    for f in FIELDS[:-1]:
        _bits_equal(np.asarray(out[f])[..., tail], ref[f], f)
    _identity(out)


# ------------------------------------------------------------------------------------------------ known answers
def _one_hot(config, actions, G):
    """[G, stride] tables whose greedy action is actions[i] in every row of agent i."""
    ag, _, _ = M.params(config)
    parts = []
    for p, a in zip(ag, actions):
        t = np.zeros((p["states"] + 1, p["actions"]))
        t[:, a] = 1.0
        parts.append(t.ravel())
    return np.tile(np.concatenate(parts)[None, :], (G, 1))


@pytest.mark.parametrize("noise_prob", [0.05, 1.0])
def test_constant_policies_known_answer(noise_prob):
    """Every cell plays the same tuple t, so every row of P is q e_det + p n(t, .): that row is the distribution after
    one step and for ever, and the lazy iterate reaches it geometrically (the distance halves per step)."""
    from th_rl_amd.batched import GameBatch
    import equilibrium_mirror as E
    tabs, pl = _tabs(TWO), E.plan(TWO)
    acts = [(14, 12), (3, 17), (20, 0)]
    q = np.concatenate([_one_hot(TWO, a, 1) for a in acts])
    gb = GameBatch(TWO, n_games=3, dtype="float64", seed=1).set_tables(q, np.full(3, 5.0))
    out = _check(gb, TWO, noise_prob=noise_prob, tol=0.0, max_iters=80)     # past the 53 halvings of the distance
    p, qq = noise_prob, 1.0 - noise_prob
    n = S.full_band(tabs)
    for g, (a0, a1) in enumerate(acts):
        t = a0 * 21 + a1
        want = p * n[t]
        want[tabs["det_cell"][t]] += qq
        ulp = (out["iters"][g] + 2) * 2.0 ** -52
        err = np.abs(out["pi"][g] - want).max()
        print("game %d: iters %d, max |pi - row| = %.3e (bound %.3e)" % (g, out["iters"][g], err, ulp))
        assert err <= ulp
        for i in range(2):
            r = qq * pl["rew"][i][t] + p * tabs["noise_reward"][i][t]
            rel = abs(out["stat_reward"][i, g] - r) / abs(r)
            print("game %d agent %d: |stat_reward - (q r + p noise_reward)| / |.| = %.3e (bound %.3e)" % (g, i, rel, ulp))
            assert rel <= ulp


def test_planted_pair_of_cells():
    """Two cells whose deterministic successors are each other and whose bands never leave the pair (hand-made tables
    in place of the config's): from a start on the pair the mass splits as the direct solve says."""
    tabs = dict(_tabs(SMALL))
    J, T = tabs["n_cells"], tabs["n_tuples"]
    gb = _batch(SMALL, 5, "float64", seed=2)
    pol = S.policies(SMALL, gb.tables_numpy())
    tup = S.cell_tuples(SMALL, pol, tabs, 5)
    ka, kb = 7, 8
    det, blo = np.array(tabs["det_cell"]), np.array(tabs["band_lo"])
    band = np.array(tabs["band"])
    for g in range(5):
        ta, tb = tup[g, ka], tup[g, kb]
        if ta == tb:
            continue
        det[ta], det[tb] = kb, ka
        blo[ta] = blo[tb] = ka
        band[ta], band[tb] = 0.0, 0.0
        band[ta, :2] = (0.25, 0.75)
        band[tb, :2] = (0.5, 0.5)
    tabs.update(det_cell=det, band_lo=blo, band=band)
    from th_rl_amd import stationary as sn
    s0 = np.full(5, ka * 10.0 / 20)                                    # the centre of cell ka
    assert (S.start_cells(SMALL, tabs, s0) == ka).all()
    out = sn.run(gb, noise_prob=0.3, start="state", state0=s0, pi=True, tabs=tabs)
    ref = S.iterate(SMALL, tabs, pol, 0.3, state0=s0)
    sol = S.solve(SMALL, tabs, pol, 0.3, state0=s0)
    for f in FIELDS:
        _bits_equal(out[f], ref[f], f)
    done = 0
    for g in range(5):
        if tup[g, ka] == tup[g, kb]:
            continue
        done += 1
        assert abs(out["pi"][g, ka] + out["pi"][g, kb] - 1.0) <= 1e-12 and sol["classes"][g] >= 1
        assert np.abs(out["pi"][g] - sol["pi"][g]).sum() <= 1e-9
    assert done >= 1


# ------------------------------------------------------------------------------------------------ invariances
def test_invariances_state_order_shards_mixed():
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    from th_rl_amd import stationary as sn
    G = 64
    gb = _batch(TWO, G, seed=13, episodes=50)
    want = gb.stationary(noise_prob=0.05, pi=True)
    q = gb.tables_numpy()
    # the training state does not enter a start from the reset distribution
    gb.state.fill_(1.25)
    got = gb.stationary(noise_prob=0.05, pi=True)
    for f in FIELDS:
        _bits_equal(got[f], want[f], f)
    # game order
    perm = np.random.RandomState(1).permutation(G)
    gp = GameBatch(TWO, n_games=G, dtype="float32", seed=1).set_tables(q[perm], np.full(G, 5.0))
    got = gp.stationary(noise_prob=0.05, pi=True)
    for f in FIELDS:
        _bits_equal(got[f], np.asarray(want[f])[..., perm] if f != "pi" else want[f][perm], f)
    # shard split
    parts = []
    for lo, hi in ((0, 23), (23, 64)):
        gs = GameBatch(TWO, n_games=hi - lo, dtype="float32", seed=1, game_offset=lo).set_tables(q[lo:hi], np.full(hi - lo, 5.0))
        parts.append(gs.stationary(noise_prob=0.05, pi=True))
    both = sn.combine(parts)
    for f in FIELDS:
        _bits_equal(both[f], want[f], f)
    # MixedGameBatch, all QTable
    mb = MixedGameBatch(TWO, n_games=G, dtype="float32").set_tables(q, np.full(G, 5.0))
    got = mb.stationary(noise_prob=0.05, pi=True)
    for f in FIELDS:
        _bits_equal(got[f], want[f], f)


def test_train_one_stationary_artefacts_and_readers(tmp_path):
    from th_rl_amd import trainer, utils, stationary as sn
    from th_rl_amd.batched import GameBatch
    G = 48
    cfg = dict(TWO, training={"epochs": 10, "print_freq": 500, "seed": 21, "n_games": G, "n_groups": 2,
                              "groups": [g % 2 for g in range(G)], "attractors": True,
                              "stationary": {"noise_prob": 0.05, "pi": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "stationary.json"))
    assert desc["options"] == dict(sn.DEFAULTS, noise_prob=0.05, pi=True) and desc["n_cells"] == 101
    assert [r["games"] for r in desc["summary"]] == [G // 2] * 2
    assert all(r["converged"] == 1.0 and r["noise_cost_mean"] is not None for r in desc["summary"])
    g = sn.load_games(str(exp))
    assert g["pi"].shape == (G, 101) and (g["noise_prob"] == 0.05).all()
    gb = GameBatch(TWO, n_games=G).load(str(exp / "batch.pt"))
    ref = S.iterate(TWO, _tabs(TWO), S.policies(TWO, gb.tables_numpy()), 0.05)
    for f in FIELDS:
        _bits_equal(g[f], ref[f], f)
    nash, cartel = sn.optimal(TWO)
    again = sn.summarize(g, np.arange(G) % 2, 2, nash, cartel, 8192, reset_reward=np.load(exp / "attr_reset_reward.npy"))
    assert desc["summary"] == json.loads(json.dumps(again))
    df = utils.stationary_summary(str(exp))
    assert len(df) == 2 and df.loc[0, "n_cells"] == 101
    gm = utils.stationary_games(str(exp))
    assert gm.index.tolist() == list(range(G)) and "delta_reset" in gm.columns
    _bits_equal(gm["reward_1"].to_numpy(), g["stat_reward"][1])


def test_sharded_launch_stationary_equal_single_process(tmp_path):
    from th_rl_amd import trainer, utils
    from th_rl_amd.launch import launch
    G = 37
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 500, "seed": 17, "n_games": G, "n_groups": 2,
                              "groups": [g % 2 for g in range(G)], "attractors": True,
                              "stationary": {"noise_prob": 0.2, "pi": True}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    assert json.load(open(tmp_path / "one" / "stationary.json")) == json.load(open(tmp_path / "two" / "stationary.json"))
    for f in ("stat_iters", "stat_games", "stat_reward", "stat_action", "stat_pi"):
        _bits_equal(np.load(tmp_path / "one" / (f + ".npy")), np.load(tmp_path / "two" / (f + ".npy")), f)
    a, b = utils.stationary_games(str(tmp_path / "one")), utils.stationary_games(str(tmp_path / "two"))
    assert a.index.tolist() == b.index.tolist() == list(range(G))
    for c in a.columns:
        assert np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=True), c
