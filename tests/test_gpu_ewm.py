"""Smoothed learning curves on the device (thrl_ewm_rows, group_stats.Smoother, training.group_stats.smooth): the
kernel against its numpy restatement (group_stats.ewm_host, the same float64 operations) bit for bit, in place and
out of place, with the state carried across calls; every episode path's out["group_stats_smooth"] against the
reduction of the smoothed rows of the same run, with the raw statistics identical to a run without smoothing; the
trainer's artefacts against pandas' ewm; a sharded launch against the single process."""
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
GRIDS = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=21, states=100, action_range=[0.2, 0.4], min_memory=10, alpha=0.3, gamma=0.9)],
         "environment": dict(ENV, max_steps=40)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _eq(a, b):
    for k in ("hist", "sums", "minmax"):
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape, k
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(L, rew, act, E, decay, den, state_in, state_out, out=None):
    """thrl_ewm_rows as it is, on device tensors: (return code, den after)."""
    from th_rl_amd import _lib
    a = _lib.EwmRowsArgs()
    a.n_games, a.n_agents, a.n_episodes = rew.shape[2], rew.shape[1], int(E)
    a.decay, a.den = decay, den
    a.reward_rows, a.action_rows = rew.data_ptr(), act.data_ptr()
    o_r, o_a = (rew, act) if out is None else out
    a.reward_out, a.action_out = o_r.data_ptr(), o_a.data_ptr()
    a.state_in = None if state_in is None else state_in.data_ptr()
    a.state_out = state_out.data_ptr()
    d = ctypes.c_double(-1.0)
    a.den_out = ctypes.pointer(d)
    return L.thrl_ewm_rows(ctypes.byref(a), _stream()), d.value


# ------------------------------------------------------------------------------------------------ kernel alone
@pytest.mark.parametrize("N,G,E", [(1, 1, 1), (2, 65, 7), (3, 257, 12), (2, 64, 0)])
def test_kernel_matches_numpy_mirror(N, G, E):
    import torch
    from th_rl_amd import _lib
    from th_rl_amd.group_stats import ewm_decay, ewm_host
    L = _lib.load()
    rs = np.random.RandomState(100 * N + G + E)
    R = max(E, 1)                                               # (an empty tensor has no address)
    r, a = rs.uniform(-1.0, 26.0, (R, N, G)), rs.uniform(0.0, 1.0, (R, N, G))
    h = 3.0
    _, d = ewm_decay(h)
    want_r, want_a, want_s, want_den = ewm_host(r[:E], a[:E], h)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    marker = np.full((2 * N, G), 7.25)

    # out of place, state_in NULL
    rt, at, o_r, o_a, s = dev(r), dev(a), dev(np.zeros_like(r)), dev(np.zeros_like(a)), dev(marker)
    rc, den = _call(L, rt, at, E, d, 0.0, None, s, out=(o_r, o_a))
    torch.cuda.synchronize()
    assert rc == 0 and den == want_den
    assert _bits(o_r.cpu().numpy()[:E], want_r) and _bits(o_a.cpu().numpy()[:E], want_a)
    assert _bits(rt.cpu().numpy(), r) and _bits(at.cpu().numpy(), a)            # the inputs are left alone
    if E == 0:          # a no-op: nothing written, the denominator as it was
        assert _bits(s.cpu().numpy(), marker) and _bits(o_r.cpu().numpy(), np.zeros_like(r))
        rc, den = _call(L, rt, at, 0, d, 2.5, None, s)
        assert rc == 0 and den == 2.5
        return
    assert _bits(s.cpu().numpy(), want_s)

    # in place, state_in an explicit zeros buffer that is also state_out
    rt, at, s = dev(r), dev(a), dev(np.zeros((2 * N, G)))
    rc, den = _call(L, rt, at, E, d, 0.0, s, s)
    torch.cuda.synchronize()
    assert rc == 0 and den == want_den
    assert _bits(rt.cpu().numpy(), want_r) and _bits(at.cpu().numpy(), want_a) and _bits(s.cpu().numpy(), want_s)

    # two calls with the state carried (5 + 7 of 12): the same bits, through the Smoother and by hand
    if E >= 2:
        from th_rl_amd.group_stats import Smoother
        k = 5 * E // 12
        sm = Smoother(N, G, h, "cuda")
        rt, at = dev(r), dev(a)
        sm.apply(L, rt[:k], at[:k], k, _stream())
        sm.apply(L, rt[k:], at[k:], E - k, _stream())
        torch.cuda.synchronize()
        assert sm.rows == E and sm.den == want_den and _bits(sm.state.cpu().numpy(), want_s)
        assert _bits(rt.cpu().numpy(), want_r) and _bits(at.cpu().numpy(), want_a)
        rt, at, s0, s1 = dev(r), dev(a), dev(marker), dev(marker)
        rc, den = _call(L, rt[:k], at[:k], k, d, 0.0, None, s0)
        rc2, den = _call(L, rt[k:], at[k:], E - k, d, den, s0, s1)                 # state_out another buffer
        torch.cuda.synchronize()
        assert rc == 0 and rc2 == 0 and den == want_den and _bits(s1.cpu().numpy(), want_s)
        assert _bits(rt.cpu().numpy(), want_r) and _bits(at.cpu().numpy(), want_a)


def test_kernel_non_finite_values_stay():
    import torch
    from th_rl_amd import _lib
    from th_rl_amd.group_stats import Smoother, ewm_host
    N, G, E = 2, 70, 9
    rs = np.random.RandomState(3)
    r, a = rs.uniform(0, 25, (E, N, G)), rs.uniform(0, 1, (E, N, G))
    r[2, 0, 5], r[4, 1, 69], a[0, 0, 0] = np.nan, np.inf, -np.inf
    want_r, want_a, _, _ = ewm_host(r, a, 8.0)
    rt, at = torch.from_numpy(r).cuda(), torch.from_numpy(a).cuda()
    Smoother(N, G, 8.0, "cuda").apply(_lib.load(), rt, at, E, _stream())
    got_r, got_a = rt.cpu().numpy(), at.cpu().numpy()
    assert np.array_equal(np.isnan(got_r), np.isnan(want_r)) and np.array_equal(np.isnan(got_a), np.isnan(want_a))
    assert np.isnan(got_r[2:, 0, 5]).all() and not np.isfinite(got_r[4:, 1, 69]).any()
    assert np.array_equal(got_r, want_r, equal_nan=True) and np.array_equal(got_a, want_a, equal_nan=True)


# ------------------------------------------------------------------------------------------------ episode paths
G_RUN, E_RUN, H_RUN = 96, 6, 3.0


def _spec(config):
    from th_rl_amd.group_stats import GroupSpec, resolve_ranges
    ids = (np.arange(G_RUN) % 3).astype(np.int32)
    return GroupSpec(len(config["agents"]), ids, 3, resolve_ranges(config), bins=64), ids


def _check_runs(make, run, kernel=None):
    """Two launches of E_RUN episodes with one Smoother, three ways: with the rows, without them, and without
    smoothing."""
    from th_rl_amd.group_stats import Smoother, ewm_host, merge, reduce_host
    a, b, c = make(), make(), make()
    spec, ids = _spec(a.config)
    sa, sc = Smoother(a.N, G_RUN, H_RUN, a.device), Smoother(a.N, G_RUN, H_RUN, a.device)
    oa = [run(a, per_game_logs=True, group_stats=spec, smooth=sa) for _ in range(2)]
    ob = [run(b, per_game_logs=True, group_stats=spec) for _ in range(2)]
    oc = [run(c, per_game_logs=False, group_stats=spec, smooth=sc) for _ in range(2)]
    if kernel is not None:
        assert oa[0]["kernel"] == kernel, oa[0]["kernel"]
    rew = np.concatenate([o["game_reward_log"] for o in oa])
    act = np.concatenate([o["game_action_log"] for o in oa])
    assert rew.shape == (2 * E_RUN, a.N, G_RUN)
    s_r, s_a, state, den = ewm_host(rew, act, H_RUN)
    assert _bits(np.concatenate([o["game_reward_smooth"] for o in oa]), s_r)
    assert _bits(np.concatenate([o["game_action_smooth"] for o in oa]), s_a)
    assert sa.rows == 2 * E_RUN and sa.den == den and _bits(sa.state.cpu().numpy(), state)
    want = reduce_host(s_r, s_a, ids, 3, spec.describe())
    for outs in (oa, oc):
        got = {k: np.concatenate([o["group_stats_smooth"][k] for o in outs]) for k in ("hist", "sums", "minmax")}
        _eq(got, want)
    for x, y, z in zip(oa, ob, oc):         # smoothing changes nothing else
        _eq(x["group_stats"], y["group_stats"])
        _eq(z["group_stats"], y["group_stats"])
        assert _bits(x["game_reward_log"], y["game_reward_log"]) and _bits(x["game_action_log"], y["game_action_log"])
        assert "group_stats_smooth" not in y and "game_reward_smooth" not in y
    assert np.array_equal(a.tables_numpy(), b.tables_numpy()) and np.array_equal(c.tables_numpy(), b.tables_numpy())


@pytest.mark.parametrize("label,config,kernel", [("generic", TWO, "generic"), ("wave", TWO, "wave"),
                                                 ("tuple", GRIDS, "tuple")], ids=["generic", "wave", "tuple"])
def test_gamebatch_smoothed_statistics(label, config, kernel):
    from th_rl_amd.batched import GameBatch
    make = lambda: GameBatch(config, n_games=G_RUN, dtype="float32", kernel=kernel, seed=11).init_tables()
    _check_runs(make, lambda gb, **kw: gb.run(E_RUN, **kw), kernel=label)


def test_gamebatch_device_outputs_and_keep_games():
    """sync=False returns device tensors (the raw rows stay, the smoothed ones beside them); keep_games selects the
    columns of both."""
    import torch
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import Smoother, ewm_host, to_numpy
    make = lambda: GameBatch(TWO, n_games=G_RUN, dtype="float32", kernel="wave", seed=11).init_tables()
    a, b = make(), make()
    spec, ids = _spec(TWO)
    oa = a.run(E_RUN, per_game_logs=True, group_stats=spec, smooth=Smoother(2, G_RUN, H_RUN, a.device), sync=False)
    keep = torch.tensor([5, 17, 95], device=b.device)
    ob = b.run(E_RUN, per_game_logs=True, keep_games=keep, group_stats=spec, smooth=Smoother(2, G_RUN, H_RUN, b.device))
    torch.cuda.synchronize()
    rew, act = oa["game_reward_log"].cpu().numpy(), oa["game_action_log"].cpu().numpy()
    s_r, s_a, _, _ = ewm_host(rew, act, H_RUN)
    assert _bits(oa["game_reward_smooth"].cpu().numpy(), s_r) and _bits(oa["game_action_smooth"].cpu().numpy(), s_a)
    _eq(to_numpy(oa["group_stats_smooth"]), ob["group_stats_smooth"])
    assert _bits(ob["game_reward_log"], rew[:, :, [5, 17, 95]]) and _bits(ob["game_reward_smooth"], s_r[:, :, [5, 17, 95]])
    assert _bits(ob["game_action_smooth"], s_a[:, :, [5, 17, 95]])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_mixed_smoothed_statistics(fused):
    from th_rl_amd.mixed import MixedGameBatch
    make = lambda: MixedGameBatch(MIXED, n_games=G_RUN, dtype="float32", seed=5).init_tables()

    def run(mb, per_game_logs, **kw):
        if fused:
            return mb.run(E_RUN, fused=True, per_game_logs=per_game_logs, **kw)
        return mb.run(E_RUN, fused=False, **kw)
    _check_runs(make, run)


def test_run_refuses_a_smoother_it_cannot_use():
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import Smoother
    gb = GameBatch(TWO, n_games=G_RUN, dtype="float32", seed=1).init_tables()
    with pytest.raises(ThrlError, match="group_stats or per_game_logs"):
        gb.run(2, smooth=Smoother(2, G_RUN, 3.0, gb.device))
    with pytest.raises(ThrlError, match="smoother is for"):
        gb.run(2, per_game_logs=True, smooth=Smoother(2, G_RUN + 1, 3.0, gb.device))
    assert gb.episode == 0


# ------------------------------------------------------------------------------------------------ trainer, launch
def _rel(got, want):
    diff, mag = np.abs(got - want), np.abs(want)
    return float(np.max(np.where(mag > 0, diff / np.where(mag > 0, mag, 1.0), np.where(diff == 0, 0.0, np.inf))))


def test_train_one_smoothed_artefacts(tmp_path):
    import pandas
    from th_rl_amd import trainer, utils
    from th_rl_amd.group_stats import ewm_decay, finalize, reduce_host
    G, epochs, h = 32, 24, 3
    training = {"epochs": epochs, "print_freq": 5, "seed": 8, "n_games": G, "groups": [g % 3 for g in range(G)],
                "game_logs": True}
    for name, opt in (("on", {"bins": 32, "histograms": True, "smooth": h}), ("off", {"bins": 32, "histograms": True})):
        (tmp_path / (name + ".json")).write_text(json.dumps(dict(TWO, training=dict(training, group_stats=opt))))
        trainer.train_one(str(tmp_path / name), str(tmp_path / (name + ".json")))
    on, off = tmp_path / "on", tmp_path / "off"
    fields = ("mean", "std", "min", "max", "quantiles", "sums", "hist")
    for f in fields:
        assert os.path.isfile(on / ("group_smooth_%s.npy" % f)), f
        assert not os.path.exists(off / ("group_smooth_%s.npy" % f))
        x, y = np.load(on / ("group_%s.npy" % f)), np.load(off / ("group_%s.npy" % f))
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f       # the raw statistics: as without smoothing
    assert not os.path.exists(off / "game_rewards_smooth.npy")
    desc, desc_off = json.load(open(on / "groups.json")), json.load(open(off / "groups.json"))
    assert desc["smooth"] == {"halflife": 3.0, "decay": ewm_decay(3.0)[1]} and "smooth" not in desc_off
    assert {k: v for k, v in desc.items() if k != "smooth"} == desc_off
    rew, act = np.load(on / "game_rewards.npy"), np.load(on / "game_actions.npy")
    assert _bits(rew, np.load(off / "game_rewards.npy")) and _bits(act, np.load(off / "game_actions.npy"))
    s_r, s_a = np.load(on / "game_rewards_smooth.npy"), np.load(on / "game_actions_smooth.npy")
    assert s_r.shape == rew.shape == (epochs, 2, G) and s_a.shape == act.shape
    # pandas per column: E = 24 rows of three roundings each, far inside 1e-13 (E * 2^-52 = 5.3e-15)
    for raw, sm in ((rew, s_r), (act, s_a)):
        want = pandas.DataFrame(raw.reshape(epochs, 2 * G)).ewm(halflife=h).mean().to_numpy().reshape(epochs, 2, G)
        err = _rel(sm, want)
        print("train_one smoothed rows vs pandas ewm(halflife=%d): max rel err %.3g" % (h, err))
        assert err <= 1e-13
    # one smoother for the whole run: print_freq 5 cuts the 24 epochs into launches, the curve does not see it
    ids = np.arange(G) % 3
    raw = reduce_host(s_r, s_a, ids, 3, desc)
    fin = finalize(raw, desc)
    for f in fields:
        want = raw[f] if f in ("sums", "hist") else fin[f]
        assert np.array_equal(np.load(on / ("group_smooth_%s.npy" % f)), want, equal_nan=f not in ("sums", "hist")), f
    df = utils.group_quantiles(str(on), 1, prefix="group_smooth")
    assert list(df.columns) == ["25th", "median", "75th", "Nash", "Cartel"] and len(df) == epochs
    assert np.array_equal(df["median"].to_numpy(), fin["quantiles"][:, 1, 4, 1])
    assert np.array_equal(utils.group_log(str(on), 2, prefix="group_smooth").to_numpy(), fin["mean"][:, 2, :4])
    gl = utils.game_log(str(on), 7, smooth=True).to_numpy()
    assert np.array_equal(gl, np.concatenate([s_r[:, :, 7], s_a[:, :, 7]], axis=1))


def test_sharded_launch_smoothed_equal_single_process(tmp_path):
    from th_rl_amd import trainer
    from th_rl_amd.launch import launch
    G = 33
    cfg = dict(TWO, training={"epochs": 6, "print_freq": 4, "seed": 17, "n_games": G,
                              "groups": [g % 3 for g in range(G)],
                              "group_stats": {"bins": 32, "histograms": True, "smooth": 3}})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    trainer.train_one(str(tmp_path / "one"), str(tmp_path / "c.json"))
    launch(str(tmp_path / "c.json"), str(tmp_path / "two"), gpus=2)
    for p in ("group_smooth", "group"):
        for f in ("sums", "hist", "min", "max", "quantiles", "mean", "std"):
            x = np.load(tmp_path / "one" / ("%s_%s.npy" % (p, f)))
            y = np.load(tmp_path / "two" / ("%s_%s.npy" % (p, f)))
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (p, f)
    assert json.load(open(tmp_path / "one" / "groups.json")) == json.load(open(tmp_path / "two" / "groups.json"))
