"""Sampled play on the device (thrl_price_probs, thrl_sampled_chain, MixedGameBatch.sampled_play, training.sampled_play):
the probabilities bit-equal to thrl_nn_act / thrl_ac_act's prob_out; the chain bit-equal to the numpy mirror
(tests/sampled_mirror.py) in every output for every shape, start and epsilon mode, for one game, in halves and at the edge
of the working-set plan; with no mirror in between, one step against a product computed in torch, and an all-QTable batch
at epsilon = 0 against thrl_tuple_walk's cycle means; the trainer's artefacts.

The random networks carry the coverage (tests/test_sampled_host.py asserts on the mirror that their chains concentrate
and that their rows are peaked in part of the games)."""
import json

import numpy as np
import pytest

import sampled_mirror as SPM
from sampled_mirror import AG, CAC, CASES, ENV, RF, RR, SHIP, WIDE

pytestmark = pytest.mark.gpu

OUT = ("iters", "change", "mass", "samp_reward", "samp_action", "samp_price", "agree", "pi")


def _bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.astype(np.float64).view(np.uint64).ravel())
        assert bad.size == 0, (what, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, np.flatnonzero(a != b)[:5])


def _mixed(config, n_games, seed=3):
    from th_rl_amd.mixed import MixedGameBatch
    return MixedGameBatch(config, n_games=n_games, dtype="float32", seed=seed).init_tables()


def _dev(mb, x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(mb.state.device)


def _case(name):
    """(batch, tabs, probs on the device, probs as numpy, dpolicy, eps [N, G] with bad entries, start with -1 and T) of
    CASES[name]: the random networks of the host test evaluated by thrl_price_probs."""
    def make():
        from th_rl_amd import sampled_play as sp
        config, T, n_games, _, seed = CASES[name]
        tabs = sp.tables(config)
        mb = _mixed(config, n_games)
        for i, w in SPM.case_weights(name, tabs).items():
            mb.nn[i].set_params(w)
        probs = sp.price_probs(mb, tabs["dprice"])
        host = {i: p.cpu().numpy() for i, p in probs.items()}
        pol = SPM.greedy_of(host, tabs, np.random.RandomState(seed + 100), n_games)
        eps = SPM.case_epsilon(name, tabs)
        eps[0, 7], eps[0, 11] = np.nan, 1.5                               # agent 0 is a QTable agent in every case
        return mb, tabs, probs, host, pol, eps, SPM.case_starts(name, tabs)
    return SPM.cached(("device case", name), make)


def _ref(name, key, **kw):
    mb, tabs, probs, host, pol, eps, start = _case(name)
    return SPM.cached(("device ref", name, key), lambda: SPM.analyse(tabs, host, pol, **kw))


def _run(name, eps, start, max_iters, sl=slice(None), tol=1e-12):
    mb, tabs, probs, host, pol, _, _ = _case(name)
    n = len(range(*sl.indices(pol.shape[0])))
    return mb.sampled_play(epsilon=eps, start="uniform" if start is None else start, tol=tol, max_iters=max_iters, pi=True,
                           n_games=n, probs={i: p[sl].contiguous() for i, p in probs.items()}, dpolicy=_dev(mb, pol[sl]),
                           tabs=tabs)


# ------------------------------------------------------------------------------------------------ the probabilities
@pytest.mark.parametrize("A", [2, 5, 21, 32])
@pytest.mark.parametrize("kind", ["Reinforce", "ActorCritic"])
def test_price_probs_are_the_act_kernels_prob_out(kind, A):
    from th_rl_amd import sampled_play as sp
    from test_gpu_tuple_attractors import _kinked_weights
    config = {"agents": [dict(AG, actions=3), dict(RF, name=kind, actions=A)], "environment": dict(ENV)}
    rs = np.random.RandomState(7 * A + len(kind))
    for n_games in (1, 203):                                              # one wave; 203 is no multiple of 4
        mb = _mixed(config, n_games)
        rb = mb.nn[1]
        rb.set_params(_kinked_weights(rs, n_games, A, rb.P, 0.0, 10.0))
        for J in (1, 130):                                                # 130: more than two passes of 64 prices
            x = rs.uniform(0.0, 10.0, J)
            got = sp.price_probs(mb, x)
            assert sorted(got) == [1] and tuple(got[1].shape) == (n_games, J, A)
            got = got[1].cpu().numpy()
            for k in range(J):
                _, want = rb.act(np.full(n_games, x[k]), want_probs=True)
                assert np.array_equal(got[:, k].view(np.uint32), want.cpu().numpy().view(np.uint32)), (n_games, J, k)
            assert (np.abs(got.sum(axis=2) - 1.0) < 1e-5).all()
    part = sp.price_probs(mb, x[:5], n_games=6)[1]
    assert np.array_equal(part.cpu().numpy(), got[:6, :5])


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", ["QQ", "QR", "QRA", "SHIP"])
def test_the_chain_equals_the_mirror(name):
    mb, tabs, probs, host, pol, eps, start = _case(name)
    config, T, n_games, max_iters, _ = CASES[name]
    bad_eps = np.zeros(n_games, bool)
    bad_eps[[7, 11]] = True
    bad_start = np.zeros(n_games, bool)
    bad_start[[2, 5]] = True
    # per-game epsilon, uniform start
    out = _run(name, eps, None, max_iters)
    ref = _ref(name, "uniform", eps=eps, tol=1e-12, max_iters=max_iters)
    for f in OUT:
        _bits_equal(out[f], ref[f], "%s uniform %s" % (name, f))
    assert (out["iters"][bad_eps] == -1).all() and not out["pi"][bad_eps].any() and not out["agree"][bad_eps].any()
    assert (out["iters"][~bad_eps] >= 1).all() and (np.abs(out["mass"][~bad_eps] - 1.0) < 1e-12).all()
    _bits_equal(out["epsilon"], eps, "epsilon")
    print("%s: iters %d..%d, at the cap %.2f, agree %.3f..%.3f, LDS %d bytes"
          % (name, out["iters"][~bad_eps].min(), out["iters"].max(), np.mean(out["iters"] == max_iters),
             out["agree"][~bad_eps].min(), out["agree"].max(), out["lds_bytes"]))
    # start tuples with -1 and T mixed in; the shipped shape on its first 64 games
    n = 64 if name == "SHIP" else n_games
    out = _run(name, eps[:, :n], start[:n], max_iters, slice(0, n))
    ref = SPM.cached(("device ref", name, "tuple"), lambda: SPM.analyse(
        tabs, {i: p[:n] for i, p in host.items()}, pol[:n], eps[:, :n], start=start[:n], tol=1e-12, max_iters=max_iters))
    for f in OUT:
        _bits_equal(out[f], ref[f], "%s tuple %s" % (name, f))
    bad = (bad_eps | bad_start)[:n]
    assert (out["iters"][bad] == -1).all() and (out["iters"][~bad] >= 1).all() and np.array_equal(out["start"], start[:n])
    # scalar epsilon: one number, and one per agent
    if name != "SHIP":
        for e in (0.0, [0.25] + [0.5] * (mb.N - 1)):
            out = _run(name, e, None, 16)
            ref = SPM.analyse(tabs, host, pol, [e] * mb.N if np.ndim(e) == 0 else e, tol=1e-12, max_iters=16)
            for f in OUT:
                _bits_equal(out[f], ref[f], "%s eps=%s %s" % (name, e, f))


@pytest.mark.parametrize("name", ["QRA", "QQ"])
def test_one_game_and_the_batch_in_halves(name):
    mb, tabs, probs, host, pol, eps, start = _case(name)
    config, T, n_games, max_iters, _ = CASES[name]
    whole = _run(name, eps, start, max_iters)
    h = n_games // 2
    parts = [_run(name, eps[:, :h], start[:h], max_iters, slice(0, h)), _run(name, eps[:, h:], start[h:], max_iters, slice(h, n_games))]
    from th_rl_amd import sampled_play as sp
    both = sp.combine(parts)
    for f in OUT + ("start", "epsilon"):
        _bits_equal(both[f], whole[f], "halves %s" % f)
    one = _run(name, eps[:, 8:9], start[8:9], max_iters, slice(8, 9))
    for f in OUT:
        _bits_equal(one[f], whole[f][8:9] if f == "pi" else whole[f][..., 8:9], "one game %s" % f)
    ref = SPM.analyse(tabs, {i: p[8:9] for i, p in host.items()}, pol[8:9], eps[:, 8:9], start=start[8:9], max_iters=max_iters)
    for f in OUT:
        _bits_equal(one[f], ref[f], "one game, mirror %s" % f)


@pytest.mark.parametrize("trained", [False, True])
def test_the_shipped_pairing_extracted_on_the_device(trained):
    """Everything from the batch itself: thrl_nn_init's networks and the QTable agent's own tables, fresh and after 20
    episodes, the probabilities, the greedy entries and epsilon taken by run()."""
    from th_rl_amd import sampled_play as sp, tuple_stationary as ts
    n = 64
    mb = _mixed(dict(SHIP, environment=dict(ENV, max_steps=20)), n, seed=21)
    if trained:
        mb.run(20, per_game_logs=False)
    tabs = sp.tables(mb.config)
    out = mb.sampled_play(max_iters=12, pi=True)
    host = {i: p.cpu().numpy() for i, p in sp.price_probs(mb, tabs["dprice"]).items()}
    pol = ts.price_policy(mb, tabs["dprice"]).cpu().numpy().view(np.uint16)
    ref = SPM.analyse(tabs, host, pol, list(mb.eps)[:2], max_iters=12)
    for f in OUT:
        _bits_equal(out[f], ref[f], "trained=%s %s" % (trained, f))
    assert (out["iters"] == 12).all() and (out["T"], out["n_prices"]) == (441, 441)
    state = mb.sampled_play(start="state", max_iters=12, pi=True)
    t0 = np.asarray(state["start"])
    ref = SPM.analyse(tabs, host, pol, list(mb.eps)[:2], start=t0, max_iters=12)
    for f in OUT:
        _bits_equal(state[f], ref[f], "trained=%s state %s" % (trained, f))
    assert (t0 >= 0).all() if trained else (t0 == -1).all()               # a fresh reset's price is no tuple's price


def test_current_epsilon_of_a_swept_batch_is_its_per_game_array():
    """epsilon="current" on a batch with an epsilon sweep: the device array [N, G] is what the chain reads, per game."""
    from sampled_mirror import QR
    from th_rl_amd import sampled_play as sp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    n = 12
    eps = np.random.RandomState(33).uniform(0.0, 0.6, (2, n))
    mb = MixedGameBatch(QR, n_games=n, dtype="float32", seed=5)
    mb.set_sweep({"eps": eps})
    mb.init_tables()
    tabs = sp.tables(QR)
    host = {i: p.cpu().numpy() for i, p in sp.price_probs(mb, tabs["dprice"]).items()}
    pol = ts.price_policy(mb, tabs["dprice"]).cpu().numpy().view(np.uint16)
    for k in (n, 5):
        out = mb.sampled_play(max_iters=24, pi=True, n_games=k)
        _bits_equal(out["epsilon"], mb.sweep["eps"].cpu().numpy()[:, :k], "epsilon")
        _bits_equal(out["epsilon"], eps[:, :k], "epsilon given")
        ref = SPM.analyse(tabs, {i: p[:k] for i, p in host.items()}, pol[:k], eps[:, :k], max_iters=24)
        for f in OUT:
            _bits_equal(out[f], ref[f], "sweep %s" % f)
    flat = mb.sampled_play(epsilon=float(eps[0, 0]), max_iters=24)
    assert flat["samp_price"][0] == out["samp_price"][0] and (flat["samp_price"][1:5] != out["samp_price"][1:5]).any()


# ------------------------------------------------------------------------------------------------ the edge of the plan
def _edge(aq):
    return {"agents": [dict(AG, actions=aq), dict(RF, actions=32)], "environment": dict(ENV)}


def test_the_largest_accepted_shape_and_the_first_refused():
    """A 32-action network against a QTable: the working set grows with the tuples and with the distinct prices, which
    depend on how the two grids align.  The heaviest working set working_set() accepts (30 QTable actions, T = D = 960,
    1,136 bytes under a CU's LDS), the last count before the first refusal (31) and the largest count accepted at all (many
    tuples on few prices) are solved and equal the mirror; the first refused count is refused from its shape alone."""
    from th_rl_amd import sampled_play as sp
    from th_rl_amd._lib import ThrlError
    fits = [aq for aq in range(2, 129) if sp.working_set(_edge(aq))["fits"]]
    top = max(fits)
    first_refused = min(aq for aq in range(2, 129) if aq not in fits)
    heaviest = max(fits, key=lambda aq: sp.working_set(_edge(aq))["bytes"])
    print("accepted up to %d actions (%d bytes), the heaviest accepted %d (%d bytes), the first refused %d (%d bytes)"
          % (top, sp.working_set(_edge(top))["bytes"], heaviest, sp.working_set(_edge(heaviest))["bytes"], first_refused,
             sp.working_set(_edge(first_refused))["bytes"]))
    assert first_refused == 32 and heaviest == 30 and top > first_refused
    assert sp.MAX_LDS - 2048 < sp.working_set(_edge(heaviest))["bytes"] <= sp.MAX_LDS
    rs = np.random.RandomState(81)
    for aq in sorted({top, heaviest, first_refused - 1}):
        config = _edge(aq)
        tabs = sp.tables(config)
        mb = _mixed(config, 2)
        mb.nn[1].set_params(SPM.random_weights(rs, 2, 32, "Reinforce", tabs["price"].min(), tabs["price"].max()))
        probs = sp.price_probs(mb, tabs["dprice"])
        host = {1: probs[1].cpu().numpy()}
        pol = SPM.greedy_of(host, tabs, rs, 2)
        for start in (None, np.array([tabs["n_tuples"] - 1, 0], np.int32)):
            out = mb.sampled_play(epsilon=[0.1, 0.0], start="uniform" if start is None else start, max_iters=4, pi=True,
                                  probs=probs, dpolicy=_dev(mb, pol), tabs=tabs)
            ref = SPM.analyse(tabs, host, pol, [0.1, 0.0], start=start, max_iters=4)
            for f in OUT:
                _bits_equal(out[f], ref[f], "A_q=%d %s" % (aq, f))
            assert out["iters"].tolist() == [4, 4]
    mb = _mixed(_edge(first_refused), 2)
    with pytest.raises(ThrlError, match="bytes of LDS") as e:
        mb.sampled_play(max_iters=4)
    assert e.value.code == -3


# ------------------------------------------------------------------------------------------------ without the mirror
def test_one_step_from_a_unit_mass_is_the_product_of_the_act_kernels_rows():
    """RR: two networks.  One step from the unit mass on t is 0.5 [t' = t] + 0.5 prod_i p_i(a_i(t')) / prod_i sum(p_i) with
    p_i = thrl_nn_act's prob_out at price[t]; the product and the division differ from the device's in the order of a
    handful of roundings: relative 2^-49."""
    import torch
    from th_rl_amd import sampled_play as sp
    n = 203
    tabs = sp.tables(RR)
    assert tabs["n_prices"] == 41
    mb = _mixed(RR, n)
    rs = np.random.RandomState(91)
    for i, rb in mb.nn.items():
        rb.set_params(SPM.random_weights(rs, n, 21, "Reinforce", tabs["price"].min(), tabs["price"].max()))
    start = rs.randint(0, 441, n).astype(np.int32)
    out = mb.sampled_play(start=start, max_iters=1, pi=True)
    p = [mb.nn[i].act(tabs["price"][start], want_probs=True)[1].to(torch.float64) for i in range(2)]
    s = (p[0][:, :, None] * p[1][:, None, :]).reshape(n, 441) / (p[0].sum(dim=1) * p[1].sum(dim=1))[:, None]
    want = 0.5 * s
    want = want.cpu().numpy()
    want[np.arange(n), start] += 0.5
    diff = np.abs(out["pi"] - want)
    print("one step: largest relative difference %.3g (2^-49 = %.3g), %.2f of the entries are 0"
          % ((diff[want > 0] / want[want > 0]).max(), 2.0 ** -49, np.mean(want == 0)))
    assert (diff <= 2.0 ** -49 * want).all() and np.mean(want > 0) > 0.5
    assert (out["iters"] == 1).all() and abs(out["mass"] - 1.0).max() < 1e-14


CYC = {"agents": [dict(AG, actions=5), dict(AG, actions=5, alpha=0.3, gamma=0.9)], "environment": dict(ENV, max_steps=20)}


def test_all_qtable_at_epsilon_zero_earns_the_greedy_cycle():
    """An all-QTable GameBatch at epsilon = 0 is a deterministic map: from the state's tuple the lazy chain ends on the
    greedy cycle thrl_tuple_walk finds, and on a cycle of length lam <= 4 reached within mu <= 16 steps its error after
    512 steps is below cos(pi / 4)^400: samp_reward equals cycle_reward within 1e-9 max |reward|."""
    from th_rl_amd import sampled_play as sp, tuple_play as tp
    from th_rl_amd.batched import GameBatch
    n = 203
    gb = GameBatch(CYC, n_games=n, dtype="float32", seed=11).init_tables()
    gb.run(40, logs=False)
    tabs = sp.tables(CYC)
    walk = tp.run(gb, tabs=tabs)
    ok = (walk["mu"] >= 0) & (walk["mu"] <= 16) & (walk["lam"] >= 1) & (walk["lam"] <= 4)
    print("greedy cycles: %.2f of the games have lam <= 4 and mu <= 16 (lam up to %d, mu up to %d)"
          % (ok.mean(), walk["lam"].max(), walk["mu"].max()))
    assert ok.mean() >= 0.25
    out = gb.sampled_play(epsilon=0.0, start="state", max_iters=512, tol=0.0)
    assert np.array_equal(out["start"], walk["start"]) and (out["iters"][ok] >= 1).all()
    top = np.abs(tabs["reward"]).max()
    err = np.abs(out["samp_reward"] - walk["cycle_reward"])[:, ok].max()
    print("largest difference to the cycle means %.3g (bound %.3g)" % (err, 1e-9 * top))
    assert err <= 1e-9 * top
    assert (np.abs(out["agree"][ok] - 1.0) < 1e-12).all() and len(set(out["samp_price"][ok].tolist())) > 1


# ------------------------------------------------------------------------------------------------ refusals, trainer
def test_refusals_and_validation():
    from test_sampled_host import check_validation
    from th_rl_amd import _lib
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.mixed import MixedGameBatch
    check_validation(_lib.load())
    with pytest.raises(ValueError, match="4096"):
        MixedGameBatch(WIDE, n_games=4).init_tables().sampled_play()
    with pytest.raises(ValueError, match="continuous"):
        MixedGameBatch(CAC, n_games=4).init_tables().sampled_play()
    with pytest.raises(ThrlError, match="init_tables"):
        MixedGameBatch(SHIP, n_games=4).sampled_play()
    mb = _mixed(SHIP, 8)
    for bad in (dict(epsilon=1.5), dict(epsilon="final"), dict(epsilon=[0.1]), dict(start="reset"), dict(n_games=9),
                dict(start=np.zeros(3, np.int32)), dict(max_iters=0), dict(tol=-1.0)):
        with pytest.raises(ThrlError):
            mb.sampled_play(**bad)
    out = mb.sampled_play(max_iters=50)
    assert (out["iters"] >= 1).all() and "pi" not in out and (out["epsilon"][0] == mb.eps[0]).all()


def test_train_one_artefacts(tmp_path):
    from th_rl_amd import sampled_play as sp, trainer, utils
    from th_rl_amd.mixed import MixedGameBatch
    n = 64
    base = dict(SHIP, environment=dict(ENV, max_steps=20))
    cfg = dict(base, training={"epochs": 5, "print_freq": 500, "seed": 19, "n_games": n, "greedy_cycles": True,
                               "sampled_play": True})
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "sampled_play.json"))
    assert desc["options"] == sp.DEFAULTS and desc["T"] == 441 and desc["n_prices"] == 441
    assert json.loads(json.dumps(desc)) == desc and len(desc["summary"]) == 1 and desc["summary"][0]["games"] == n
    assert (exp / "greedy_cycles.json").exists() and not (exp / "splay_pi.npy").exists()
    assert np.load(exp / "splay_iters.npy").shape == (n,) and np.load(exp / "splay_games.npy").shape == (4, n)
    mb = MixedGameBatch(base, n_games=n).load(str(exp / "batch.pt"))
    direct = mb.sampled_play()
    saved = sp.load_games(str(exp))
    for f in OUT[:-1] + ("epsilon",):
        _bits_equal(saved[f], direct[f], f)
    games = utils.sampled_play_games(str(exp))
    assert games.index.tolist() == list(range(n)) and games["iters"].tolist() == direct["iters"].tolist()
    for col, f in (("change", "change"), ("mass", "mass"), ("price", "samp_price"), ("agree", "agree")):
        _bits_equal(games[col].to_numpy(), direct[f], col)
    for i in range(2):
        _bits_equal(games["reward_%d" % i].to_numpy(), direct["samp_reward"][i], "reward")
        _bits_equal(games["action_%d" % i].to_numpy(), direct["samp_action"][i], "action")
    assert (np.abs(games["mass"].to_numpy() - 1.0) <= 1e-9).all()
    assert ((games["agree"].to_numpy() >= 0.0) & (games["agree"].to_numpy() <= 1.0)).all()
    assert np.isfinite(games["delta_sampled"].to_numpy()).all()
    summ = utils.sampled_play_summary(str(exp))
    assert len(summ) == 1 and summ["T"][0] == 441 and summ["n_prices"][0] == 441
    assert {"converged", "iters_q50", "delta_sampled_mean", "agree_mean", "price_mean", "delta_greedy_mean",
            "randomness_cost_mean"} <= set(summ.columns)
    assert np.isfinite(summ["randomness_cost_mean"][0])
    print("sampled play after 5 episodes: delta_sampled %.4f, delta_greedy %.4f, agree %.3f, iters up to %d"
          % (summ["delta_sampled_mean"][0], summ["delta_greedy_mean"][0], summ["agree_mean"][0], games["iters"].max()))
    with pytest.raises(KeyError):
        utils.sampled_play_games(str(tmp_path))
    (tmp_path / "cac.json").write_text(json.dumps(dict(CAC, training={"epochs": 1, "n_games": 4, "sampled_play": True})))
    with pytest.raises(ValueError, match="continuous"):
        trainer.train_one(str(tmp_path / "cac"), str(tmp_path / "cac.json"))
