"""Best responses to sampled play on the device (thrl_sampled_response, MixedGameBatch.sampled_response,
training.sampled_play.response): every output bit-equal to the numpy mirror (tests/sampled_response_mirror.py) on every
shape and argument mode, for one game, in halves and at the edge of the working-set plan; the unsolved games of each kind
beside solved neighbours; with no new code in between, an all-QTable batch at epsilon = 0 against greedy_equilibrium; the
trainer's artefacts.  A handful of games per case: the mirror solves one (agent, game) at a time."""
import json
import os

import numpy as np
import pytest

import sampled_mirror as SPM
import sampled_response_mirror as SRM
from sampled_mirror import AG, ENV, QQ, QR, QRA, RF, RR, SHIP

pytestmark = pytest.mark.gpu

OUT = ("iters", "sweeps", "n_diff", "loss_all", "loss_mean")
WEIGHTED = ("loss_w", "gain_w", "v_w", "br_prob_w")
POL = ("br_policy", "v_opt", "v_pi")
# (config, games, seed, gamma: None = the agents' own)
CASES = {"QQ": (QQ, 5, 21, None), "QR": (QR, 4, 22, None), "QRA": (QRA, 3, 23, None), "RR": (RR, 1, 24, None),
         "SHIP": (SHIP, 3, 25, 0.5)}


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


def _inputs(config, n_games, seed):
    """(batch, tabs, probs on the device, probs as numpy, dpolicy, eps [N, G], pi [G, T]): random networks evaluated by
    thrl_price_probs, the networks' dpolicy entries their rows' first maxima, the QTable entries random with some at or
    above the action count."""
    from th_rl_amd import sampled_play as sp
    tabs = sp.tables(config)
    mb = _mixed(config, n_games)
    rs = np.random.RandomState(seed)
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            mb.nn[i].set_params(SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, tabs["price"].min(), tabs["price"].max()))
    probs = sp.price_probs(mb, tabs["dprice"])
    host = {i: p.cpu().numpy() for i, p in probs.items()}
    pol = SPM.greedy_of(host, tabs, rs, n_games)
    eps = rs.uniform(0.0, 0.2, (len(tabs["kinds"]), n_games))
    pi = rs.dirichlet(np.ones(int(tabs["n_tuples"])), n_games)
    return mb, tabs, probs, host, pol, eps, pi


def _case(name):
    config, n_games, seed, _ = CASES[name]
    return SPM.cached(("response case", name), lambda: _inputs(config, n_games, seed))


def _run(case, sl=slice(None), **kw):
    mb, tabs, probs, host, pol, eps, pi = case
    n = len(range(*sl.indices(pol.shape[0])))
    return mb.sampled_response(n_games=n, probs={i: p[sl].contiguous() for i, p in probs.items()}, dpolicy=_dev(mb, pol[sl]),
                               tabs=tabs, **kw)


def _same(out, ref, fields, what):
    for f in fields:
        _bits_equal(out[f], ref[f], "%s %s" % (what, f))


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", ["QQ", "QR", "QRA", "RR", "SHIP"])
def test_the_device_equals_the_mirror(name):
    case = _case(name)
    mb, tabs, probs, host, pol, eps, pi = case
    config, G, _, gamma = CASES[name]
    N = mb.N
    own = SRM.own_gammas(config) if gamma is None else [gamma] * N
    # per-game epsilon, the given pi, the policies; gamma as the case has it (None: the agents' own from the batch)
    out = _run(case, epsilon=eps, gamma=gamma, pi=pi, policies=True)
    ref = SPM.cached(("response ref", name), lambda: SRM.analyse(tabs, host, pol, eps, own, pi=pi))
    _same(out, ref, OUT + WEIGHTED + POL, name)
    assert (out["iters"] >= 0).all() and out["agents"] == list(range(N))
    _bits_equal(out["gamma"], np.repeat(np.asarray(own)[:, None], G, axis=1), "gamma")
    _bits_equal(out["epsilon"], eps, "epsilon")
    assert ((out["br_prob_w"] >= 0.0) & (out["br_prob_w"] <= 1.0 + 1e-6)).all() and (out["gain_w"] > -1e-9).all()
    print("%s: iters %d..%d, sweeps %d..%d, n_diff up to %d of %d, loss_all up to %.3g, LDS %d bytes"
          % (name, out["iters"].min(), out["iters"].max(), out["sweeps"].min(), out["sweeps"].max(), out["n_diff"].max(),
             out["n_prices"], out["loss_all"].max(), out["lds_bytes"]))
    # without pi: the weighted outputs are absent, the others the same bits
    bare = _run(case, epsilon=eps, gamma=gamma, pi=False)
    assert not any(f in bare for f in WEIGHTED + POL)
    _same(bare, ref, OUT, name + " no pi")
    if name == "SHIP":
        return
    # a subset of the agents, per-game gamma, scalar epsilon; the other agents' entries stay zero
    sub = [N - 1]
    gam_g = np.random.RandomState(7).uniform(0.3, 0.7, (N, G))
    part = _run(case, agents=sub, epsilon=0.125, gamma=gam_g, pi=pi, policies=True)
    want = SRM.analyse(tabs, host, pol, 0.125, gam_g, agents=sub, pi=pi)
    _same(part, want, OUT + WEIGHTED + POL, name + " subset")
    assert not part["sweeps"][0].any() and not part["v_opt"][0].any()
    # pi computed by the call itself is sampled_play's
    auto = _run(case, epsilon=0.125, gamma=0.5)
    sp_pi = mb.sampled_play(epsilon=0.125, pi=True, probs=probs, dpolicy=_dev(mb, pol), tabs=tabs)["pi"]
    _bits_equal(auto["pi"], sp_pi, "pi")
    _same(auto, SRM.analyse(tabs, host, pol, 0.125, 0.5, pi=sp_pi), OUT + WEIGHTED, name + " own pi")


@pytest.mark.parametrize("name", ["QQ", "QRA"])
def test_one_game_and_the_batch_in_halves(name):
    case = _case(name)
    mb, tabs, probs, host, pol, eps, pi = case
    G = pol.shape[0]
    gam_g = np.random.RandomState(8).uniform(0.3, 0.7, (mb.N, G))
    whole = _run(case, epsilon=eps, gamma=gam_g, pi=pi, policies=True)
    h = G // 2
    for sl in (slice(0, h), slice(h, G), slice(G - 1, G)):
        part = _run(case, sl, epsilon=eps[:, sl], gamma=gam_g[:, sl], pi=pi[sl], policies=True)
        for f in OUT + WEIGHTED + POL:
            _bits_equal(part[f], whole[f][:, sl], "%s %s %s" % (name, sl, f))


# ------------------------------------------------------------------------------------------------ unsolved games
def test_unsolved_games_write_what_the_header_says_and_leave_their_neighbours_alone():
    case = _case("QR")
    mb, tabs, probs, host, pol, eps, pi = case
    G, N, D = pol.shape[0], mb.N, int(tabs["n_prices"])
    clean = _run(case, epsilon=eps, gamma=0.5, pi=pi, policies=True)
    # a bad epsilon refuses game 1 for both agents; a gamma of 1.0 leaves (agent 1, game 2) unsolved
    bad_eps = eps.copy()
    bad_eps[0, 1] = 1.5
    gam = np.full((N, G), 0.5)
    gam[1, 2] = 1.0
    out = _run(case, epsilon=bad_eps, gamma=gam, pi=pi, policies=True)
    _same(out, SRM.analyse(tabs, host, pol, bad_eps, gam, pi=pi), OUT + WEIGHTED + POL, "unsolved")
    assert (out["iters"][:, 1] == -1).all() and not out["sweeps"][:, 1].any()
    for f in ("loss_all", "loss_mean") + WEIGHTED + POL:
        assert not out[f][:, 1].any(), f
    assert out["iters"][1, 2] == -1 and out["sweeps"][1, 2] == 0 and out["n_diff"][1, 2] == 0
    for f in ("loss_all", "loss_mean") + WEIGHTED:
        assert np.isnan(out[f][1, 2]), f
    assert np.isnan(out["v_opt"][1, 2]).all() and np.isnan(out["v_pi"][1, 2]).all()
    assert np.array_equal(out["br_policy"][1, 2], host[1][2].argmax(axis=1))          # the modal action
    ok = np.ones((N, G), bool)
    ok[:, 1], ok[1, 2] = False, False
    for f in OUT + WEIGHTED + POL:
        _bits_equal(out[f][ok], clean[f][ok], "neighbours " + f)
    # max_sweeps = 3 caps the one (agent, game) whose gamma is not 0: gamma = 0 settles in two sweeps
    gam = np.zeros((N, G))
    gam[0, 3] = 0.9
    cap = _run(case, epsilon=eps, gamma=gam, max_sweeps=3, pi=pi, policies=True)
    _same(cap, SRM.analyse(tabs, host, pol, eps, gam, max_sweeps=3, pi=pi), OUT + WEIGHTED + POL, "capped")
    assert cap["iters"][0, 3] == -1 and cap["sweeps"][0, 3] == 3 and np.isnan(cap["loss_all"][0, 3])
    assert np.array_equal(cap["br_policy"][0, 3], np.minimum(pol[3, 0], 1))
    ok = np.ones((N, G), bool)
    ok[0, 3] = False
    assert (cap["iters"][ok] >= 0).all() and not np.isnan(cap["loss_w"][ok]).any()


# ------------------------------------------------------------------------------------------------ against older code
def test_deterministic_rivals_give_greedy_equilibriums_best_response_values():
    """An all-QTable batch at epsilon = 0 has deterministic rivals, so V*(row(t)) is thrl_tuple_equilibrium's V*(t), a
    solver that predates this one (evaluation by doubling, exact to 2^-64).  Tolerance: this solver's stopping bound
    gamma eval_tol / (1 - gamma) -- the other's is 0 -- plus a rounding allowance of four times the largest excess over
    that bound between the two CPU mirrors on the same strategies (tuple_equilibrium_mirror against
    sampled_response_mirror); the device enters neither."""
    import tuple_equilibrium_mirror as EM
    from th_rl_amd import sampled_play as sp
    from th_rl_amd import tuple_play as tp
    config = {"agents": [dict(AG, actions=5), dict(AG, actions=4, gamma=0.9)], "environment": dict(ENV)}
    G = 4
    mb = _mixed(config, G, seed=5)
    tabs = sp.tables(config)
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    given = tp.extract(mb, tabs)
    ge = mb.greedy_equilibrium(policies=True, tuple_policy=given, start=np.zeros(G, np.int32))
    out = mb.sampled_response(epsilon=0.0, pi=False, policies=True, tabs=tabs)
    assert (ge["iters"] >= 0).all() and (out["iters"] >= 0).all()
    pol = given.cpu().numpy().view(np.uint16)
    rep = np.asarray(tabs["grp_perm"])[np.asarray(tabs["grp_first"])[:-1]]
    gam = np.array([0.95, 0.9])
    m_old = EM.analyse(tabs, pol, np.zeros(G, np.int64), gamma=gam, policies=True)
    m_new = SRM.analyse(tabs, {}, pol[:, :, rep], 0.0, gam)
    row = np.asarray(tabs["row"])
    for i in range(2):
        bound = gam[i] * 1e-12 / (1.0 - gam[i])
        excess = max(0.0, np.abs(m_new["v_opt"][i][:, row] - m_old["v_opt"][i]).max() - bound)
        err = np.abs(out["v_opt"][i][:, row] - ge["v_opt"][i]).max()
        print("agent %d: device difference %.3g, bound %.3g, CPU mirrors' excess %.3g" % (i, err, bound, excess))
        assert err <= bound + 4.0 * excess, (i, err, bound, excess)


# ------------------------------------------------------------------------------------------------ the working set
def test_the_largest_accepted_working_set_and_the_first_refused_shape():
    """The working set is not monotone in the action counts (the distinct prices D are not): of QTable A x Reinforce B
    for A in 20..35 and B in 24..32 the heaviest shape the plan accepts is 33 x 30 (T = 990, D = 842: 163,616 of 163,840
    bytes), solved here for one game at gamma 0 and equal to the mirror; the lightest it refuses is 26 x 32 (T = D = 832:
    165,392 bytes), THRL_ERR_UNSUPPORTED without a launch."""
    from th_rl_amd import _lib
    from th_rl_amd import sampled_play as sp
    from th_rl_amd import sampled_response as sr
    from th_rl_amd._lib import ThrlError

    def cfg(A, B):
        return {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}
    ws, over = sr.working_set(cfg(33, 30)), sr.working_set(cfg(26, 32))
    assert ws == dict(bytes=163616, T=990, D=842, team=1, fits=True) and ws["bytes"] <= sr.MAX_LDS
    assert over == dict(bytes=165392, T=832, D=832, team=1, fits=False)
    case = _inputs(cfg(33, 30), 1, 31)
    mb, tabs, probs, host, pol, eps, pi = case
    out = _run(case, epsilon=eps, gamma=0.0, pi=pi, policies=True)
    assert out["lds_bytes"] == ws["bytes"]
    _same(out, SRM.analyse(tabs, host, pol, eps, 0.0, pi=pi), OUT + WEIGHTED + POL, "largest")
    # the next shape: refused by the library from the shape alone (no tensor is valid, none is touched)
    mb2 = _mixed(cfg(26, 32), 1)
    tabs2 = sp.tables(cfg(26, 32))
    with pytest.raises(ThrlError) as e:
        mb2.sampled_response(tabs=tabs2, pi=False)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a = _lib.SampledResponseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.agents, a.max_sweeps = 1, 832, 832, 3, 8
    a.kind[1] = 1
    assert mb2.L.thrl_sampled_response(mb2.cfg, a, None) == _lib.ERR_UNSUPPORTED
    assert b"165392 bytes of LDS per game" in mb2.L.thrl_last_error()


# ------------------------------------------------------------------------------------------------ the trainer
def test_train_one_writes_the_response_beside_sampled_play(tmp_path):
    from th_rl_amd import utils
    from th_rl_amd.trainer import train_one
    base = {"agents": [dict(AG, actions=3, states=10), dict(RF, actions=3)], "environment": dict(ENV, max_steps=10)}
    runs = {}
    for key, extra in (("plain", {}), ("resp", {"response": {"policies": True, "max_sweeps": 8192}})):
        cfg = dict(base, training={"epochs": 4, "print_freq": 500, "seed": 3, "n_games": 6,
                                   "sampled_play": dict({"pi": True}, **extra)})
        (tmp_path / (key + ".json")).write_text(json.dumps(cfg))
        train_one(str(tmp_path / key), str(tmp_path / (key + ".json")))
        runs[key] = str(tmp_path / key)
    files = sorted(os.listdir(runs["resp"]))
    for f in ("sampled_response.json", "sresp_counts.npy", "sresp_loss.npy", "sresp_weighted.npy", "sresp_gamma.npy",
              "sresp_epsilon.npy", "sresp_br_policy.npy", "sresp_v_opt.npy", "sresp_v_pi.npy"):
        assert f in files, (f, files)
    assert not any(f.startswith("sresp") or f == "sampled_response.json" for f in os.listdir(runs["plain"]))
    for f in sorted(os.listdir(runs["plain"])):
        if f.startswith("splay_"):
            assert open(os.path.join(runs["plain"], f), "rb").read() == open(os.path.join(runs["resp"], f), "rb").read(), f
    desc = json.load(open(os.path.join(runs["resp"], "sampled_response.json")))
    assert desc["options"]["policies"] is True and desc["agents"] == [0, 1]
    assert "response" not in json.load(open(os.path.join(runs["resp"], "sampled_play.json")))["options"]
    summary = utils.sampled_response_summary(runs["resp"])
    games = utils.sampled_response_games(runs["resp"])
    assert len(games) == 6 and (games["iters_0"] >= 0).all() and (games["iters_1"] >= 0).all()
    assert set(summary["agent"].dropna().astype(int)) == {0, 1} and "nashconv_mean" in summary.columns
    assert np.isfinite(games["exploit_0"]).all() and (games["nashconv"] > -1e-9).all()
