"""Best responses to sampled play under demand noise on the device (thrl_sampled_response_noise,
MixedGameBatch.sampled_response_noise, training.sampled_play.response with "noise"): every output bit-equal to the numpy
mirror (tests/sampled_response_noise_mirror.py) on every shape and argument mode, for one game, in halves and at the edge
of the working-set plan; the unsolved games of each kind beside solved neighbours; with no new code in between, an
all-QTable batch at epsilon = 0 against greedy_equilibrium_noise; the trainer's artefacts.  A handful of games per case:
the mirror solves one (agent, game) at a time."""
import json
import os

import numpy as np
import pytest

import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import sampled_response_noise_mirror as SRNM
from sampled_mirror import AG, ENV, QQ, QR, QRA, RF, RR, SHIP

pytestmark = pytest.mark.gpu

OUT = SRNM.INT + SRNM.FLOAT
WEIGHTED = SRNM.WEIGHTED
POL = ("br_policy", "v_opt", "v_pi")
EVAL_TOL = 1e-10
# (config, resolution, games, seed, gamma per agent).  RR has S = 50 states, fewer than the block has threads; three_agents
# and QRA take the generic product over the rivals; SHIP at resolution 16 has S = 554: more than two states per thread
CASES = {"QQ": (QQ, 8, 5, 31, [0.95, 0.9]), "QR": (QR, 8, 4, 32, [0.9, 0.95]), "QRA": (QRA, 12, 3, 33, [0.9, 0.8, 0.7]),
         "RR": (RR, 8, 3, 34, [0.9, 0.95]), "three": (SNM.three_agents(), 8, 3, 35, [0.8, 0.9, 0.7]),
         "SHIP": (SHIP, 16, 3, 36, [0.5, 0.5])}


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


def _inputs(config, resolution, n_games, seed):
    """dict(mb, tabs, probs / nprobs on the device and as numpy, pol, npol, eps [N, G], p [G] in (0.01, 0.5], pi [G, T]):
    random networks evaluated by thrl_price_probs at the distinct prices and at the nodes, the networks' policy entries their
    rows' first maxima, the QTable entries random with some at or above the action count."""
    from th_rl_amd import sampled_play as sp
    tabs = sp.noise_tables(config, resolution)
    mb = _mixed(config, n_games)
    rs = np.random.RandomState(seed)
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            mb.nn[i].set_params(SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, 0.0, float(tabs["price"].max())))
    probs, nprobs = sp.price_probs(mb, tabs["dprice"]), sp.price_probs(mb, tabs["xn"])
    host = {i: x.cpu().numpy() for i, x in probs.items()}
    nhost = {i: x.cpu().numpy() for i, x in nprobs.items()}
    pol = SPM.greedy_of(host, tabs, rs, n_games)
    npol = SPM.greedy_of(nhost, SNM.node_tabs(tabs), rs, n_games)
    N, T = len(tabs["kinds"]), int(tabs["n_tuples"])
    return dict(mb=mb, tabs=tabs, probs=probs, nprobs=nprobs, host=host, nhost=nhost, pol=pol, npol=npol,
                eps=rs.uniform(0.0, 0.2, (N, n_games)), p=rs.uniform(0.01, 0.5, n_games), pi=rs.dirichlet(np.ones(T), n_games))


def _case(name):
    config, resolution, n_games, seed, _ = CASES[name]
    return SPM.cached(("response noise case", name), lambda: _inputs(config, resolution, n_games, seed))


def _run(c, sl=slice(None), eval_tol=EVAL_TOL, **kw):
    mb = c["mb"]
    n = len(range(*sl.indices(c["pol"].shape[0])))
    cut = lambda d: {i: x[sl].contiguous() for i, x in d.items()}
    return mb.sampled_response_noise(n_games=n, probs=cut(c["probs"]), dpolicy=_dev(mb, c["pol"][sl]), nprobs=cut(c["nprobs"]),
                                     npolicy=_dev(mb, c["npol"][sl]), ntabs=c["tabs"], eval_tol=eval_tol, **kw)


def _mirror(c, eps, gamma, p, sl=slice(None), eval_tol=EVAL_TOL, **kw):
    cut = lambda d: {i: x[sl] for i, x in d.items()}
    return SRNM.analyse(c["tabs"], cut(c["host"]), c["pol"][sl], cut(c["nhost"]), c["npol"][sl], eps, gamma, p, eval_tol=eval_tol,
                        **kw)


def _same(out, ref, fields, what):
    for f in fields:
        _bits_equal(out[f], ref[f], "%s %s" % (what, f))


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_device_equals_the_mirror(name):
    c = _case(name)
    mb, tabs, eps, p, pi = c["mb"], c["tabs"], c["eps"], c["p"], c["pi"]
    _, _, G, _, gammas = CASES[name]
    N, S = mb.N, int(tabs["n_prices"]) + int(tabs["n_nodes"])
    # per-game epsilon and noise, the agents' gammas, the given pi, the policies
    out = _run(c, epsilon=eps, gamma=gammas, noise_prob=p, pi=pi, policies=True)
    ref = SPM.cached(("response noise ref", name), lambda: _mirror(c, eps, gammas, p, pi=pi))
    _same(out, ref, OUT + WEIGHTED + POL, name)
    assert (out["iters"] >= 0).all() and out["agents"] == list(range(N)) and out["v_opt"].shape == (N, G, S)
    _bits_equal(out["gamma"], np.repeat(np.asarray(gammas)[:, None], G, axis=1), "gamma")
    _bits_equal(out["epsilon"], eps, "epsilon")
    _bits_equal(out["noise_prob"], p, "noise_prob")
    assert ((out["br_prob_w"] >= 0.0) & (out["br_prob_w"] <= 1.0 + 1e-6)).all() and (out["gain_w"] > -1e-7).all()
    print("%s: S = %d, iters %d..%d, sweeps %d..%d, n_diff up to %d prices and %d nodes, loss_all up to %.3g, LDS %d bytes"
          % (name, S, out["iters"].min(), out["iters"].max(), out["sweeps"].min(), out["sweeps"].max(),
             out["n_diff_prices"].max(), out["n_diff_nodes"].max(), out["loss_all"].max(), out["lds_bytes"]))
    # without pi: the weighted outputs are absent, the others the same bits
    bare = _run(c, epsilon=eps, gamma=gammas, noise_prob=p, pi=False)
    assert not any(f in bare for f in WEIGHTED + POL)
    _same(bare, ref, OUT, name + " no pi")
    if name == "SHIP":
        return
    # a subset of the agents, per-game gamma, scalar epsilon and noise; the other agents' entries stay zero
    sub = [N - 1]
    gam_g = np.random.RandomState(7).uniform(0.3, 0.7, (N, G))
    part = _run(c, agents=sub, epsilon=0.125, gamma=gam_g, noise_prob=0.05, pi=pi, policies=True)
    want = _mirror(c, 0.125, gam_g, 0.05, agents=sub, pi=pi)
    _same(part, want, OUT + WEIGHTED + POL, name + " subset")
    assert not part["sweeps"][0].any() and not part["v_opt"][0].any()
    # pi computed by the call itself is sampled play's under the same noise
    auto = _run(c, epsilon=0.125, gamma=0.5, noise_prob=p)
    sp_pi = mb.sampled_play(epsilon=0.125, pi=True, probs=c["probs"], dpolicy=_dev(mb, c["pol"]), tabs=tabs, noise_prob=p,
                            nprobs=c["nprobs"], npolicy=_dev(mb, c["npol"]))["pi"]
    _bits_equal(auto["pi"], sp_pi, "pi")
    _same(auto, _mirror(c, 0.125, 0.5, p, pi=sp_pi), OUT + WEIGHTED, name + " own pi")
    w = np.stack([SRNM.weights(tabs, sp_pi[g], float(p[g])) for g in range(G)])
    assert np.abs(w.sum(axis=1) - 1.0).max() < 1e-9         # the long-run distribution of the deciding state


@pytest.mark.parametrize("name", ["QQ", "three"])
def test_one_game_and_the_batch_in_halves(name):
    c = _case(name)
    eps, p, pi = c["eps"], c["p"], c["pi"]
    G = c["pol"].shape[0]
    gam_g = np.random.RandomState(8).uniform(0.3, 0.7, (c["mb"].N, G))
    whole = _run(c, epsilon=eps, gamma=gam_g, noise_prob=p, pi=pi, policies=True)
    h = G // 2
    for sl in (slice(0, h), slice(h, G), slice(G - 1, G)):
        part = _run(c, sl, epsilon=eps[:, sl], gamma=gam_g[:, sl], noise_prob=p[sl], pi=pi[sl], policies=True)
        for f in OUT + WEIGHTED + POL:
            _bits_equal(part[f], whole[f][:, sl], "%s %s %s" % (name, sl, f))
        _bits_equal(part["noise_prob"], p[sl], "noise_prob")


# ------------------------------------------------------------------------------------------------ unsolved games
def test_unsolved_games_write_what_the_header_says_and_leave_their_neighbours_alone():
    c = _case("QR")
    mb, tabs, eps, p, pi = c["mb"], c["tabs"], c["eps"], c["p"], c["pi"]
    G, N, D = c["pol"].shape[0], mb.N, int(tabs["n_prices"])
    clean = _run(c, epsilon=eps, gamma=0.5, noise_prob=p, pi=pi, policies=True)
    # a bad epsilon refuses game 1 for both agents, a bad noise_prob game 3; a gamma of 1.0 leaves (agent 1, game 2) unsolved
    bad_eps, bad_p = eps.copy(), p.copy()
    bad_eps[0, 1], bad_p[3] = 1.5, 0.0
    gam = np.full((N, G), 0.5)
    gam[1, 2] = 1.0
    out = _run(c, epsilon=bad_eps, gamma=gam, noise_prob=bad_p, pi=pi, policies=True)
    _same(out, _mirror(c, bad_eps, gam, bad_p, pi=pi), OUT + WEIGHTED + POL, "unsolved")
    for g in (1, 3):
        assert (out["iters"][:, g] == -1).all() and not out["sweeps"][:, g].any()
        for f in SRNM.FLOAT + ("n_diff_prices", "n_diff_nodes") + WEIGHTED + POL:
            assert not out[f][:, g].any(), (f, g)
    assert out["iters"][1, 2] == -1 and out["sweeps"][1, 2] == 0 and out["n_diff_prices"][1, 2] == 0 and out["n_diff_nodes"][1, 2] == 0
    for f in SRNM.FLOAT + WEIGHTED:
        assert np.isnan(out[f][1, 2]), f
    assert np.isnan(out["v_opt"][1, 2]).all() and np.isnan(out["v_pi"][1, 2]).all()
    modal = np.concatenate([c["host"][1][2].argmax(axis=1), c["nhost"][1][2].argmax(axis=1)])
    assert np.array_equal(out["br_policy"][1, 2], modal)                              # the modal action, prices then nodes
    ok = np.ones((N, G), bool)
    ok[:, 1], ok[:, 3], ok[1, 2] = False, False, False
    for f in OUT + WEIGHTED + POL:
        _bits_equal(out[f][ok], clean[f][ok], "neighbours " + f)
    for bad in (np.nan, -0.1, 1.5):                      # every kind of bad noise_prob entry; 1.0 is a valid one
        bad_p = p.copy()
        bad_p[0], bad_p[2] = bad, 1.0
        o = _run(c, epsilon=eps, gamma=0.5, noise_prob=bad_p, pi=False)
        assert (o["iters"][:, 0] == -1).all() and (o["iters"][:, 1:] >= 0).all() and not o["loss_all"][:, 0].any()
    # max_sweeps = 3 caps the one (agent, game) whose gamma is not 0: gamma = 0 settles in two sweeps
    gam = np.zeros((N, G))
    gam[0, 3] = 0.9
    cap = _run(c, epsilon=eps, gamma=gam, noise_prob=p, max_sweeps=3, pi=pi, policies=True)
    _same(cap, _mirror(c, eps, gam, p, max_sweeps=3, pi=pi), OUT + WEIGHTED + POL, "capped")
    assert cap["iters"][0, 3] == -1 and cap["sweeps"][0, 3] == 3 and np.isnan(cap["loss_all"][0, 3])
    assert np.array_equal(cap["br_policy"][0, 3], np.minimum(np.concatenate([c["pol"][3, 0], c["npol"][3, 0]]), 1))
    ok = np.ones((N, G), bool)
    ok[0, 3] = False
    assert (cap["iters"][ok] >= 0).all() and not np.isnan(cap["loss_w"][ok]).any()


# ------------------------------------------------------------------------------------------------ against older code
def test_deterministic_rivals_give_greedy_equilibrium_noises_best_response_values():
    """An all-QTable batch at epsilon = 0 has deterministic rivals, so V* at the price-state row(t) is
    thrl_tuple_equilibrium_noise's V* at the tuple-state t and V* at node 1 + k its V* at cell k: a QTable agent's action
    is exact on a cell, and the atom's mass plays cell 0's actions in both models.  No new code in between.

    Tolerance: the bound of the noise-free cross-check
    (test_deterministic_rivals_give_greedy_equilibriums_best_response_values).  A Jacobi evaluation that stops at a change
    of at most eval_tol lies within gamma eval_tol / (1 - gamma) of its fixed point (the contraction carries the last
    change through the geometric series), which is the stopping bound; beside it a rounding allowance of four times the
    largest excess over that bound between the two CPU mirrors on the same strategies (tuple_equilibrium_noise_mirror
    against sampled_response_noise_mirror).  The device enters neither.  (With deterministic rivals the two solvers
    make the same operations in the same order -- a rival's probability is exactly 1.0 or 0.0 -- so the mirrors' excess,
    and the device's difference, are expected to be 0.)"""
    import tuple_equilibrium_noise_mirror as TENM
    from th_rl_amd import sampled_play as sp
    from th_rl_amd import tuple_play as tp
    from th_rl_amd import tuple_stationary as ts
    config = {"agents": [dict(AG, actions=5), dict(AG, actions=4, gamma=0.9)], "environment": dict(ENV)}
    G, res, tol = 4, 16, 1e-12
    mb = _mixed(config, G, seed=5)
    tabs, old_tabs = sp.noise_tables(config, res), ts.tables(config, res)
    T, D, Jn = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"])
    p = np.array([0.05, 0.2, 0.5, 1.0])
    tup, cell, npol = tp.extract(mb, tabs), ts.extract_cells(mb, old_tabs), ts.price_policy(mb, tabs["xn"])
    rep = np.asarray(tabs["grp_perm"])[np.asarray(tabs["grp_first"])[:-1]]
    h_tup, h_cell, h_npol = (x.cpu().numpy().view(np.uint16) for x in (tup, cell, npol))
    top = np.array([4, 3])[None, :, None]                # the entries as both calls clamp them
    assert np.array_equal(np.minimum(h_npol[:, :, 1:], top), np.minimum(h_cell, top))
    assert np.array_equal(h_npol[:, :, 0], h_npol[:, :, 1])
    ge = mb.greedy_equilibrium_noise(noise_prob=p, resolution=res, eval_tol=tol, policies=True, weights=None, tuple_policy=tup,
                                     cell_policy=cell, tabs=old_tabs)
    out = mb.sampled_response_noise(epsilon=0.0, noise_prob=p, ntabs=tabs, eval_tol=tol, pi=False, policies=True,
                                    dpolicy=_dev(mb, h_tup[:, :, rep]), npolicy=npol)
    assert (ge["iters"] >= 0).all() and (out["iters"] >= 0).all() and ge["n_cells"] == Jn - 1
    gam = np.array([0.95, 0.9])
    m_old = TENM.analyse(old_tabs, h_tup, h_cell, p, gamma=gam, eval_tol=tol)
    m_new = SRNM.analyse(tabs, {}, h_tup[:, :, rep], {}, h_npol, 0.0, gam, p, eval_tol=tol)
    row = np.asarray(tabs["row"])

    def diff(new, old, i):
        return max(np.abs(new["v_opt"][i][:, row] - old["v_opt"][i][:, :T]).max(),
                   np.abs(new["v_opt"][i][:, D + 1:] - old["v_opt"][i][:, T:]).max())
    for i in range(2):
        bound = gam[i] * tol / (1.0 - gam[i])
        excess = max(0.0, diff(m_new, m_old, i) - bound)
        err = diff(out, ge, i)
        e_0 = np.abs(out["v_opt"][i][:, D] - out["v_opt"][i][:, D + 1]).max()          # the atom plays cell 0's actions
        print("agent %d: device difference %.3g, atom against cell 0 %.3g, bound %.3g, CPU mirrors' excess %.3g"
              % (i, err, e_0, bound, excess))
        assert err <= bound + 4.0 * excess, (i, err, bound, excess)
        assert e_0 <= bound + 4.0 * excess


# ------------------------------------------------------------------------------------------------ the working set
def test_the_largest_accepted_working_set_and_the_first_refused_shape():
    """Of QTable A x Reinforce B for A in 20..39 and B in {21, 24, 28, 32} at the default resolution (Jn = 1,121) the
    heaviest shape the plan accepts is 33 x 28 (T = 924, D = 555: 161,216 of 163,840 bytes), solved here for one game at
    gamma 0 with max_sweeps = 4 (an evaluation at gamma 0 settles in two sweeps) and equal to the mirror; the lightest it
    refuses is 35 x 21 (T = D = 735: 165,632 bytes), THRL_ERR_UNSUPPORTED without a launch."""
    from th_rl_amd import _lib
    from th_rl_amd import sampled_play as sp
    from th_rl_amd import sampled_response as sr
    from th_rl_amd._lib import ThrlError

    def cfg(A, B):
        return {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}
    ws, over = sr.working_set_noise(cfg(33, 28)), sr.working_set_noise(cfg(35, 21))
    assert ws == dict(bytes=161216, T=924, D=555, Jn=1121, fits=True) and ws["bytes"] <= sr.MAX_LDS
    assert over == dict(bytes=165632, T=735, D=735, Jn=1121, fits=False)
    c = _inputs(cfg(33, 28), 1024, 1, 41)
    out = _run(c, epsilon=c["eps"], gamma=0.0, noise_prob=c["p"], max_sweeps=4, pi=c["pi"], policies=True)
    assert out["lds_bytes"] == ws["bytes"] and out["n_nodes"] == 1121 and (out["iters"] >= 0).all()
    _same(out, _mirror(c, c["eps"], 0.0, c["p"], max_sweeps=4, pi=c["pi"]), OUT + WEIGHTED + POL, "largest")
    # the next shape: refused by the library from the shape alone (no tensor is valid, none is touched)
    mb2 = _mixed(cfg(35, 21), 1)
    with pytest.raises(ThrlError) as e:
        mb2.sampled_response_noise(noise_prob=0.05, pi=False)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a = _lib.SampledResponseNoiseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.n_nodes, a.band_w, a.agents, a.max_sweeps, a.noise_prob = 1, 735, 735, 1121, 310, 3, 8, 0.05
    a.kind[1] = 1
    assert mb2.L.thrl_sampled_response_noise(mb2.cfg, a, None) == _lib.ERR_UNSUPPORTED
    assert b"165632 bytes of LDS per game" in mb2.L.thrl_last_error()


# ------------------------------------------------------------------------------------------------ the trainer
def test_train_one_writes_the_response_under_noise_beside_sampled_play(tmp_path):
    from th_rl_amd import utils
    from th_rl_amd.trainer import train_one
    base = {"agents": [dict(AG, actions=3, states=10), dict(RF, actions=3, gamma=0.95)],
            "environment": dict(ENV, max_steps=10, noise_prob=0.1)}
    runs = {}
    for key, extra in (("plain", {}), ("resp", {"response": {"noise": True, "policies": True, "eval_tol": 1e-10}})):
        cfg = dict(base, training={"epochs": 4, "print_freq": 500, "seed": 3, "n_games": 6,
                                   "sampled_play": dict({"pi": True, "noise": {"resolution": 16}}, **extra)})
        (tmp_path / (key + ".json")).write_text(json.dumps(cfg))
        train_one(str(tmp_path / key), str(tmp_path / (key + ".json")))
        runs[key] = str(tmp_path / key)
    files = sorted(os.listdir(runs["resp"]))
    for f in ("sampled_response_noise.json", "srespn_counts.npy", "srespn_loss.npy", "srespn_weighted.npy", "srespn_gamma.npy",
              "srespn_epsilon.npy", "srespn_noise_prob.npy", "srespn_br_policy.npy", "srespn_v_opt.npy", "srespn_v_pi.npy"):
        assert f in files, (f, files)
    # the noise-free analysis' files are what they are without it: absent
    assert not any(f.startswith("sresp_") or f == "sampled_response.json" for f in files)
    assert not any(f.startswith("sresp") or f.startswith("sampled_response") for f in os.listdir(runs["plain"]))
    for f in sorted(os.listdir(runs["plain"])):
        if f.startswith("splay_"):
            assert open(os.path.join(runs["plain"], f), "rb").read() == open(os.path.join(runs["resp"], f), "rb").read(), f
    desc = json.load(open(os.path.join(runs["resp"], "sampled_response_noise.json")))
    assert desc["options"]["noise"] is True and desc["options"]["policies"] is True and desc["agents"] == [0, 1]
    assert desc["resolution"] == 16 and desc["n_nodes"] == np.load(os.path.join(runs["resp"], "srespn_v_opt.npy")).shape[2] - desc["n_prices"]
    assert "response" not in json.load(open(os.path.join(runs["resp"], "sampled_play.json")))["options"]
    assert np.load(os.path.join(runs["resp"], "srespn_counts.npy")).shape == (4, 2, 6)
    assert np.array_equal(np.load(os.path.join(runs["resp"], "srespn_noise_prob.npy")), np.full(6, 0.1))
    summary = utils.sampled_response_noise_summary(runs["resp"])
    games = utils.sampled_response_noise_games(runs["resp"])
    assert len(games) == 6 and (games["iters_0"] >= 0).all() and (games["iters_1"] >= 0).all()
    assert set(summary["agent"].dropna().astype(int)) == {0, 1}
    for col in ("nashconv_mean", "exploit_mean", "diff_nodes_mean", "max_jump_max"):
        assert col in summary.columns, col
    assert np.isfinite(games["exploit_0"]).all() and (games["nashconv"] > -1e-9).all()
