"""Sampled play under demand noise on the device (thrl_sampled_noise_chain, MixedGameBatch.sampled_play(noise_prob=...),
training.sampled_play with noise_prob): the chain bit-equal to the numpy mirror (tests/sampled_noise_mirror.py) in every
output for every shape, start, noise and epsilon mode, for one game, in halves, with the node count on the tile's edges and
at the edge of the working-set plan; with p = 0 bit-equal to thrl_sampled_chain; an all-QTable batch at epsilon = 0 against
thrl_tuple_stationary, the same chain in another summation order; max_jump; the trainer's artefacts."""
import json

import numpy as np
import pytest

import sampled_mirror as SPM
import sampled_noise_mirror as SNM
from sampled_noise_mirror import ATOM, NO_ATOM, RESET, three_agents, two_agents
from th_rl_amd import _lib

pytestmark = pytest.mark.gpu

OUT = ("iters", "change", "mass", "samp_reward", "samp_action", "samp_price", "agree", "pi", "max_jump")
TILE = _lib.SPN_TILE
G = 203
# name -> (config, resolution, max_iters)
SHAPES = {
    "S1": (two_agents("QTable", 2, "QTable", 2), 0, 64),
    "S1n": (two_agents("QTable", 2, "QTable", 2, NO_ATOM), 0, 64),
    "S2": (two_agents("QTable", 2, "Reinforce", 3), 8, 64),
    "S2n": (two_agents("QTable", 2, "Reinforce", 3, NO_ATOM), 8, 64),
    "S3": (three_agents(), 8, 32),
    "S3n": (three_agents([0.0, 0.2]), 8, 32),
    "S4": (two_agents("QTable", 21, "Reinforce", 21), 64, 3),
    "S5a": (two_agents("Reinforce", 5, "Reinforce", 5), TILE - 1, 12),
    "S5b": (two_agents("Reinforce", 5, "Reinforce", 5, NO_ATOM), TILE, 12),
    "S5c": (two_agents("Reinforce", 5, "Reinforce", 5), 2 * TILE - 2, 12),
    "S5d": (two_agents("Reinforce", 5, "Reinforce", 5), 2 * TILE, 12),
}
S5_NODES = {"S5a": TILE, "S5b": TILE + 1, "S5c": 2 * TILE - 1, "S5d": 2 * TILE + 1}
BAD_P = {3: np.nan, 7: -0.1, 11: 0.0, 13: 1.0, 17: 1.5}


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


def _case(name, n_games=G):
    """dict(mb, tabs, probs / nprobs on the device and as numpy, dpolicy, npolicy, eps [N, G] and noise_prob [G] with bad
    entries, start with -1 and T): random networks evaluated by thrl_price_probs at the distinct prices and at the nodes."""
    def make():
        from th_rl_amd import sampled_play as sp
        config, resolution, _ = SHAPES[name]
        seed = 300 + sorted(SHAPES).index(name)
        tabs = sp.noise_tables(config, resolution)
        mb = _mixed(config, n_games)
        rs = np.random.RandomState(seed)
        for i, k in enumerate(tabs["kinds"]):
            if k != "QTable":
                mb.nn[i].set_params(SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, 0.0, float(tabs["price"].max())))
        probs, nprobs = sp.price_probs(mb, tabs["dprice"]), sp.price_probs(mb, tabs["xn"])
        host = {i: p.cpu().numpy() for i, p in probs.items()}
        nhost = {i: p.cpu().numpy() for i, p in nprobs.items()}
        pol = SPM.greedy_of(host, tabs, rs, n_games)
        npol = SPM.greedy_of(nhost, SNM.node_tabs(tabs), rs, n_games)
        N, T = len(tabs["kinds"]), int(tabs["n_tuples"])
        eps = rs.uniform(0.0, 0.2, (N, n_games))
        eps[:, ::4] = 0.0
        p = rs.uniform(0.0, 0.5, n_games)
        start = rs.randint(0, T, n_games).astype(np.int32)
        if n_games > 20:
            for g, v in BAD_P.items():
                p[g] = v
            start[2], start[5] = -1, T
            q = [i for i, k in enumerate(tabs["kinds"]) if k == "QTable"]
            if q:
                eps[q[0], 8], eps[q[0], 12] = np.nan, 1.5
        return dict(mb=mb, tabs=tabs, probs=probs, nprobs=nprobs, host=host, nhost=nhost, pol=pol, npol=npol, eps=eps, p=p,
                    start=start)
    return SPM.cached(("noise case", name, n_games), make)


def _run(c, eps, p, start, max_iters, sl=slice(None), tol=1e-12):
    mb = c["mb"]
    n = len(range(*sl.indices(c["pol"].shape[0])))
    cut = lambda d: {i: x[sl].contiguous() for i, x in d.items()}
    return mb.sampled_play(epsilon=eps, start="uniform" if start is None else start, tol=tol, max_iters=max_iters, pi=True,
                           n_games=n, probs=cut(c["probs"]), dpolicy=_dev(mb, c["pol"][sl]), tabs=c["tabs"], noise_prob=p,
                           nprobs=cut(c["nprobs"]), npolicy=_dev(mb, c["npol"][sl]))


def _mirror(c, eps, p, start, max_iters, sl=slice(None), tol=1e-12):
    cut = lambda d: {i: x[sl] for i, x in d.items()}
    return SNM.analyse(c["tabs"], cut(c["host"]), c["pol"][sl], cut(c["nhost"]), c["npol"][sl], eps, p, start=start, tol=tol,
                       max_iters=max_iters)


# ------------------------------------------------------------------------------------------------ mirror, bit for bit
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_chain_equals_the_mirror(name):
    c = _case(name)
    tabs, eps, p, start = c["tabs"], c["eps"], c["p"], c["start"]
    max_iters = SHAPES[name][2]
    if name in S5_NODES:
        assert tabs["n_nodes"] == S5_NODES[name]                         # the node count sits on the tile's edge
    assert (tabs["nn"][:, 0] > 0).any() == (not name.endswith("n") and name != "S5b")     # the atom is hit / never hit
    bad = ~((p >= 0.0) & (p <= 1.0))
    for i, k in enumerate(tabs["kinds"]):
        if k == "QTable":
            bad |= ~((eps[i] >= 0.0) & (eps[i] <= 1.0))
    assert bad.sum() >= 3 and not bad[11] and not bad[13]
    bad_start = np.zeros(G, bool)
    bad_start[[2, 5]] = True
    # per-game noise and epsilon from the three starts, -1 and T mixed into the start tuples
    for what, st in (("uniform", None), ("reset", RESET), ("tuple", start)):
        out = _run(c, eps, p, st, max_iters)
        ref = _mirror(c, eps, p, st, max_iters)
        for f in OUT:
            _bits_equal(out[f], ref[f], "%s %s %s" % (name, what, f))
        b = bad | bad_start if what == "tuple" else bad
        assert (out["iters"][b] == -1).all() and not out["pi"][b].any() and not out["agree"][b].any()
        assert (out["iters"][~b] >= 1).all() and (np.abs(out["mass"][~b] - 1.0) < 1e-12).all()
        _bits_equal(out["noise_prob"], p, "noise_prob")
        _bits_equal(out["epsilon"], eps, "epsilon")
        assert out["n_nodes"] == tabs["n_nodes"]
    print("%s: T = %d, D = %d, Jn = %d, W = %d, iters %d..%d, max_jump up to %.3g, LDS %d bytes"
          % (name, tabs["n_tuples"], tabs["n_prices"], tabs["n_nodes"], tabs["band_w"], out["iters"][~b].min(), out["iters"].max(),
             out["max_jump"].max(), out["lds_bytes"]))
    # scalar noise, scalar and per-agent epsilon
    if name != "S4":
        N = c["mb"].N
        for pp, e in ((0.05, 0.0), (1.0, [0.25] + [0.5] * (N - 1)), (0.5, 0.1)):
            out = _run(c, e, pp, RESET, 16)
            ref = _mirror(c, [e] * N if np.ndim(e) == 0 else e, pp, RESET, 16)
            for f in OUT:
                _bits_equal(out[f], ref[f], "%s p=%s eps=%s %s" % (name, pp, e, f))


@pytest.mark.parametrize("name", ["S3", "S1"])
def test_one_game_and_the_batch_in_halves(name):
    from th_rl_amd import sampled_play as sp
    c = _case(name)
    eps, p, start = c["eps"], c["p"], c["start"]
    max_iters = SHAPES[name][2]
    whole = _run(c, eps, p, start, max_iters)
    h = G // 2
    parts = [_run(c, eps[:, :h], p[:h], start[:h], max_iters, slice(0, h)), _run(c, eps[:, h:], p[h:], start[h:], max_iters, slice(h, G))]
    both = sp.combine(parts)
    for f in OUT + ("start", "epsilon", "noise_prob"):
        _bits_equal(both[f], whole[f], "halves %s" % f)
    one = _run(c, eps[:, 9:10], p[9:10], start[9:10], max_iters, slice(9, 10))
    ref = _mirror(c, eps[:, 9:10], p[9:10], start[9:10], max_iters, slice(9, 10))
    for f in OUT:
        _bits_equal(one[f], whole[f][9:10] if f == "pi" else whole[f][..., 9:10], "one game %s" % f)
        _bits_equal(one[f], ref[f], "one game, mirror %s" % f)
    assert one["iters"][0] >= 1


# ------------------------------------------------------------------------------------------------ p = 0
@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S5b", "S4"])
def test_without_noise_it_is_the_noise_free_chain_bit_for_bit(name):
    """p = 0 for every game (as an array, which takes the noisy entry point): s = 1.0 * Sd + 0.0 * Sn = Sd."""
    c = _case(name)
    mb, eps, start = c["mb"], c["eps"], c["start"]
    max_iters = SHAPES[name][2]
    for st in (None, start):
        noisy = _run(c, eps, np.zeros(G), st, max_iters)
        plain = mb.sampled_play(epsilon=eps, start="uniform" if st is None else st, max_iters=max_iters, pi=True,
                                probs=c["probs"], dpolicy=_dev(mb, c["pol"]), tabs=c["tabs"])
        assert "max_jump" in noisy and "max_jump" not in plain
        for f in ("iters", "change", "mass", "pi", "samp_reward", "samp_action", "samp_price", "agree"):
            _bits_equal(noisy[f], plain[f], "%s %s" % (name, f))
        assert (plain["iters"] >= 1).sum() >= G - 6


# ------------------------------------------------------------------------------------------------ against thrl_tuple_stationary
@pytest.mark.parametrize("name", ["S1", "Q5"])
def test_all_qtable_greedy_play_against_tuple_stationary(name):
    """With epsilon = 0 an all-QTable game's rows are 0 / 1 and this chain is thrl_tuple_stationary's (the atom plays the
    row of cell 0, as the clipped mass lumped into cell 0 does there), summed in another order.  Both run up to K steps (tol = 0: a chain stops early only at an exact fixed point).
    One step is a column-stochastic map, so it does not expand an earlier difference in the 1-norm, and it adds per entry
    at most R roundings of non-negative terms: here M (T), W (1), the products (2 N), Sd (D), nu (2 T), V (1), Sn (Jn) and
    q Sd + p Sn, m / 2 + s / 2 (6): R_a = 3 T + D + Jn + 2 N + 8; there the two gathers (T and 2 T), the sum over the
    cells (Jn) and the same 6: R_b = 3 T + Jn + 6.  The reset start adds Jn + N + 2 on each side.  So sum_t |pi_a - pi_b|
    <= B = 2 (K (R_a + R_b) + 2 (Jn + N + 2)) 2^-53 (the 2 covers second order terms), and an output, a sum of T products
    with a value of size <= top (2 T + 4 roundings on each side), differs by at most (B + 2 (2 T + 4) 2^-53) top."""
    from th_rl_amd import sampled_play as sp, tuple_stationary as ts
    config = SHAPES["S1"][0] if name == "S1" else two_agents("QTable", 5, "QTable", 5)
    n, K, p = 64, 64, 0.05
    mb = _mixed(config, n, seed=17)
    mb.run(30, per_game_logs=False)
    a = mb.sampled_play(epsilon=0.0, start="reset", tol=0.0, max_iters=K, pi=True, noise_prob=p, resolution=0)
    b = mb.greedy_stationary(noise_prob=p, start="reset", resolution=0, tol=0.0, max_iters=K, pi=True)
    tabs = sp.noise_tables(config, 0)
    T, D, Jn, N = tabs["n_tuples"], tabs["n_prices"], tabs["n_nodes"], 2
    # a chain that stops before K has reached chg == 0.0: its iterate is a fixed point in its own arithmetic, so it is
    # also what K steps give
    assert (a["iters"] >= 1).all() and (a["iters"] <= K).all() and (b["iters"] >= 1).all() and (b["iters"] <= K).all()
    assert b["n_cells"] == Jn - 1 and not a["max_jump"].any()
    B = 2 * (K * ((3 * T + D + Jn + 2 * N + 8) + (3 * T + Jn + 6)) + 2 * (Jn + N + 2)) * 2.0 ** -53
    l1 = np.abs(a["pi"] - b["pi"]).sum(axis=1).max()
    print("%s: sum_t |pi - pi'| up to %.3g, bound %.3g" % (name, l1, B))
    assert l1 <= B
    out_u = 2 * (2 * T + 4) * 2.0 ** -53
    for fa, fb, top in (("samp_reward", "stat_reward", max(np.abs(tabs["reward"]).max(), np.abs(tabs["noise_reward"]).max())),
                        ("samp_action", "stat_action", np.abs(tabs["scaled"]).max()),
                        ("samp_price", "stat_price", max(np.abs(tabs["price"]).max(), np.abs(tabs["noise_price"]).max()))):
        worst = np.abs(a[fa] - b[fb]).max()
        print("%s %s: largest difference %.3g, bound %.3g" % (name, fa, worst, (B + out_u) * top))
        assert worst <= (B + out_u) * top, fa
    assert (np.abs(a["agree"] - 1.0) < 1e-12).all() and len(set(a["samp_price"].tolist())) > 1


# ------------------------------------------------------------------------------------------------ max_jump
def test_max_jump_is_the_largest_change_between_adjacent_nodes():
    for name in ("S1", "S3", "S5c"):
        c = _case(name)
        out = _run(c, c["eps"], c["p"], None, 2)
        want = np.zeros(G)
        for x in c["nhost"].values():
            x64 = x.astype(np.float64)
            for j in range(1, x.shape[1] - 1):
                want = np.fmax(want, np.abs(x64[:, j + 1] - x64[:, j]).max(axis=1))
        _bits_equal(out["max_jump"], want, name)
        assert (out["iters"] == -1).any() and (want > 0).all() == (name != "S1")     # written for refused games too


# ------------------------------------------------------------------------------------------------ the edge of the plan
def test_the_largest_accepted_shape_and_the_first_refused():
    from test_sampled_noise_host import plan_edge
    from th_rl_amd import sampled_play as sp
    from th_rl_amd._lib import ThrlError
    fits, refused = plan_edge()
    rs = np.random.RandomState(91)
    tabs = sp.noise_tables(fits, 1024)
    mb = _mixed(fits, 2)
    mb.nn[1].set_params(SPM.random_weights(rs, 2, 32, "Reinforce", 0.0, float(tabs["price"].max())))
    probs, nprobs = sp.price_probs(mb, tabs["dprice"]), sp.price_probs(mb, tabs["xn"])
    host, nhost = {1: probs[1].cpu().numpy()}, {1: nprobs[1].cpu().numpy()}
    pol, npol = SPM.greedy_of(host, tabs, rs, 2), SPM.greedy_of(nhost, SNM.node_tabs(tabs), rs, 2)
    out = mb.sampled_play(epsilon=[0.1, 0.0], start="reset", max_iters=4, pi=True, probs=probs, dpolicy=_dev(mb, pol), tabs=tabs,
                          noise_prob=0.05, nprobs=nprobs, npolicy=_dev(mb, npol))
    ref = SNM.analyse(tabs, host, pol, nhost, npol, [0.1, 0.0], 0.05, start=RESET, max_iters=4)
    for f in OUT:
        _bits_equal(out[f], ref[f], f)
    assert out["iters"].tolist() == [4, 4] and sp.MAX_LDS - 16384 < out["lds_bytes"] <= sp.MAX_LDS
    with pytest.raises(ThrlError, match="bytes of LDS") as e:
        _mixed(refused, 2).sampled_play(max_iters=4, noise_prob=0.05)
    assert e.value.code == -3


# ------------------------------------------------------------------------------------------------ the trainer
def test_train_one_artefacts(tmp_path):
    from th_rl_amd import sampled_play as sp, trainer, utils
    n = 16
    base = dict(SPM.SHIP, environment=dict(SPM.ENV, max_steps=20))
    train = {"epochs": 20, "print_freq": 500, "seed": 23, "n_games": n}
    cfg = dict(base, training=dict(train, sampled_play={"noise": {"noise_prob": 0.05, "resolution": 64}},
                                   greedy_stationary={"resolution": 64, "noise_prob": 0.05}))
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    exp = tmp_path / "run"
    trainer.train_one(str(exp), str(tmp_path / "c.json"))
    desc = json.load(open(exp / "sampled_play.json"))
    assert desc["options"] == dict(sp.DEFAULTS, noise={"noise_prob": 0.05, "resolution": 64}) and desc["n_nodes"] == sp.n_nodes_of(base, 64)
    games = utils.sampled_play_games(str(exp))
    assert games.index.tolist() == list(range(n)) and (games["noise_prob"] == 0.05).all() and (games["iters"] >= 1).all()
    assert (games["max_jump"] >= 0.0).all() and (np.abs(games["mass"].to_numpy() - 1.0) <= 1e-9).all()
    _bits_equal(np.load(exp / "splay_max_jump.npy"), games["max_jump"].to_numpy(), "max_jump")
    summ = utils.sampled_play_summary(str(exp))
    assert {"max_jump_max", "delta_greedy_noise_mean", "randomness_cost_noise_mean", "n_nodes"} <= set(summ.columns)
    assert np.isfinite(summ["randomness_cost_noise_mean"][0]) and summ["max_jump_max"][0] == games["max_jump"].max()
    print("sampled play under noise after 20 episodes: delta_sampled %.4f, delta_greedy_noise %.4f, max_jump %.3g, iters up to %d"
          % (summ["delta_sampled_mean"][0], summ["delta_greedy_noise_mean"][0], summ["max_jump_max"][0], games["iters"].max()))
    # sampled_play: true leaves the noise-free mode's files and nothing else
    (tmp_path / "d.json").write_text(json.dumps(dict(base, training=dict(train, sampled_play=True))))
    plain = tmp_path / "plain"
    trainer.train_one(str(plain), str(tmp_path / "d.json"))
    files = sorted(f.name for f in plain.iterdir() if f.name.startswith("splay_"))
    assert files == ["splay_action.npy", "splay_epsilon.npy", "splay_games.npy", "splay_iters.npy", "splay_reward.npy"]
    desc = json.load(open(plain / "sampled_play.json"))
    assert "n_nodes" not in desc and desc["options"] == sp.DEFAULTS
    assert "max_jump" not in utils.sampled_play_games(str(plain)).columns
