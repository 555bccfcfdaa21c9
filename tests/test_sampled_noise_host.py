"""Host side of sampled play under demand noise (th_rl_amd.sampled_play.noise_tables, thrl_sampled_noise_chain): the node
tables, the numpy mirror's hand answers, the model against a simulation of the environment that shares no code with the
chain, option parsing and refusals, the summary rows and readers, the ctypes mirror of the args struct against the header
and the entry point's validation through the library loaded without a GPU.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

import policy_reference as PR
import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import tuple_stationary_mirror as TSM
from sampled_mirror import AG, CAC, ENV, RF, SHIP
from sampled_noise_mirror import NO_ATOM, RESET, three_agents, two_agents
from test_tuple_stationary_host import _offsets
from th_rl_amd import sampled_play as sp
from th_rl_amd import tuple_stationary as ts

FAKE = 4096                           # never dereferenced: validation fails before any launch
U = 2.0 ** -52


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def plan_edge():
    """(fits, refused): a QTable against a 32-action network at the default resolution, one QTable action apart: the
    heaviest count up to 30 that working_set() accepts and whose successor it refuses."""
    cfg = lambda aq: two_agents("QTable", aq, "Reinforce", 32)
    ws = {aq: sp.working_set(cfg(aq), resolution=1024) for aq in range(2, 32)}
    aq = max((a for a in range(2, 31) if ws[a]["fits"] and not ws[a + 1]["fits"]), key=lambda a: ws[a]["bytes"])
    return cfg(aq), cfg(aq + 1)


# ------------------------------------------------------------------------------------------------ the node tables
@pytest.mark.parametrize("config,resolution", [(SHIP, 1024), (two_agents("QTable", 2, "QTable", 2), 0), (three_agents(), 8),
                                               (two_agents("QTable", 2, "Reinforce", 3, NO_ATOM), 8),
                                               (two_agents("Reinforce", 5, "Reinforce", 5), 64)])
def test_noise_tables(config, resolution):
    t = sp.noise_tables(config, resolution)
    base = ts.tables(config, resolution)
    Jn, T = t["n_nodes"], t["n_tuples"]
    assert Jn == base["n_cells"] + 1 and t["xn"][0] == 0.0 and np.array_equal(t["xn"][1:], base["cell_x"])
    assert t["node_w"][0] == 0.0 and np.array_equal(t["node_w"][1:], base["cell_w"]) and t["nn"].shape == (T, Jn)
    assert (np.abs(t["nn"].sum(axis=1) - 1.0) <= Jn * U).all()
    # the atom carries mass exactly for the tuples whose band reaches below price 0: u(t) > 0.7 a
    a, b = float(config["environment"]["a"]), float(config["environment"]["b"])
    u = b * (a / b * t["scaled"]).sum(axis=0)
    assert np.array_equal(t["nn"][:, 0] > 0, u > 0.7 * a)
    # the band is nn, contiguous from its first to its last non-zero entry
    W = t["band_w"]
    full = np.zeros((T, Jn + W))
    for k in range(T):
        full[k, t["band_lo"][k]:t["band_lo"][k] + W] = t["band"][k]
    assert t["band"].shape == (T, W) and np.array_equal(full[:, :Jn], t["nn"]) and not full[:, Jn:].any()
    # folding the atom into cell 0 gives tuple_stationary's weights: bit for bit without clipped mass, else one rounding
    fold = t["nn"][:, 1:].copy()
    fold[:, 0] = fold[:, 0] + t["nn"][:, 0]
    fullb = np.zeros((T, Jn - 1 + base["band_w"]))
    for k in range(T):
        fullb[k, base["band_lo"][k]:base["band_lo"][k] + base["band_w"]] = base["band"][k]
    z0 = t["nn"][:, 0] == 0
    assert np.array_equal(fold[z0], fullb[z0, :Jn - 1])
    assert (np.abs(fold - fullb[:, :Jn - 1]) <= U * fullb[:, :Jn - 1]).all()
    assert np.array_equal(t["noise_price"], base["noise_price"]) and np.array_equal(t["noise_reward"], base["noise_reward"])
    if all(k != "QTable" for k in t["kinds"]):
        assert Jn == resolution + 1
    for f in ("dprice", "grp_first", "grp_perm", "price", "reward", "scaled"):
        assert np.array_equal(t[f], sp.tables(config)[f])


def test_working_set_follows_the_layout():
    r16 = lambda x: (x + 15) & ~15
    ws = sp.working_set(SHIP, resolution=1024)
    assert ws["Jn"] == 1121 and ws["bytes"] == sp.working_set(SHIP)["bytes"] + r16(8 * 1121) + r16(2 * 1121) \
        + 2 * r16(4 * (sp.TILE * 21 + 3)) == 79232 and 2 * ws["bytes"] <= sp.MAX_LDS
    assert sp.working_set(SHIP, n_nodes=1121) == ws and "Jn" not in sp.working_set(SHIP)
    fits, refused = plan_edge()
    a, b = sp.working_set(fits, resolution=1024), sp.working_set(refused, resolution=1024)
    assert a["fits"] and not b["fits"] and (a["bytes"], b["bytes"]) == (153696, 179728)
    assert [x["actions"] for x in fits["agents"]] == [27, 32] and [x["actions"] for x in refused["agents"]] == [28, 32]
    with pytest.raises(ValueError, match="4095"):
        sp.working_set(two_agents("Reinforce", 5, "Reinforce", 5), resolution=4096)
    assert sp.n_nodes_of(two_agents("Reinforce", 5, "Reinforce", 5), 4095) == 4096


# ------------------------------------------------------------------------------------------------ mirror, hand answers
def _constant_rows(t, n_games, p1, p2):
    D, Jn = t["n_prices"], t["n_nodes"]
    probs = {0: np.tile(p1, (n_games, D, 1)), 2: np.tile(p2, (n_games, D, 1))}
    nprobs = {0: np.tile(p1, (n_games, Jn, 1)), 2: np.tile(p2, (n_games, Jn, 1))}
    pol, npol = np.zeros((n_games, 3, D), np.uint16), np.zeros((n_games, 3, Jn), np.uint16)
    pol[:, 1], npol[:, 1] = 2, 2                                          # the QTable agent's greedy action everywhere
    return probs, nprobs, pol, npol


def test_rows_that_ignore_the_price_give_the_product_after_one_step():
    t = sp.noise_tables(three_agents(), 8)
    p1, p2 = np.array([0.25, 0.75], np.float32), np.array([0.5, 0.5], np.float32)
    probs, nprobs, pol, npol = _constant_rows(t, 3, p1, p2)
    eps = 0.3
    q1 = np.array([eps / 3, eps / 3, (1 - eps) + eps / 3])
    want = (p1.astype(np.float64)[:, None, None] * q1[None, :, None] * p2.astype(np.float64)[None, None, :]).reshape(-1)
    for p in (0.0, 0.05, 0.5, 1.0):
        for start in (None, [0, 5, 11]):
            r = SNM.analyse(t, probs, pol, nprobs, npol, [0, eps, 0], p, start=start, max_iters=1)
            m0 = np.full((3, 12), 1 / 12.0) if start is None else np.eye(12)[start]
            assert np.abs(2 * r["pi"] - m0 - want[None, :]).max() < 1e-15, (p, start)
        r = SNM.analyse(t, probs, pol, nprobs, npol, [0, eps, 0], p, start=RESET, max_iters=1)
        assert np.abs(r["pi"] - want[None, :]).max() < 1e-15               # the reset start is the product already
        assert not r["max_jump"].any() and np.abs(r["agree"] - 0.25 * q1[2] * 0.5).max() < 1e-15
    r = SNM.analyse(t, probs, pol, nprobs, npol, [0, eps, 0], 1.0, start=[0, 5, 11], tol=1e-13)
    m = r["pi"]
    assert np.abs(r["samp_price"] - (m * t["noise_price"][None, :]).sum(axis=1)).max() < 1e-13
    assert np.abs(r["samp_price"] - want @ t["noise_price"]).max() < 1e-11
    assert np.abs(r["samp_reward"][:, 0] - t["noise_reward"] @ want).max() < 1e-11


@pytest.mark.parametrize("name", ["QR", "QRA", "QQ"])
def test_without_noise_the_mirror_is_the_noise_free_mirror(name):
    config, T, n_games, max_iters, seed = SPM.CASES[name]
    n_games = 24
    x = SNM.make_inputs(config, 8, n_games, seed)
    x["eps"][0, 1], x["start"][2] = np.nan, T
    for start in (None, x["start"]):
        for p in (0.0, np.zeros(n_games)):
            r = SNM.analyse(x["tabs"], x["probs"], x["dpolicy"], x["nprobs"], x["npolicy"], x["eps"], p, start=start,
                            max_iters=max_iters)
            ref = SPM.analyse(x["tabs"], x["probs"], x["dpolicy"], x["eps"], start=start, max_iters=max_iters)
            for f in ref:
                assert np.array_equal(np.asarray(r[f]).view(np.uint8), np.asarray(ref[f]).view(np.uint8)), (name, f)
            assert (r["iters"] == -1).sum() == (1 if start is None else 2)


@pytest.mark.parametrize("config", [two_agents("QTable", 2, "QTable", 2), two_agents("QTable", 5, "QTable", 5, NO_ATOM)])
def test_the_reset_start_of_greedy_qtables_is_tuple_stationarys(config):
    """epsilon = 0, all QTable: m_0 is the weight of the cells in which a tuple is played, tuple_stationary_mirror's start
    (its grouped sum of cell_w), up to the order of the sum and the division by Zn = 1."""
    n = 12
    x = SNM.make_inputs(config, 0, n, 5)
    tabs, base = x["tabs"], ts.tables(config, 0)
    Jn, T = tabs["n_nodes"], tabs["n_tuples"]
    x["npolicy"][:, :, 0] = x["npolicy"][:, :, 1]                         # a QTable's atom sits in the row of cell 0
    cells = x["npolicy"][:, :, 1:]
    want = TSM.grouped(TSM.tuple_of(base, cells), np.broadcast_to(base["cell_w"], (n, Jn - 1)), T)
    Pn, Zn, _ = SPM.rows_of(SNM.node_tabs(tabs), {}, x["npolicy"], np.zeros((2, n)))
    got = SNM.reset_start(tabs, Pn, Zn, SPM.actions_of(tabs))
    assert (Zn == 1.0).all() and (np.abs(got - want) <= Jn * U).all() and (want > 0).sum() > n
    r = SNM.analyse(tabs, {}, x["dpolicy"], {}, x["npolicy"], [0.0, 0.0], 1.0, start=RESET, max_iters=1)
    ref = TSM.analyse(base, np.zeros((n, 2, T), np.uint16), cells, 1.0, max_iters=1, kinds=["QTable", "QTable"])
    assert (np.abs(r["pi"] - ref["pi"]) <= 4 * Jn * U).all()             # one step under p = 1 reads no tuple strategy


def test_the_model_against_a_simulation_of_the_environment():
    """QTable 3 x Reinforce 3 under noise_prob = 0.3 with epsilon = 0.1, action range [0.2, 0.4] (redrawn prices clip to
    0): NoisyPriceState.step's arithmetic simulated with the policies evaluated at the exact continuous price (the
    network by policy_reference.probs64) for 1e5 steps after 1e3; each agent's mean reward with the standard error of 100
    batch means.  The mirror at resolution 1024 must lie within 5 standard errors: the error of the midpoint rule is far
    below that."""
    config = two_agents("QTable", 3, "Reinforce", 3)
    noise_prob, eps, a, b = 0.3, 0.1, 10.0, 1.0
    rs = np.random.RandomState(2024)
    w = SPM.random_weights(rs, 2, 3, "Reinforce", 0.0, 6.0)[1]            # game 1: fc_pi scaled by 8, peaked rows
    ga = rs.randint(0, 3, 101)                                            # the QTable's greedy action per state row
    row = lambda x: np.round(np.asarray(x) / 10.0 * 100).astype(np.int64)
    tabs = sp.noise_tables(config, 1024)
    probs = {1: PR.probs64(w, 3, tabs["dprice"])[0].astype(np.float32)[None]}
    nprobs = {1: PR.probs64(w, 3, tabs["xn"])[0].astype(np.float32)[None]}
    pol = np.stack([ga[row(tabs["dprice"])], probs[1][0].argmax(axis=1)])[None].astype(np.uint16)
    npol = np.stack([ga[row(tabs["xn"])], nprobs[1][0].argmax(axis=1)])[None].astype(np.uint16)
    r = SNM.analyse(tabs, probs, pol, nprobs, npol, [eps, 0.0], noise_prob, start=RESET, tol=1e-11)
    assert 1 <= r["iters"][0] < 8192 and (tabs["nn"][:, 0] > 0).any() and r["max_jump"][0] < 0.2
    # the simulation: environments.py:25-39, agents.py:80-89; nothing of the chain's code
    quant0 = a / b * (0.2 + np.arange(3) / 2.0 * 0.2)                     # QTable.scale, agents.py:51-57: k / (A - 1)
    quant1 = a / b * (0.2 + np.arange(3) / 3.0 * 0.2)                     # Reinforce.scale, agents.py:154-158: k / A
    burn, n_steps, n_batches = 1000, 100000, 100
    state = rs.uniform(0.0, a)
    rewards = np.zeros((n_steps, 2))
    u_all = rs.uniform(0.0, 1.0, (burn + n_steps, 4))
    new_a = rs.uniform(0.7 * a, a, burn + n_steps)
    explore = rs.randint(0, 3, burn + n_steps)
    for k in range(burn + n_steps):
        u = u_all[k]
        a0 = explore[k] if u[0] < eps else ga[int(np.round(state / 10.0 * 100))]
        c = np.cumsum(PR.probs64(w, 3, [state])[0][0])
        a1 = min(int(np.searchsorted(c, u[1] * c[-1], side="right")), 2)
        q0, q1 = quant0[a0], quant1[a1]
        price = max(0.0, (new_a[k] if u[2] < noise_prob else a) - b * (q0 + q1))
        if k >= burn:
            rewards[k - burn] = price * q0, price * q1
        state = price
    means = rewards.reshape(n_batches, -1, 2).mean(axis=1)
    est, se = means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(n_batches)
    print("simulated %s +- %s, model %s, iters %d, max_jump %.3g"
          % (est, se, r["samp_reward"][:, 0], r["iters"][0], r["max_jump"][0]))
    assert (np.abs(r["samp_reward"][:, 0] - est) <= 5.0 * se).all()


# ------------------------------------------------------------------------------------------------ options, refusals
def test_parse_options():
    """The noisy mode is the sub-dict "noise": without it every option dict parses to what it did before (five keys, "reset"
    no start, noise_prob no key: tests/test_sampled_host.py), with it the result carries it filled in."""
    old = dict(epsilon="current", start="uniform", tol=1e-12, max_iters=8192, pi=False)
    assert sp.parse_options(True, SHIP) == old == sp.DEFAULTS
    assert sp.parse_options({"noise": None}, SHIP) == old and sp.parse_options({"noise": False}, SHIP) == old
    noisy_env = dict(SHIP, environment=dict(ENV, noise_prob=0.05))
    assert sp.parse_options({"noise": True}, noisy_env) == dict(old, noise=dict(noise_prob=None, resolution=1024))
    got = sp.parse_options({"noise": {"noise_prob": 0.05, "resolution": 64}, "start": "reset", "pi": True}, SHIP)
    assert got == dict(old, start="reset", pi=True, noise=dict(noise_prob=0.05, resolution=64))
    for p in (0, 0.0, 1, 0.3):
        assert sp.parse_options({"noise": {"noise_prob": p, "resolution": 0}}, SHIP)["noise"] == dict(noise_prob=float(p), resolution=0)
    swept = dict(SHIP, training={"sweep": {"noise_prob": [0.01, 0.05]}})
    assert sp.parse_options({"noise": {"noise_prob": None}}, swept)["noise"]["noise_prob"] is None
    for own in (True, {}, {"noise_prob": None}):
        with pytest.raises(ValueError, match="noise_prob = 0"):
            sp.parse_options({"noise": own}, SHIP)
    for bad in ({"noise_prob": -0.1}, {"noise_prob": 1.5}, {"noise_prob": True}, {"noise_prob": "own"}, {"resolution": -1},
                {"resolution": 4097}, {"resolution": 2.0}, {"resolution": True}, {"start": "reset"}, 7, "yes"):
        with pytest.raises(ValueError, match="sampled_play.noise"):
            sp.parse_options({"noise": bad}, noisy_env)
    with pytest.raises(ValueError, match="start must be one of"):
        sp.parse_options({"noise": {"noise_prob": 0.05}, "start": "cycle"}, SHIP)
    with pytest.raises(ValueError, match="start must be one of"):
        sp.parse_options({"start": "reset"}, noisy_env)                   # the reset start belongs to the noisy mode
    rr = two_agents("Reinforce", 5, "Reinforce", 5)
    assert sp.parse_options({"noise": {"noise_prob": 0.05, "resolution": 4095}}, rr)["noise"]["resolution"] == 4095
    with pytest.raises(ValueError, match="sampled_play.*4095"):
        sp.parse_options({"noise": {"noise_prob": 0.05, "resolution": 4096}}, rr)
    fits, refused = plan_edge()
    assert sp.parse_options({"noise": {"noise_prob": 0.05}}, fits)["noise"]["noise_prob"] == 0.05 and sp.parse_options(True, refused)
    with pytest.raises(ValueError, match=r"179728 bytes \(T=896, D=896, Jn=1121\)"):
        sp.parse_options({"noise": {"noise_prob": 0.05}}, refused)
    with pytest.raises(ValueError, match="continuous"):
        sp.parse_options({"noise": {"noise_prob": 0.05}}, CAC)
    assert sp.noisy(0.05) and sp.noisy(None) and sp.noisy(np.zeros(3)) and sp.noisy(1)
    assert not sp.noisy(0.0) and not sp.noisy(0)


def test_refused_under_launch():
    from th_rl_amd import launch
    with pytest.raises(ValueError, match="sampled_play is not available under th_rl_amd.launch"):
        launch.check_launch_config(dict(SHIP, training={"n_games": 8, "sampled_play": {"noise": {"noise_prob": 0.05}}}))


def test_summary_rows_and_readers(tmp_path):
    from th_rl_amd import utils
    rs = np.random.RandomState(6)
    n = 6
    g = {"iters": np.array([3, 9, -1, 10, 10, 4], np.int32), "change": rs.rand(n), "mass": np.ones(n), "samp_price": rs.rand(n),
         "agree": rs.rand(n), "samp_reward": rs.rand(2, n) + 2.0, "samp_action": rs.rand(2, n), "epsilon": np.full((2, n), 0.01),
         "noise_prob": np.full(n, 0.05), "max_jump": np.array([.1, .2, .9, .3, .05, .01])}
    ids = [0, 0, 0, 1, 1, 1]
    rows = sp.summarize(g, ids, 2, 2.0, 4.0, 10)
    assert [r["max_jump_max"] for r in rows] == [0.9, 0.3] and "delta_greedy_noise_mean" not in rows[0]
    plain = sp.summarize({f: v for f, v in g.items() if f != "max_jump"}, ids, 2, 2.0, 4.0, 10)
    assert "max_jump_max" not in plain[0] and all(plain[0][f] == rows[0][f] for f in plain[0])
    sr, git = rs.rand(2, n) + 2.5, np.array([5, -1, 5, 5, 5, 5])
    rows = sp.summarize(g, ids, 2, 2.0, 4.0, 10, greedy_noise=(sr, git))
    delta, dn = (g["samp_reward"].sum(axis=0) - 2.0) / 2.0, (sr.sum(axis=0) - 2.0) / 2.0
    assert abs(rows[0]["delta_greedy_noise_mean"] - dn[0]) < 1e-15        # game 1 is refused there, game 2 here
    assert abs(rows[1]["randomness_cost_noise_mean"] - (dn[3:] - delta[3:]).mean()) < 1e-15
    json.dumps(rows)
    d = str(tmp_path)
    sp.save_games(d, g)
    assert {"splay_noise_prob.npy", "splay_max_jump.npy"} <= set(os.listdir(d))
    back = sp.load_games(d)
    assert sorted(back) == sorted(g) and all(np.array_equal(back[f], g[f]) for f in g)
    both = sp.combine([{f: v[..., :2] for f, v in g.items()}, {f: v[..., 2:] for f, v in g.items()}])
    assert all(np.array_equal(both[f], g[f]) for f in g)
    # greedy play under the same noise in the same directory, and under another
    gs = {"iters": git.astype(np.int32), "n_switch": np.zeros(n, np.int32), "change": rs.rand(n), "mass": np.ones(n),
          "stat_price": rs.rand(n), "unresolved": np.zeros(n), "noise_prob": np.full(n, 0.05), "stat_reward": sr,
          "stat_action": rs.rand(2, n)}
    assert sp.greedy_noise_of(d, g["noise_prob"]) is None
    ts.save_games(d, gs)
    open(os.path.join(d, "greedy_stationary.json"), "w").write("{}")
    got = sp.greedy_noise_of(d, g["noise_prob"])
    assert np.array_equal(got[0], sr) and np.array_equal(got[1], git)
    assert sp.greedy_noise_of(d, np.full(n, 0.01)) is None and sp.greedy_noise_of(d, np.full(n + 1, 0.05)) is None
    desc = sp.describe(dict(sp.DEFAULTS, noise=dict(sp.NOISE_DEFAULTS, noise_prob=0.05)), 441, 441, 2.0, 4.0, rows, n_nodes=1121)
    assert "n_nodes" not in sp.describe(dict(sp.DEFAULTS), 441, 441, 2.0, 4.0, rows)
    json.dump(desc, open(os.path.join(d, "sampled_play.json"), "w"))
    games = utils.sampled_play_games(d)
    assert games["max_jump"].tolist() == g["max_jump"].tolist() and (games["noise_prob"] == 0.05).all()
    summ = utils.sampled_play_summary(d)
    assert summ["n_nodes"].tolist() == [1121, 1121] and summ["max_jump_max"].tolist() == [0.9, 0.3]
    assert {"delta_greedy_noise_mean", "randomness_cost_noise_mean"} <= set(summ.columns)
    sp.save_games(d, {f: v for f, v in g.items() if f not in ("max_jump", "noise_prob")})      # a noise-free run after it
    assert "max_jump" not in sp.load_games(d) and "max_jump" not in utils.sampled_play_games(d).columns


# ------------------------------------------------------------------------------------------------ the entry point
def test_args_struct_matches_the_header():
    from th_rl_amd import _lib
    got, mine = _offsets(_lib.SampledNoiseChainArgs, "thrl_sampled_noise_chain_args",
                         ["THRL_SPN_START_TUPLE", "THRL_SPN_START_RESET", "THRL_SPN_TILE", "THRL_SP_MAX_LDS", "THRL_STAT_MAX_CELLS",
                          "THRL_ABI_VERSION"])
    assert got == mine[:1] + [_lib.SPN_START_TUPLE, _lib.SPN_START_RESET, _lib.SPN_TILE, _lib.SP_MAX_LDS, sp.MAX_CELLS, 4] + mine[1:]
    assert "thrl_sampled_noise_chain" in _lib.SYMBOLS and _lib.ABI_VERSION == 4 and sp.TILE == 64


SN_REQUIRED = ("dpolicy", "npolicy", "grp_first", "grp_perm", "reward", "scaled", "price", "band_lo", "band", "noise_price",
               "noise_reward", "node_w", "iters", "change", "mass", "samp_reward", "samp_action", "samp_price", "agree")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    c = config or SHIP
    qt = {"agents": [dict(AG, actions=a.get("actions", 21)) for a in c["agents"]], "environment": c["environment"]}
    return _lib.cfg_from_config(qt, n_games, 0)[0]


def sn_args(**kw):
    from th_rl_amd import _lib
    a = _lib.SampledNoiseChainArgs()
    a.n_games, a.n_tuples, a.n_prices, a.n_nodes, a.band_w, a.max_iters, a.tol = 64, 441, 441, 1121, 338, 100, 1e-12
    a.kind[1], a.prob[1], a.nprob[1], a.eps[0], a.noise_prob = 1, FAKE, FAKE, 0.01, 0.05
    for f in SN_REQUIRED:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k in ("kind", "eps", "prob", "nprob"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


SN_BAD = [dict(n_games=0), dict(flags=4), dict(flags=-1), dict(flags=3), dict(reserved=1), dict(n_tuples=0), dict(n_tuples=440),
          dict(n_prices=0), dict(n_prices=442), dict(n_nodes=1), dict(n_nodes=0), dict(band_w=0), dict(max_iters=0),
          dict(max_iters=65537), dict(tol=-1e-9), dict(tol=float("nan")), dict(eps=[-0.1]), dict(eps=[1.5]),
          dict(eps=[float("nan")]), dict(noise_prob=-0.1), dict(noise_prob=1.5), dict(noise_prob=float("nan")),
          dict(kind=[0, 4]), dict(kind=[-1, 0])]


def check_validation(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path of thrl_sampled_noise_chain that the host can see; none touches a device."""
    call = lambda c, a: lib.thrl_sampled_noise_chain(ctypes.byref(c), ctypes.byref(a), None)
    cfg = _cfg()
    for bad in SN_BAD:
        assert call(cfg, sn_args(**bad)) == -1, bad
        assert lib.thrl_last_error()
    # zero noise and both ends of the range are allowed; a per-game array takes the place of the scalar
    for ok in (dict(noise_prob=0.0), dict(noise_prob=1.0), dict(noise_prob=7.0, noise_prob_g=FAKE), dict(eps=[0.0, 7.0]),
               dict(eps=[7.0], eps_g=FAKE), dict(flags=2), dict(n_nodes=2), dict(n_nodes=4096)):
        assert call(cfg, sn_args(iters=None, **ok)) == -2, ok
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097, n_prices=1), dict(n_nodes=4097)):
        assert call(cfg, sn_args(**unsupported)) == -3, unsupported
    # the plan's edge: refused from the shape alone, with every pointer NULL
    fits, refused = plan_edge()
    for config, rc in ((fits, -2), (refused, -3)):
        ws = sp.working_set(config, resolution=1024)
        a = sn_args(n_tuples=ws["T"], n_prices=ws["D"], n_nodes=ws["Jn"], prob=[None, None], nprob=[None, None],
                    **{f: None for f in SN_REQUIRED})
        assert call(_cfg(config), a) == rc, ws
        assert (b"%d bytes of LDS" % ws["bytes"] in lib.thrl_last_error()) == (rc == -3)
    for null in SN_REQUIRED:
        assert call(cfg, sn_args(**{null: None})) == -2, null
    assert call(cfg, sn_args(nprob=[None, None])) == -2 and b"nprob[1]" in lib.thrl_last_error()
    assert call(cfg, sn_args(prob=[None, None])) == -2
    assert call(cfg, sn_args(flags=1)) == -2 and b"start" in lib.thrl_last_error()
    assert lib.thrl_sampled_noise_chain(ctypes.byref(cfg), None, None) == -2
    assert lib.thrl_sampled_noise_chain(None, ctypes.byref(sn_args()), None) == -2


def test_entry_point_validates_before_any_launch(lib):
    check_validation(lib)
