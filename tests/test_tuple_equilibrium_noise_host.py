"""Host side of the equilibrium check under demand noise in tuple form (thrl_tuple_equilibrium_noise,
th_rl_amd/tuple_analysis.py), no GPU: the mirror against independent solves on the S = T + J states (the dense chain with
numpy.linalg.solve, plain value iteration), against the merged QTable analysis on an all-QTable config, the symmetry of
tuple-states with one price, that the random strategies of the device tests make policy iteration run, option parsing,
the args struct against the header, the entry point's validation through the library loaded without a GPU, the summary
and the readers."""
import ctypes
import json
import os

import numpy as np
import pytest

import equilibrium_mirror as E
import equilibrium_noise_mirror as EN
import stationary_mirror as S
import tuple_equilibrium_noise_mirror as TM
import tuple_stationary_mirror as SM
from test_tuple_stationary_host import AG, CAC, ENV, MIXED, WIDE, _cfg, _offsets
from th_rl_amd import equilibrium as eq
from th_rl_amd import stationary as sn
from th_rl_amd import tuple_analysis as ta
from th_rl_amd import tuple_stationary as ts

Q5 = dict(AG, actions=5, states=10, gamma=0.9)
R5 = dict(name="Reinforce", gamma=0.8, actions=5, states=1, action_range=[0.2, 0.4])
# the configs of the device tests with the resolution each is run at and the seed of its random strategies (chosen on
# the mirror so that policy iteration runs: test_random_strategies_make_policy_iteration_run)
QR = {"agents": [dict(Q5), dict(R5)], "environment": dict(ENV)}                                  # T = 25, J = 24
NINE = {"agents": [dict(Q5, actions=9), dict(R5, actions=9)], "environment": dict(ENV)}          # T = 81, J = 100
TRIO = {"agents": [dict(Q5, actions=3, action_range=[0.1, 0.3]), dict(R5, actions=4, action_range=[0.05, 0.25]),
                   dict(R5, name="ActorCritic", actions=2, gamma=0.85, action_range=[0.0, 0.3])],
        "environment": dict(ENV, nplayers=3, max_steps=40)}                                        # T = 24
CASES = {"QR": (QR, 25, 16, 70, 51), "NINE": (NINE, 81, 100, 9, 52), "TRIO": (TRIO, 24, 16, 21, 53)}
QQ = {"agents": [dict(AG, states=20), dict(AG, states=20, gamma=0.9)], "environment": dict(ENV)}  # all-QTable, T = 441
U = 2.0 ** -53


def gammas(config):
    return np.array([float(a["gamma"]) for a in config["agents"]])


def strategies(tabs, n_games, seed):
    """(tuple_policy uint16 [G, N, T], cell_policy uint16 [G, N, J]) of test_tuple_stationary_host.random_strategies:
    uniform entries over the tuples, a few runs of one action over the cells, 2 % of the entries above the action count."""
    from test_tuple_stationary_host import random_strategies
    return random_strategies(tabs, n_games, seed)


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the mirror itself
@pytest.mark.parametrize("gamma,eval_tol", [(0.9, 1e-12), (0.95, 1e-9), (0.99, 1e-9)])
@pytest.mark.parametrize("name", ["QR", "NINE", "TRIO"])
def test_mirror_against_independent_solves(name, gamma, eval_tol):
    """Random strategies, every agent of 4 games.  V_pi against (I - gamma P_sigma)^-1 R_sigma on the dense chain over
    the S states, V* against value iteration run far past convergence.

    Bounds, nothing added.  e = TM.error_bound: gamma / (1 - gamma) * eval_tol of truncation plus (W + 3) u max|V| /
    (1 - gamma) of rounding (derived there: S does not enter, a state's value is read back from its tuple's, and only
    the band sum grows with W).  V_pi: e.  V*: the iteration stops when no action's Q exceeds the incumbent's by more
    than margin, both Q within gamma e of the true ones, so the last strategy's Bellman residual is at most d = margin +
    2 gamma e and its value within d / (1 - gamma) of the optimum: e + d / (1 - gamma)."""
    config, T, res, _, seed = CASES[name]
    tabs = ts.tables(config, res)
    N, W, G = len(config["agents"]), tabs["band_w"], 4
    tpol, cpol = strategies(tabs, G, seed)
    out = TM.analyse(tabs, tpol, cpol, 0.05, gamma=np.full(N, gamma), eval_tol=eval_tol)
    assert (out["iters"] >= 0).all() and out["iters"].max() <= 12 and tabs["n_tuples"] == T
    tup = TM.state_tuples(tabs, tpol, cpol)
    worst_pi = worst_opt = 0.0
    for g in range(G):
        for i in range(N):
            R, P, pk = TM.dense(tabs, tup[g], i, 0.05)
            assert np.abs(P.sum(axis=2) - 1.0).max() <= (W + 2) * 2 * U
            vd = TM.direct_value(R, P, pk, gamma)
            vi = TM.value_iteration(R, P, gamma)
            e = TM.error_bound(gamma, eval_tol, W, np.abs(vi).max())
            d = float(TM.margin_of(gamma, eval_tol)) + 2.0 * gamma * e
            err_pi = np.abs(out["v_pi"][i, g] - vd).max()
            err_opt = np.abs(out["v_opt"][i, g] - vi).max()
            worst_pi, worst_opt = max(worst_pi, err_pi / e), max(worst_opt, err_opt / (e + d / (1.0 - gamma)))
            assert err_pi <= e, (g, i, err_pi, e)
            assert err_opt <= e + d / (1.0 - gamma), (g, i, err_opt)
            assert (out["v_opt"][i, g] >= out["v_pi"][i, g] - 2 * e).all()
    print("%s gamma %g eval_tol %g: rounds <= %d, sweeps <= %d, max |V_pi - direct| / bound = %.3f, max |V* - VI| / bound = %.3f"
          % (name, gamma, eval_tol, out["iters"].max(), out["sweeps"].max(), worst_pi, worst_opt))


def _qtable_strategies(config, tabs_q, policy):
    """The strategies of an all-QTable game in tuple form, from its policy entries [G, P]: a cell's entry is the one at
    the cell's row, a tuple-state's the one at the row of the tuple's noise-free price, which is its det_cell's row."""
    pl = E.plan(config)
    roff = np.concatenate([[0], np.cumsum([p["states"] + 1 for p in pl["ag"]])])
    cp = np.stack([policy[:, roff[i] + np.asarray(tabs_q["cell_rows"][i], np.int64)] for i in range(pl["N"])], axis=1)
    return np.ascontiguousarray(cp[:, :, np.asarray(tabs_q["det_cell"])]).astype(np.uint16), cp.astype(np.uint16)


def test_all_qtable_game_against_the_qtable_analysis():
    """resolution = 0 on an all-QTable config whose tuple prices sit on no tie breakpoint (no point cell): the cells are
    thrl_stationary's.  V_pi on cell k is the QTable analysis' V_pi[k] and on tuple-state t its V_pi[det_cell(t)], each
    within the sum of the two evaluations' bounds; V* here is at least the QTable one less that sum, because the strategy
    space here is larger (the agent may act at a tuple's exact price otherwise than in the cell around it)."""
    tq, tt = sn.tables(QQ), ts.tables(QQ, 0)
    J, T, W = tq["n_cells"], tq["n_tuples"], tq["band_w"]
    det = np.asarray(tq["det_cell"])
    assert tq["n_intervals"] == J == tt["n_cells"] and ((det >= 0) & (det < J)).all()       # no tie breakpoint is hit
    assert np.array_equal(tq["band"], tt["band"]) and np.array_equal(tq["band_lo"], tt["band_lo"])
    G = 3
    policy = S.policies(QQ, S.fresh_tables(QQ, G, 7))
    tpol, cpol = _qtable_strategies(QQ, tq, policy)
    assert np.array_equal(SM.tuple_of(tt, cpol), S.cell_tuples(QQ, policy, tq, G))
    ref = EN.analyse(QQ, tq, policy, 0.05)
    out = TM.analyse(tt, tpol, cpol, 0.05, gamma=gammas(QQ))
    assert (ref["iters"] >= 0).all() and (out["iters"] >= 0).all()
    for i, gamma in enumerate(gammas(QQ)):
        both = 2.0 * TM.error_bound(gamma, 1e-12, W, np.abs(ref["v_opt"][i]).max())
        d = float(TM.margin_of(gamma, 1e-12)) + gamma * both
        assert np.abs(out["v_pi"][i][:, T:] - ref["v_pi"][i]).max() <= both
        assert np.abs(out["v_pi"][i][:, :T] - ref["v_pi"][i][:, det]).max() <= both
        # both are within e + d / (1 - gamma) of their own optimum (the bound of the test above), the larger space's
        # optimum is no smaller
        slack = both + 2.0 * d / (1.0 - gamma)
        assert (out["v_opt"][i][:, T:] >= ref["v_opt"][i] - slack).all()
        assert (out["v_opt"][i][:, :T] >= ref["v_opt"][i][:, det] - slack).all()


def test_tuple_states_with_one_price_are_one_state():
    """Tuple-states with bitwise equal price at which every agent's entry is equal get equal br_policy, v_opt and v_pi:
    strategies that are functions of the price, as every extracted one is."""
    # actions on a dyadic grid, so that every quantity and price is exact and (a, b) and (b, a) share a price bit for bit
    # (two QTable agents: the two kinds of agent scale their actions differently)
    exact = {"agents": [dict(Q5, action_range=[0.25, 0.5]), dict(Q5, action_range=[0.25, 0.5], gamma=0.8)],
             "environment": dict(ENV)}
    tabs = ts.tables(exact, 16)
    T, J, G = tabs["n_tuples"], tabs["n_cells"], 5
    price = np.asarray(tabs["price"])
    _, cls = np.unique(price.view(np.uint64), return_inverse=True)
    assert cls.max() + 1 == 9 and T == 25                        # a + b in 0..8
    rs = np.random.RandomState(11)
    tpol = np.stack([rs.randint(0, 5, (G, cls.max() + 1))[:, cls] for _ in range(2)], axis=1).astype(np.uint16)
    _, cpol = strategies(tabs, G, 12)
    out = TM.analyse(tabs, tpol, cpol, 0.05, gamma=gammas(QR))
    assert (out["iters"] >= 0).all()
    first = np.array([np.flatnonzero(cls == c)[0] for c in cls])
    for f in TM.STATE_FIELDS:
        x = out[f][:, :, :T]
        assert np.array_equal(x, x[:, :, first]), f


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_strategies_make_policy_iteration_run(name):
    """What the device tests rely on, asserted on the mirror: with their seeds some (agent, game) needs two rounds or
    more and changes its action in some cell, and none is capped."""
    config, T, res, G, seed = CASES[name]
    tabs = ts.tables(config, res)
    tpol, cpol = strategies(tabs, G, seed)
    out = TM.analyse(tabs, tpol, cpol, 0.05, gamma=gammas(config))
    assert (out["iters"] >= 0).all() and (out["iters"] >= 2).any() and (out["n_diff_cells"] > 0).any()
    assert (out["n_diff_tuples"] > 0).any() and (out["loss_all"] > 0).any()
    print("%s: T %d, J %d, W %d, rounds %d..%d, sweeps <= %d" % (name, T, tabs["n_cells"], tabs["band_w"],
                                                                 out["iters"].min(), out["iters"].max(), out["sweeps"].max()))
    if name == "NINE":
        assert T > 64 and T % 64 and tabs["n_cells"] > 64 and tabs["n_cells"] % 64


def test_not_solved_rules_and_weights_on_the_mirror():
    tabs = ts.tables(QR, 16)
    T, J, G = tabs["n_tuples"], tabs["n_cells"], 6
    tpol, cpol = strategies(tabs, G, 3)
    pi = SM.analyse(tabs, tpol, cpol, 0.05)["pi"]
    out = TM.analyse(tabs, tpol, cpol, 0.05, gamma=gammas(QR), max_sweeps=16, pi=pi)
    assert (out["iters"] == -1).all() and (out["sweeps"] == 16).all() and not out["n_diff_cells"].any()
    assert np.isnan(out["loss_all"]).all() and np.isnan(out["v_w"]).all() and np.isnan(out["v_opt"]).all()
    gam = np.repeat(gammas(QR)[:, None], G, axis=1)
    gam[0, 1], gam[1, 2] = 1.0, -0.1
    p = np.array([0.05, 0.05, 0.05, 0.0, np.nan, 1.0])
    out = TM.analyse(tabs, tpol, cpol, p, gamma=gam, pi=pi)
    assert out["iters"][0, 1] == -1 and out["iters"][1, 2] == -1 and np.isnan(out["loss_w"][0, 1]) and out["sweeps"][0, 1] == 0
    assert out["iters"][1, 1] >= 0 and out["iters"][0, 2] >= 0 and (out["iters"][:, [0, 5]] >= 0).all()
    for f in TM.INT_FIELDS + TM.FLOAT_FIELDS + TM.W_FIELDS + TM.STATE_FIELDS:
        assert (np.asarray(out[f])[:, 3:5] == (-1 if f == "iters" else 0)).all(), f
    # the weights are a distribution over where decisions are made: q at the tuple prices, p in the cells
    w = TM.weights_of(tabs, pi, np.full(G, 0.05))
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-12 and np.abs(w[:, :T].sum(axis=1) - 0.95).max() <= 1e-12
    every = TM.analyse(tabs, tpol, cpol, 0.05, gamma=gammas(QR), pi=pi)
    assert (every["diff_w"] <= 1.0 + 1e-12).all() and (every["loss_w"] <= every["loss_all"] + 1e-15).all()


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_with_noise():
    noisy = dict(MIXED, environment=dict(ENV, noise_prob=0.05))
    base = dict(tol=0.0, policies=False, agents=[0, 1])
    assert ta.parse_equilibrium_options(True, MIXED) == base                # pinned: nothing appears unless given
    assert ta.parse_equilibrium_options({"noise": None}, MIXED) == base and ta.parse_equilibrium_options({"noise": False}, MIXED) == base
    assert ta.NOISE_DEFAULTS == dict(noise_prob=None, eval_tol=1e-12, max_sweeps=8192, resolution=1024)
    assert ta.parse_equilibrium_options({"noise": True}, noisy) == dict(base, noise=ta.NOISE_DEFAULTS)
    got = ta.parse_equilibrium_options({"agents": [1], "noise": {"noise_prob": 0.2, "eval_tol": 0, "max_sweeps": 100,
                                                                   "resolution": 32}}, MIXED)
    assert got == dict(agents=[1], tol=0.0, policies=False,
                       noise=dict(noise_prob=0.2, eval_tol=0.0, max_sweeps=100, resolution=32))
    swept = dict(MIXED, training={"sweep": {"noise_prob": [0.1]}})
    assert ta.parse_equilibrium_options({"noise": True}, swept)["noise"]["noise_prob"] is None
    with pytest.raises(ValueError, match=r"training\.greedy_equilibrium\.noise: the environment has noise_prob = 0: give"):
        ta.parse_equilibrium_options({"noise": True}, MIXED)
    for bad in ({"tables": "final"}, {"noise_prob": 0}, {"noise_prob": 1.5}, {"noise_prob": "x"}, {"noise_prob": True},
                {"eval_tol": -1}, {"eval_tol": "a"}, {"eval_tol": True}, {"eval_tol": float("nan")}, {"max_sweeps": 0},
                {"max_sweeps": 65537}, {"max_sweeps": 1.5}, {"max_sweeps": True}, {"resolution": -1}, {"resolution": 1.5},
                {"resolution": True}, {"resolution": 4096}, 5, "yes"):
        with pytest.raises(ValueError, match="greedy_equilibrium"):
            ta.parse_equilibrium_options({"noise": bad}, noisy)
    with pytest.raises(ValueError, match="continuous"):
        ta.parse_equilibrium_options({"noise": True}, dict(CAC, environment=dict(ENV, noise_prob=0.05)))
    with pytest.raises(ValueError, match="4096"):
        ta.parse_equilibrium_options({"noise": True}, dict(WIDE, environment=dict(ENV, noise_prob=0.05)))
    # train_one refuses before it builds a batch (no GPU is touched)
    from th_rl_amd import trainer
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "c.json"), "w").write(json.dumps(dict(MIXED, training={"epochs": 1, "n_games": 4,
                                                                                      "greedy_equilibrium": {"noise": True}})))
        with pytest.raises(ValueError, match="noise_prob = 0"):
            trainer.train_one(os.path.join(d, "run"), os.path.join(d, "c.json"))


# ------------------------------------------------------------------------------------------------ the entry point
FAKE = 4096                           # never dereferenced: validation fails before any launch
TABLES = ("tuple_policy", "cell_policy", "reward", "band_lo", "band", "noise_reward")
OUTPUTS = ("iters", "sweeps", "n_diff_tuples", "n_diff_cells", "loss_all", "loss_tuples_mean", "loss_cells_mean")
WEIGHTED = ("loss_w", "diff_w", "v_w")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleEquilibriumNoiseArgs()
    a.n_games, a.n_tuples, a.n_cells, a.band_w, a.max_sweeps, a.agents = 64, 441, 101, 31, 8192, 3
    a.eval_tol, a.noise_prob = 1e-12, 0.05
    a.gamma[0], a.gamma[1] = 0.95, 0.995
    for f in TABLES + OUTPUTS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k in ("kind", "gamma"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


BAD = [dict(n_games=0), dict(n_games=-3), dict(flags=1), dict(reserved=1), dict(agents=0), dict(agents=4), dict(n_tuples=0),
       dict(n_tuples=440), dict(kind=[0, 4]), dict(kind=[-1, 0]), dict(gamma=[1.0, 0.5]), dict(gamma=[0.5, -0.1]),
       dict(gamma=[float("nan"), 0.5]), dict(n_cells=0), dict(band_w=0), dict(max_sweeps=0), dict(max_sweeps=65537),
       dict(eval_tol=-1e-12), dict(eval_tol=float("nan")), dict(noise_prob=0.0), dict(noise_prob=1.5),
       dict(noise_prob=float("nan")), dict(noise_prob=-0.05)]


@pytest.mark.parametrize("bad", BAD)
def test_bad_arguments_are_bad_config(lib, bad):
    assert lib.thrl_tuple_equilibrium_noise(ctypes.byref(_cfg()), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", ("cfg", "args") + TABLES + OUTPUTS + WEIGHTED)
def test_missing_pointers_are_null(lib, null):
    kw = {} if null in ("cfg", "args") else {null: None}
    if null in WEIGHTED:
        kw = dict({f: FAKE for f in WEIGHTED}, pi=FAKE, **kw)
    c = None if null == "cfg" else ctypes.byref(_cfg())
    a = None if null == "args" else ctypes.byref(_args(**kw))
    assert lib.thrl_tuple_equilibrium_noise(c, a, None) == -2


def test_gamma_limits_and_working_set(lib):
    from th_rl_amd import _lib
    call = lambda a, c=None: lib.thrl_tuple_equilibrium_noise(ctypes.byref(c or _cfg()), ctypes.byref(a), None)
    # the gamma of an agent that is not solved is not read, and a device array takes the place of the host's
    assert call(_args(gamma=[1.5, 0.5], agents=2, iters=None)) == -2 and b"iters" in lib.thrl_last_error()
    assert call(_args(gamma=[1.5, 1.5], sweep_gamma=FAKE, iters=None)) == -2
    # cfg.gamma is not read at all: the table slot of a network is a placeholder
    over = _cfg({"agents": [dict(AG), dict(AG, gamma=0.5)], "environment": dict(ENV)})
    over.gamma[1] = 7.0
    assert call(_args(iters=None), over) == -2
    # a per-game noise array takes the place of the scalar; without pi the weighted outputs may be NULL
    assert call(_args(noise_prob=0.0, noise_prob_g=FAKE, sweeps=None)) == -2 and b"sweeps" in lib.thrl_last_error()
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097), dict(n_cells=4097)):
        assert call(_args(**unsupported)) == _lib.ERR_UNSUPPORTED, unsupported
    wide = _cfg({"agents": [dict(AG, actions=129), dict(AG, actions=32)], "environment": dict(ENV)})
    assert call(_args(n_tuples=4128), wide) == _lib.ERR_UNSUPPORTED
    # the working set, 44 T + 28 J + 2048 rounded up to 16 bytes against 160 KB: with T = 441, J = 4096 fits; with
    # T = 4096, J = 1 does not (180,224 + 28 + 2048), nor does the last J that would fit at T = 2304 plus one
    need = lambda T, J: (44 * T + 28 * J + 2048 + 15) // 16 * 16
    assert need(441, 4096) == 136144 <= _lib.TEN_MAX_LDS == 160 * 1024
    assert call(_args(n_cells=4096, iters=None)) == -2 and b"iters" in lib.thrl_last_error()
    big = _cfg({"agents": [dict(AG, actions=128), dict(AG, actions=32)], "environment": dict(ENV)})
    assert call(_args(n_tuples=4096, n_cells=1), big) == _lib.ERR_UNSUPPORTED and b"LDS" in lib.thrl_last_error()
    mid = _cfg({"agents": [dict(AG, actions=72), dict(AG, actions=32)], "environment": dict(ENV)})      # T = 2304
    jmax = (_lib.TEN_MAX_LDS - 2048 - 44 * 2304) // 28
    assert need(2304, jmax) <= _lib.TEN_MAX_LDS < need(2304, jmax + 1)
    assert call(_args(n_tuples=2304, n_cells=jmax, iters=None), mid) == -2
    assert call(_args(n_tuples=2304, n_cells=jmax + 1, iters=None), mid) == _lib.ERR_UNSUPPORTED
    assert str(need(2304, jmax + 1)).encode() in lib.thrl_last_error()


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    got, mine = _offsets(_lib.TupleEquilibriumNoiseArgs, "thrl_tuple_equilibrium_noise_args",
                         ["THRL_TEN_MAX_LDS", "THRL_STAT_MAX_CELLS", "THRL_STAT_MAX_ITERS", "THRL_EQ_MAX_ITERS",
                          "THRL_TP_MAX_TUPLES", "THRL_ABI_VERSION"])
    assert got == mine[:1] + [_lib.TEN_MAX_LDS, _lib.STAT_MAX_CELLS, _lib.STAT_MAX_ITERS, _lib.EQ_MAX_ITERS, 4096, 4] + mine[1:]
    assert "thrl_tuple_equilibrium_noise" in _lib.SYMBOLS and TM.MAX_ITERS == _lib.EQ_MAX_ITERS and _lib.ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------ summary, readers
def _games(G=10, weights=True):
    rs = np.random.RandomState(4)
    g = dict(iters=rs.randint(0, 4, (2, G)).astype(np.int32), sweeps=rs.randint(500, 3000, (2, G)).astype(np.int32),
             n_diff_tuples=rs.randint(0, 21, (2, G)).astype(np.int32), n_diff_cells=rs.randint(0, 9, (2, G)).astype(np.int32),
             loss_all=rs.uniform(0, 0.4, (2, G)), loss_tuples_mean=rs.uniform(0, 0.1, (2, G)),
             loss_cells_mean=rs.uniform(0, 0.1, (2, G)), noise_prob=np.full(G, 0.05))
    if weights:
        g.update(loss_w=rs.uniform(0, 0.2, (2, G)), diff_w=rs.uniform(0, 1, (2, G)), v_w=rs.uniform(200, 250, (2, G)))
    for f in ("loss_all", "loss_tuples_mean", "loss_cells_mean") + (("loss_w", "diff_w") if weights else ()):
        g[f][:, [0, 5]] = 0.0
    g["iters"][:, [0, 5]] = 0
    g["iters"][0, 3] = -1                       # capped
    return g


def test_summary_artefacts_and_readers(tmp_path):
    from th_rl_amd import utils
    G = 10
    g = _games(G)
    ids = np.array([0] * 5 + [1] * 5)
    fl = eq.flags_noise(g, [0, 1])
    assert fl["br_all"][1].tolist() == [True] + [False] * 4 + [True] + [False] * 4 and not fl["br_all"][0, 3]
    rows = ta.summarize_equilibrium_noise(g, ids, 2, [0, 1], 0.0)
    base = eq.summarize_noise(g, ids, 2, [0, 1], 0.0)
    assert [(r["group"], r["agent"]) for r in rows] == [(0, 0), (0, 1), (0, None), (1, 0), (1, 1), (1, None)]
    for r, b in zip(rows, base):
        assert {k: r[k] for k in b} == b
    assert rows[0]["capped"] == 1 and rows[0]["diff_tuples_mean"] == float(g["n_diff_tuples"][0][[0, 1, 2, 4]].mean())
    assert rows[1]["diff_cells_mean"] == float(g["n_diff_cells"][1][:5].mean()) and "diff_cells_mean" not in rows[2]
    bare = ta.summarize_equilibrium_noise(_games(weights=False), ids, 2, [0, 1])
    assert bare[0]["br_w"] is None and bare[0]["diff_w_mean"] is None and bare[0]["br_all"] == 1 / 5
    rs = np.random.RandomState(6)
    full = dict(g, br_policy=rs.randint(0, 5, (2, G, 51)).astype(np.uint16), v_opt=rs.uniform(20, 25, (2, G, 51)),
                v_pi=rs.uniform(20, 25, (2, G, 51)))
    d = tmp_path / "run"
    d.mkdir()
    ta.save_equilibrium_noise_games(str(d), full)
    assert sorted(f.name for f in d.iterdir()) == ["geqn_iters.npy", "geqn_loss.npy", "geqn_policy.npy", "geqn_prob.npy",
                                                   "geqn_v_opt.npy", "geqn_v_pi.npy", "geqn_weighted.npy"]
    back = ta.load_equilibrium_noise_games(str(d))
    assert set(back) == set(full)
    for f in full:
        assert np.array_equal(back[f], full[f]) and back[f].dtype == full[f].dtype, f
    assert np.load(d / "geqn_iters.npy").shape == (4, 2, G) and np.load(d / "geqn_loss.npy").shape == (3, 2, G)
    noisy = dict(MIXED, environment=dict(ENV, noise_prob=0.05))
    opt = ta.parse_equilibrium_options({"policies": True, "noise": True}, noisy)
    (d / "config.json").write_text(json.dumps(dict(noisy, training={"n_games": G})))
    ta.an.save_json(str(d / "greedy_equilibrium_noise.json"),
                    {"options": opt, "n_cells": 26, "T": 25, "quantiles": [0.25, 0.5, 0.75],
                     "summary": [r for r in rows if r["agent"] is not None], "perfect": [r for r in rows if r["agent"] is None]})
    df = utils.greedy_equilibrium_noise_summary(str(d))
    assert len(df) == 6 and df["n_cells"].tolist() == [26] * 6 and df["T"].tolist() == [25] * 6 and df["tol"].tolist() == [0.0] * 6
    a = utils.greedy_equilibrium_noise_games(str(d), 1)
    assert a.index.tolist() == list(range(G)) and a["loss_w"].tolist() == g["loss_w"][1].tolist()
    assert a["n_diff_cells"].tolist() == g["n_diff_cells"][1].tolist() and a["perfect"].tolist() == fl["perfect"].tolist()
    assert utils.greedy_equilibrium_noise_games(str(d))["br_all"].tolist() == fl["br_all"][0].tolist()
    with pytest.raises(KeyError, match=r"\(geqn_iters.npy\) under .* \(training\.greedy_equilibrium\.noise\)"):
        utils.greedy_equilibrium_noise_games(str(tmp_path / "none"), 0)
    with pytest.raises(KeyError, match=r"\(greedy_equilibrium_noise.json\)"):
        utils.greedy_equilibrium_noise_summary(str(tmp_path / "none"))


def test_batch_method_is_shared_and_documented():
    from th_rl_amd import analysis
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    fn = analysis.AnalysisMethods.greedy_equilibrium_noise
    assert GameBatch.greedy_equilibrium_noise is fn and MixedGameBatch.greedy_equilibrium_noise is fn
    assert "thrl_tuple_equilibrium_noise" in fn.__doc__ and len(analysis.REGISTRY) == 12
    assert [a.key for a in analysis.REGISTRY].count("greedy_equilibrium") == 1
