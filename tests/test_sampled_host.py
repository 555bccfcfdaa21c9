"""Host side of sampled play (th_rl_amd.sampled_play, thrl_price_probs, thrl_sampled_chain): the per-config tables, the
numpy mirror's hand answers, that the random networks of the device tests are no degenerate input for it, option parsing
and refusals, the summary rows and artefacts, the ctypes mirrors of the args structs against the header and both entry
points' validation through the library loaded without a GPU.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

import sampled_mirror as SPM
from sampled_mirror import AG, CAC, CASES, ENV, QQ, QR, QRA, RF, RR, SHIP, WIDE
from test_tuple_stationary_host import _offsets
from th_rl_amd import sampled_play as sp

FAKE = 4096                           # never dereferenced: validation fails before any launch


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def case_inputs(name):
    """(tabs, probs by numpy, dpolicy, eps [N, G], start [G]) of CASES[name]: what the device tests use, with the
    networks evaluated on the host."""
    def make():
        config, T, n_games, _, seed = CASES[name]
        tabs = sp.tables(config)
        w = SPM.case_weights(name, tabs)
        probs = {i: SPM.net_probs(w[i], int(tabs["n_actions"][i]), tabs["dprice"]) for i in w}
        pol = SPM.greedy_of(probs, tabs, np.random.RandomState(seed + 100), n_games)
        return tabs, probs, pol, SPM.case_epsilon(name, tabs), SPM.case_starts(name, tabs)
    return SPM.cached(("host inputs", name), make)


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", ["QR", "QRA", "SHIP", "QQ", "RR"])
def test_tables_group_the_tuples_by_price(name):
    config = CASES[name][0] if name in CASES else RR
    t = sp.tables(config)
    T, D = t["n_tuples"], t["n_prices"]
    bits = t["price"].view(np.int64)
    assert D == len(set(bits.tolist())) and t["dprice"].shape == (D,) and (np.diff(t["dprice"]) > 0).all()
    assert t["row"].dtype == np.int32 and np.array_equal(t["dprice"][t["row"]].view(np.int64), bits)
    first, perm = t["grp_first"], t["grp_perm"]
    assert first.shape == (D + 1,) and first[0] == 0 and first[-1] == T and (np.diff(first) >= 1).all()
    assert sorted(perm.tolist()) == list(range(T))
    for d in range(D):
        grp = perm[first[d]:first[d + 1]]
        assert (t["row"][grp] == d).all() and (np.diff(grp) > 0).all()
    from th_rl_amd import tuple_play as tp
    base = tp.tables(config)
    assert all(np.array_equal(t[f], base[f]) for f in ("price", "reward", "scaled"))
    if name == "RR":
        assert (T, D) == (441, 41)                                        # A0 + A1 - 1 on equal exact grids
    if name == "SHIP":
        assert (T, D) == (441, 441)
    if name == "QQ":
        assert (T, D) == (4, 3) and t["dprice"].tolist() == [2.0, 4.0, 6.0] and first.tolist() == [0, 1, 3, 4]


def test_working_set_follows_the_header():
    ws = sp.working_set(SHIP)
    r16 = lambda x: (x + 15) & ~15
    assert ws["bytes"] == 2 * r16(8 * 441) + 2 * r16(8 * 441) + r16(2 * 441) + r16(4 * 441 * 21) + r16(2 * 442) + r16(2 * 441) \
        + 512 * 6 + 256 and ws["fits"] and (ws["T"], ws["D"]) == (441, 441)
    assert sp.working_set(RR)["fits"] and sp.working_set(RR)["D"] == 41
    big = lambda aq: {"agents": [dict(AG, actions=aq), dict(RF, actions=32)], "environment": dict(ENV)}
    assert sp.working_set(big(30))["fits"] and not sp.working_set(big(32))["fits"]
    assert sp.working_set(big(32))["bytes"] > sp.MAX_LDS == 160 * 1024


# ------------------------------------------------------------------------------------------------ mirror, hand answers
def test_rows_that_ignore_the_price_give_the_product_after_one_step():
    t = sp.tables(QRA)
    D = t["n_prices"]
    p1 = np.array([0.2, 0.5, 0.3], np.float32)
    p2 = np.array([0.75, 0.25], np.float32)
    probs = {1: np.tile(p1, (3, D, 1)), 2: np.tile(p2, (3, D, 1))}
    pol = np.zeros((3, 3, D), np.uint16)
    pol[:, 0] = 1                                                         # the QTable agent's greedy action everywhere
    eps = 0.2
    q0 = np.array([eps / 2, (1 - eps) + eps / 2])
    want = (q0[:, None, None] * p1.astype(np.float64)[None, :, None] * p2.astype(np.float64)[None, None, :]).reshape(-1)
    want = want / (p1.astype(np.float64).sum() * p2.astype(np.float64).sum())
    for start in (None, [0, 5, 11]):
        r = SPM.analyse(t, probs, pol, [eps, 0, 0], start=start, max_iters=1)
        m0 = np.full((3, 12), 1 / 12.0) if start is None else np.eye(12)[start]
        assert np.abs(2 * r["pi"] - m0 - want[None, :]).max() < 1e-15
    r = SPM.analyse(t, probs, pol, [eps, 0, 0], tol=1e-13)
    assert (r["iters"] < 64).all() and np.abs(r["pi"] - want[None, :]).max() < 1e-12
    assert np.abs(r["samp_reward"][:, 0] - t["reward"] @ want).max() < 1e-11
    assert np.abs(r["agree"] - q0[1] * float(p1[0]) * 0.75 / (p1.astype(np.float64).sum() * p2.astype(np.float64).sum())).max() < 1e-12


def test_a_two_cycle_gets_half_and_half_only_through_the_lazy_form():
    t = sp.tables(QQ)                                                     # prices [2, 4, 6] <- tuples 3, {1, 2}, 0
    pol = np.array([[[0, 0, 1], [0, 0, 1]]], np.uint16)                   # after tuple 0 (price 6) play (1, 1) = tuple 3; after 3, 0
    for start in ([0], [3], [1], None):
        r = SPM.analyse(t, {}, pol, [0.0, 0.0], start=start, tol=1e-12, max_iters=500)
        assert r["iters"][0] < 500 and np.abs(r["pi"][0] - [0.5, 0, 0, 0.5]).max() < 1e-9
        assert abs(r["agree"][0] - 1.0) < 1e-12 and abs(r["mass"][0] - 1.0) < 1e-12      # degenerate rows: always greedy
        assert np.abs(r["samp_reward"][:, 0] - 0.5 * (t["reward"][:, 0] + t["reward"][:, 3])).max() < 1e-8
    P, Z, _ = SPM.rows_of(t, {}, pol, [0.0, 0.0])
    m = np.array([[1.0, 0, 0, 0]])
    new, _ = SPM.step(t, P, Z, SPM.actions_of(t), m)                      # the plain iteration m' = s flips for ever
    assert (2 * new - m)[0].tolist() == [0, 0, 0, 1.0]


def test_epsilon_one_is_uniform_and_refused_games_are_zero():
    t = sp.tables(QQ)
    pol = SPM.random_dpolicy(np.random.RandomState(2), 6, t)
    r = SPM.analyse(t, {}, pol, [1.0, 1.0], start=[0, 1, 2, 3, 0, 1], max_iters=1)
    assert np.abs(2 * r["pi"] - np.eye(4)[[0, 1, 2, 3, 0, 1]] - 0.25).max() < 1e-16 and (r["iters"] == 1).all()
    assert np.abs(r["agree"] - 0.25).max() < 1e-15
    eps = np.array([[0.1, np.nan, 0.2, 1.5, 0.0, 0.3], [0.1, 0.1, -0.1, 0.2, 1.0, 0.3]])
    r = SPM.analyse(t, {}, pol, eps, start=[0, 1, 2, 3, 4, -1], max_iters=7)
    assert r["iters"].tolist() == [7, -1, -1, -1, -1, -1]
    assert not r["pi"][1:].any() and not r["samp_reward"][:, 1:].any() and not r["mass"][1:].any() and not r["agree"][1:].any()
    assert abs(r["mass"][0] - 1.0) < 1e-15


@pytest.mark.parametrize("name", SPM.NETWORK_CASES)
def test_random_networks_carry_the_coverage(name):
    """The inputs the device is compared on are no degenerate chains: in at least half of the 203 games the final
    distribution is concentrated (max_t pi >= 4 / T) after more than one step, and at least 5 % of the probability rows
    are peaked (max_k P >= 0.9): fc_pi is scaled by 8 in three games of four."""
    config, T, n_games, max_iters, _ = CASES[name]
    tabs, probs, pol, eps, start = case_inputs(name)
    assert n_games == 203 and tabs["n_tuples"] == T
    r = SPM.cached(("host uniform", name), lambda: SPM.analyse(tabs, probs, pol, eps, tol=1e-12, max_iters=max_iters))
    share = np.mean((r["pi"].max(axis=1) >= 4.0 / T) & (r["iters"] > 1))
    rows = np.concatenate([p.max(axis=2).ravel() for p in probs.values()])
    print("%s: concentrated %.2f, peaked rows %.2f, agree %.3f..%.3f, iters %d..%d"
          % (name, share, np.mean(rows >= 0.9), r["agree"].min(), r["agree"].max(), r["iters"].min(), r["iters"].max()))
    assert share >= 0.5
    assert np.mean(rows >= 0.9) >= 0.05
    assert (np.abs(r["mass"] - 1.0) < 1e-12).all() and (r["agree"] > 0).all() and (r["agree"] <= 1.0 + 1e-12).all()
    assert all((pol[:, i] >= A).any() for i, A in enumerate(tabs["n_actions"]) if tabs["kinds"][i] == "QTable")


# ------------------------------------------------------------------------------------------------ options, refusals
def test_parse_options():
    assert sp.parse_options(True, SHIP) == sp.DEFAULTS
    got = sp.parse_options({"epsilon": 0, "start": "state", "tol": 0, "max_iters": 5, "pi": True}, SHIP)
    assert got == dict(epsilon=0.0, start="state", tol=0.0, max_iters=5, pi=True)
    assert sp.parse_options({"epsilon": [0.1, 0]}, SHIP)["epsilon"] == [0.1, 0.0]
    with pytest.raises(ValueError, match=r"unknown keys \['noise_prob'\]"):
        sp.parse_options({"noise_prob": 0.05}, SHIP)
    for bad in ({"epsilon": -0.1}, {"epsilon": 1.5}, {"epsilon": True}, {"epsilon": "final"}, {"epsilon": [0.1]},
                {"epsilon": [0.1, 2]}, {"start": "reset"}, {"tol": -1}, {"tol": "x"}, {"max_iters": 0}, {"max_iters": 1 << 17},
                {"max_iters": 2.0}, {"pi": 1}, 7, "yes"):
        with pytest.raises(ValueError, match="sampled_play"):
            sp.parse_options(bad, SHIP)
    with pytest.raises(ValueError, match="continuous"):
        sp.parse_options(True, CAC)
    with pytest.raises(ValueError, match="4096"):
        sp.parse_options(True, WIDE)
    with pytest.raises(ValueError, match="working set is .* bytes"):
        sp.parse_options(True, {"agents": [dict(AG, actions=32), dict(RF, actions=32)], "environment": dict(ENV)})


def test_refused_under_launch():
    from th_rl_amd import launch
    with pytest.raises(ValueError, match="sampled_play is not available under th_rl_amd.launch"):
        launch.check_launch_config(dict(SHIP, training={"n_games": 8, "sampled_play": True}))
    launch.check_launch_config(dict(SHIP, training={"n_games": 8, "sampled_play": False}))


def test_summary_rows_and_artefacts(tmp_path):
    rs = np.random.RandomState(5)
    n = 6
    g = {"iters": np.array([3, 9, -1, 10, 10, 4], np.int32), "change": rs.rand(n), "mass": np.ones(n), "samp_price": rs.rand(n),
         "agree": np.array([.5, .7, 0, .2, .4, .6]), "samp_reward": rs.rand(2, n) + 2.0, "samp_action": rs.rand(2, n),
         "epsilon": np.full((2, n), 0.01)}
    rows = sp.summarize(g, [0, 0, 0, 1, 1, 1], 2, 2.0, 4.0, 10)
    assert [r["games"] for r in rows] == [3, 3] and rows[0]["converged"] == 2.0 / 3.0 and rows[1]["converged"] == 1.0 / 3.0
    assert abs(rows[0]["agree_mean"] - 0.6) < 1e-15 and rows[0]["iters_max"] == 9 and "delta_greedy_mean" not in rows[0]
    delta = (g["samp_reward"].sum(axis=0) - 2.0) / 2.0
    assert abs(rows[0]["delta_sampled_mean"] - delta[:2].mean()) < 1e-15
    assert abs(rows[1]["price_mean"] - g["samp_price"][3:].mean()) < 1e-15
    cr, lam = rs.rand(2, n) + 2.5, np.array([1, 0, 2, 1, 1, 3])
    rows = sp.summarize(g, [0, 0, 0, 1, 1, 1], 2, 2.0, 4.0, 10, cycle_reward=(cr, lam))
    dg = (cr.sum(axis=0) - 2.0) / 2.0
    assert abs(rows[0]["delta_greedy_mean"] - dg[0]) < 1e-15                              # game 1 has no cycle, 2 is refused
    assert abs(rows[1]["randomness_cost_mean"] - (dg[3:] - delta[3:]).mean()) < 1e-15
    json.dumps(rows)
    sp.save_games(str(tmp_path), g)
    assert sorted(os.listdir(tmp_path)) == ["splay_action.npy", "splay_epsilon.npy", "splay_games.npy", "splay_iters.npy",
                                            "splay_reward.npy"]
    back = sp.load_games(str(tmp_path))
    assert sorted(back) == sorted(g) and all(np.array_equal(back[f], g[f]) for f in g)
    full = dict(g, pi=rs.rand(n, 4), start=np.arange(n, dtype=np.int32))
    sp.save_games(str(tmp_path), full)
    back = sp.load_games(str(tmp_path))
    assert sorted(back) == sorted(full) and all(np.array_equal(back[f], full[f]) for f in full)
    both = sp.combine([{f: (v[:2] if f == "pi" else v[..., :2]) for f, v in full.items()},
                       {f: (v[2:] if f == "pi" else v[..., 2:]) for f, v in full.items()}])
    assert all(np.array_equal(both[f], full[f]) for f in full)
    sp.save_games(str(tmp_path), g)                                       # an earlier run's pi and start do not stay
    assert sorted(sp.load_games(str(tmp_path))) == sorted(g)
    d = sp.describe(dict(sp.DEFAULTS), 441, 441, 2.0, 4.0, rows)
    assert json.loads(json.dumps(d))["T"] == 441 and d["n_prices"] == 441


# ------------------------------------------------------------------------------------------------ the entry points
def test_args_structs_match_the_header():
    from th_rl_amd import _lib
    got, mine = _offsets(_lib.PriceProbsArgs, "thrl_price_probs_args", ["THRL_STAT_MAX_CELLS"])
    assert got == mine[:1] + [sp.MAX_PRICES] + mine[1:]
    got, mine = _offsets(_lib.SampledChainArgs, "thrl_sampled_chain_args",
                         ["THRL_SP_START_TUPLE", "THRL_SP_MAX_LDS", "THRL_STAT_MAX_ITERS", "THRL_TP_MAX_TUPLES"])
    assert got == mine[:1] + [_lib.SP_START_TUPLE, _lib.SP_MAX_LDS, _lib.STAT_MAX_ITERS, 4096] + mine[1:]
    assert "thrl_price_probs" in _lib.SYMBOLS and "thrl_sampled_chain" in _lib.SYMBOLS


SC_REQUIRED = ("dpolicy", "grp_first", "grp_perm", "reward", "scaled", "price", "iters", "change", "mass", "samp_reward",
               "samp_action", "samp_price", "agree")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    c = config or SHIP
    qt = {"agents": [dict(AG, actions=a.get("actions", 21)) for a in c["agents"]], "environment": c["environment"]}
    return _lib.cfg_from_config(qt, n_games, 0)[0]


def _set(a, kw):
    for k, v in kw.items():
        if k in ("kind", "eps", "prob", "nn_params"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


def sc_args(**kw):
    from th_rl_amd import _lib
    a = _lib.SampledChainArgs()
    a.n_games, a.n_tuples, a.n_prices, a.max_iters, a.tol = 64, 441, 441, 100, 1e-12
    a.kind[1], a.prob[1], a.eps[0] = 1, FAKE, 0.01
    for f in SC_REQUIRED:
        setattr(a, f, FAKE)
    return _set(a, kw)


def pb_args(**kw):
    from th_rl_amd import _lib
    a = _lib.PriceProbsArgs()
    a.n_games, a.n_prices, a.price = 64, 101, FAKE
    a.kind[1], a.nn_params[1], a.prob[1] = 1, FAKE, FAKE
    return _set(a, kw)


SC_BAD = [dict(n_games=0), dict(flags=2), dict(flags=-1), dict(reserved=1), dict(n_tuples=0), dict(n_tuples=440),
          dict(n_prices=0), dict(n_prices=442), dict(max_iters=0), dict(max_iters=65537), dict(tol=-1e-9),
          dict(tol=float("nan")), dict(eps=[-0.1]), dict(eps=[1.5]), dict(eps=[float("nan")]), dict(kind=[0, 4]),
          dict(kind=[-1, 0]), dict(kind=[0, 1], n_tuples=21 * 40, n_prices=21)]
PB_BAD = [dict(n_games=0), dict(n_games=65), dict(flags=1), dict(reserved=1), dict(n_prices=0), dict(n_prices=-1),
          dict(kind=[0, 4]), dict(kind=[0, 1], forty=True)]


def check_validation(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path of both entry points that the host can see; none touches a device."""
    cfg = _cfg()
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})       # a network has at most 32
    for bad in SC_BAD:
        c = forty if bad.get("n_tuples") == 21 * 40 else cfg
        assert lib.thrl_sampled_chain(ctypes.byref(c), ctypes.byref(sc_args(**bad)), None) == -1, bad
        assert lib.thrl_last_error()
    for bad in PB_BAD:
        bad = dict(bad)
        c = forty if bad.pop("forty", False) else cfg
        assert lib.thrl_price_probs(ctypes.byref(c), ctypes.byref(pb_args(**bad)), None) == -1, bad
    # a neural agent's epsilon is not read; a per-game array takes the place of the scalars
    assert lib.thrl_sampled_chain(ctypes.byref(cfg), ctypes.byref(sc_args(eps=[0.0, 7.0], iters=None)), None) == -2
    assert lib.thrl_sampled_chain(ctypes.byref(cfg), ctypes.byref(sc_args(eps=[7.0], eps_g=FAKE, iters=None)), None) == -2
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097, n_prices=1)):
        assert lib.thrl_sampled_chain(ctypes.byref(cfg), ctypes.byref(sc_args(**unsupported)), None) == -3, unsupported
    # the working set: refused from the shape alone, before any pointer is looked at
    for aq, rc in ((30, -2), (32, -3)):
        c = _cfg({"agents": [dict(AG, actions=aq), dict(AG, actions=32)], "environment": dict(ENV)})
        a = sc_args(n_tuples=aq * 32, n_prices=aq * 32, mass=None)
        assert lib.thrl_sampled_chain(ctypes.byref(c), ctypes.byref(a), None) == rc, aq
    assert b"bytes of LDS" in lib.thrl_last_error()
    for unsupported in (dict(kind=[3, 0]), dict(n_prices=4097)):
        assert lib.thrl_price_probs(ctypes.byref(cfg), ctypes.byref(pb_args(**unsupported)), None) == -3, unsupported
    assert lib.thrl_price_probs(ctypes.byref(cfg), ctypes.byref(pb_args(n_prices=4096, price=None)), None) == -2
    for null in SC_REQUIRED:
        assert lib.thrl_sampled_chain(ctypes.byref(cfg), ctypes.byref(sc_args(**{null: None})), None) == -2, null
    assert lib.thrl_sampled_chain(ctypes.byref(cfg), ctypes.byref(sc_args(prob=[None, None])), None) == -2
    assert b"prob[1]" in lib.thrl_last_error()
    assert lib.thrl_sampled_chain(ctypes.byref(cfg), ctypes.byref(sc_args(flags=1)), None) == -2
    assert b"start" in lib.thrl_last_error()
    assert lib.thrl_sampled_chain(ctypes.byref(cfg), None, None) == -2
    assert lib.thrl_sampled_chain(None, ctypes.byref(sc_args()), None) == -2
    for null in (dict(price=None), dict(prob=[None, None]), dict(nn_params=[None, None])):
        assert lib.thrl_price_probs(ctypes.byref(cfg), ctypes.byref(pb_args(**null)), None) == -2, null
    assert lib.thrl_price_probs(ctypes.byref(cfg), None, None) == -2
    assert lib.thrl_price_probs(None, ctypes.byref(pb_args()), None) == -2


def test_entry_points_validate_before_any_launch(lib):
    check_validation(lib)
