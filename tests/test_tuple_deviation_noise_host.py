"""Host side of the deviation test under demand noise in tuple form (thrl_tuple_deviation_noise,
th_rl_amd/tuple_analysis.py), no GPU: the two routes of the mirror (tests/tuple_deviation_noise_mirror.py) against each
other, hand answers, the merged QTable analysis (tests/deviation_noise_mirror.py) on an all-QTable config, that the random
inputs of the device tests are no degenerate input (the deviation changes play and the switch at L matters), option
parsing, the args struct against the header, the entry point's validation through the library loaded without a GPU, the
summary, the artefacts and the readers."""
import ctypes
import json
import os

import numpy as np
import pytest

import deviation_noise_mirror as DN
import stationary_mirror as S
import tuple_deviation_noise_mirror as TD
import tuple_stationary_mirror as SM
from test_tuple_equilibrium_noise_host import NINE, Q5, QQ, QR, R5, TRIO, _qtable_strategies, gammas, strategies
from test_tuple_stationary_host import AG, CAC, ENV, MIXED, WIDE, _cfg, _offsets
from th_rl_amd import deviation as dv
from th_rl_amd import stationary as sn
from th_rl_amd import tuple_analysis as ta
from th_rl_amd import tuple_stationary as ts

FINE = QR                                                                                              # J > 512 at 600
W21 = {"agents": [dict(Q5, actions=21, states=20), dict(R5, actions=21)], "environment": dict(ENV)}    # T = 441
BIG = {"agents": [dict(Q5, actions=64, states=20), dict(R5, actions=32)], "environment": dict(ENV)}    # T = 2048
# the inputs of the device tests: (config, resolution, games, seed, deviator, steps K, dev_len L).  The seeds are chosen
# on the mirror so that the conditions of test_device_inputs_are_not_degenerate hold.
DCASES = {"QR": (QR, 16, 70, 71, 0, 12, 1), "NINE": (NINE, 100, 9, 72, 1, 8, 2), "FINE": (FINE, 600, 8, 73, 1, 8, 1),
          "W21": (W21, 100, 6, 74, 1, 6, 1), "TRIO": (TRIO, 16, 21, 75, 2, 8, 2), "BIG": (BIG, 600, 4, 77, 0, 6, 1)}
_IN = {}


def inputs(name):
    """(config, tabs, tuple_policy, cell_policy, weights [G, T], deviator, K, L) of a device case, made once; the
    weights are random distributions."""
    if name not in _IN:
        config, res, G, seed, d, K, L = DCASES[name]
        tabs = ts.tables(config, res)
        tpol, cpol = strategies(tabs, G, seed)
        w = np.random.RandomState(seed + 1000).uniform(0.0, 1.0, (G, tabs["n_tuples"]))
        _IN[name] = (config, tabs, tpol, cpol, w / w.sum(axis=1, keepdims=True), d, K, L)
    return _IN[name]


_REF = {}


def reference(name):
    """The mirror's outputs of a device case at p = 0.05 and best response, computed once and not changed."""
    if name not in _REF:
        config, tabs, tpol, cpol, w, d, K, L = inputs(name)
        _REF[name] = TD.analyse(tabs, tpol, cpol, 0.05, w, deviator=d, steps=K, dev_len=L, gamma=gammas(config))
    return _REF[name]


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the mirror itself
@pytest.mark.parametrize("name", ["QR", "NINE", "TRIO"])
def test_the_two_routes_of_the_mirror_agree(name):
    """E_i(tau) by the recurrence in the stated order against the dense products m_0 P'^L P^(tau - L), within
    TD.dense_bound: (tau (T + J + 3) + T + 3) 2^-52 max|R| (derived there from the lengths of the sums: T products into
    nu, J adds into Nn, T into D, and T + 3 for E itself).  Nothing is added to the bound.  The observed share of the
    bound is printed: at most 0.05 on these inputs."""
    config, tabs, tpol, cpol, w, d, K, L = inputs(name)
    T, J = tabs["n_tuples"], tabs["n_cells"]
    G = min(4, tpol.shape[0])
    out = TD.analyse(tabs, tpol[:G], cpol[:G], 0.05, w[:G], deviator=d, steps=K, dev_len=L, gamma=gammas(config))
    worst = 0.0
    for g in range(G):
        Ed, rmax = TD.dense(tabs, tpol[:G], cpol[:G], 0.05, w[:G], g, deviator=d, steps=K, dev_len=L)
        for t in range(K):
            err = np.abs(out["reward_rows"][t, :, g] - Ed[t]).max()
            b = TD.dense_bound(t, T, J, rmax)
            worst = max(worst, err / b)
            assert err <= b, (g, t, err, b)
    print("%s: T %d, J %d, K %d, L %d: max |E - dense| / bound = %.4f" % (name, T, J, K, L, worst))
    assert worst <= 1.0


def test_hand_answers():
    tabs = ts.tables(QR, 16)
    T, J, N, G = tabs["n_tuples"], tabs["n_cells"], 2, 5
    tpol, cpol = strategies(tabs, G, 5)
    gam = gammas(QR)
    # the deviator's given strategy is constant and equal to dev_action: started on the tuples it plays, Dv changes
    # nothing that carries mass, so dev_share = 0, gain = 0 and the rows stay at base_reward.  From the stationary
    # distribution the rows move by no more than the stationary tolerance allows: one plain step moves the distribution by
    # at most 2 tol per entry (the lazy step moved it by tol), so after tau steps |E - base| <= 2 tau T tol max|R|
    tpol2, cpol2 = tpol.copy(), cpol.copy()
    tpol2[:, 0, :], cpol2[:, 0, :] = 3, 3
    st = SM.analyse(tabs, tpol2, cpol2, 0.05, tol=1e-13)
    assert (st["iters"] < 8192).all()
    out = TD.analyse(tabs, tpol2, cpol2, 0.05, st["pi"], deviator=0, steps=6, dev_len=2, dev_action=3, gamma=gam)
    plays3 = (np.arange(T) // 5) == 3
    assert (st["pi"][:, ~plays3] == 0.0).all()           # greedy play intends only tuples in which agent 0 plays 3
    assert (out["dev_share"] == 0.0).all() and np.array_equal(out["base_reward"], st["stat_reward"])
    rmax = np.abs(TD.expected_rewards(tabs, np.full(G, 0.05))).max()
    for t in range(6):
        assert np.abs(out["reward_rows"][t] - out["base_reward"]).max() <= 2 * max(t, 1) * T * 1e-13 * rmax
    assert np.abs(out["gain"]).max() <= 6 * 2 * 6 * T * 1e-13 * rmax
    # p = 1: m_1 does not depend on F (D is multiplied by q = 0)
    w = np.random.RandomState(2).dirichlet(np.ones(T), G)
    a = TD.analyse(tabs, tpol, cpol, 1.0, w, steps=2, gamma=gam)
    other = tpol.copy()
    other[:, :, :] = (other + 1) % 5
    b = TD.analyse(tabs, other, cpol, 1.0, w, steps=2, gamma=gam)
    assert np.array_equal(a["reward_rows"][1], b["reward_rows"][1]) and np.array_equal(a["dist_rows"][1], b["dist_rows"][1])
    assert not np.array_equal(TD.analyse(tabs, tpol, cpol, 0.05, w, steps=2, gamma=gam)["reward_rows"][1],
                              TD.analyse(tabs, other, cpol, 0.05, w, steps=2, gamma=gam)["reward_rows"][1])
    # K == L: no period after the deviation
    out = TD.analyse(tabs, tpol, cpol, 0.05, w, steps=3, dev_len=3, gamma=gam)
    assert (out["low"] == 0.0).all() and (out["low_step"] == -1).all() and np.array_equal(out["gain"], out["gain_dev"])
    # unit-mass weights: period 0 is a single tuple's R_i(Dv(t)), and dev_share says whether Dv moves it
    unit = np.zeros((G, T))
    at = np.array([0, 7, 12, 18, 24])
    unit[np.arange(G), at] = 1.0
    out = TD.analyse(tabs, tpol, cpol, 0.05, unit, steps=2, gamma=gam)
    R = TD.expected_rewards(tabs, np.full(G, 0.05))
    for g in range(G):
        assert np.array_equal(out["reward_rows"][0, :, g], R[:, g, out["Dv"][g, at[g]]])
        assert np.array_equal(out["base_reward"][:, g], R[:, g, at[g]])
        assert out["dev_share"][g] == float(out["Dv"][g, at[g]] != at[g])
    assert (out["dist_rows"][0] == 0.0).all() and np.abs(out["mass"] - 1.0).max() <= 1e-12
    # games that are not solved
    p = np.array([0.05, np.nan, 0.0, 1.5, 1.0])
    out = TD.analyse(tabs, tpol, cpol, p, w, steps=3, gamma=gam)
    for f in TD.FLOAT_FIELDS + TD.AGENT_FIELDS + TD.ROW_FIELDS:
        assert (np.asarray(out[f])[..., 1:4] == 0.0).all(), f
    assert (out["low_step"][1:4] == -1).all() and (out["ret_step"][1:4] == -1).all() and out["mass"][4] > 0.99


def test_all_qtable_game_against_the_qtable_analysis():
    """resolution = 0 on an all-QTable config whose tuple prices sit on no tie breakpoint: the cells are
    thrl_stationary's, and with the cell m_0 pushed forward to tuples the distribution over the tuple intended is the
    push-forward of the distribution over the cells at every period.  E_i, A_i, base_*, dev_share, gain, gain_dev and low
    agree within the rounding of the two routes: each is within its own dense bound of exact arithmetic
    (DN.dense_bound's tau (J + 2) 2^-52 max|R| for the cells, TD.dense_bound for the tuples), the push-forward adds J
    terms once ((J + 1) 2^-52), so |E - E'| <= b(tau) = DN.dense_bound + TD.dense_bound + (J + 1) 2^-52 max|R|; the
    differences from the baseline add b(0), the discounted sums add these up with weights <= 1.  Dist and ret_step are
    not compared: total variation on tuples is coarser than on cells."""
    tq, tt = sn.tables(QQ), ts.tables(QQ, 0)
    J, T = tq["n_cells"], tq["n_tuples"]
    det = np.asarray(tq["det_cell"])
    assert tq["n_intervals"] == J == tt["n_cells"] and ((det >= 0) & (det < J)).all()
    G, K, L = 3, 6, 2
    policy = S.policies(QQ, S.fresh_tables(QQ, G, 7))
    tpol, cpol = _qtable_strategies(QQ, tq, policy)
    mu0 = np.random.RandomState(3).dirichlet(np.ones(J), G)
    m0 = SM.grouped(SM.tuple_of(tt, cpol), mu0, T)
    for d, act in ((0, -1), (1, 4)):
        ref = DN.analyse(QQ, tq, policy, 0.05, mu0, deviator=d, steps=K, dev_len=L, dev_action=act)
        out = TD.analyse(tt, tpol, cpol, 0.05, m0, deviator=d, steps=K, dev_len=L, dev_action=act, gamma=gammas(QQ))
        rmax = np.abs(TD.expected_rewards(tt, np.full(G, 0.05))).max()
        amax = np.abs(tt["scaled"]).max()
        b = lambda t, x: DN.dense_bound(t, J, x) + TD.dense_bound(t, T, J, x) + (J + 1) * 2.0 ** -52 * x
        for t in range(K):
            assert np.abs(out["reward_rows"][t] - ref["reward_rows"][t]).max() <= b(t, rmax), (d, t)
            assert np.abs(out["action_rows"][t] - ref["action_rows"][t]).max() <= b(t, amax), (d, t)
        assert np.abs(out["base_reward"] - ref["base_reward"]).max() <= b(0, rmax)
        assert np.abs(out["base_action"] - ref["base_action"]).max() <= b(0, amax)
        assert np.abs(out["dev_share"] - ref["dev_share"]).max() <= b(0, 1.0)
        total = sum(b(t, rmax) + b(0, rmax) for t in range(K))
        assert np.abs(out["gain"] - ref["gain"]).max() <= total and np.abs(out["gain_dev"] - ref["gain_dev"]).max() <= total
        assert np.abs(out["low"] - ref["low"]).max() <= b(K - 1, rmax) + b(0, rmax)
        assert (ref["dev_share"] > 0).any()


@pytest.mark.parametrize("name", sorted(DCASES))
def test_device_inputs_are_not_degenerate(name):
    """What the device tests rely on, asserted on the mirror for every config and seed of theirs: the deviation changes
    play in at least half of the games (dev_share > 0.1), the response moves the deviator's expected reward off the
    baseline in at least half (max_tau |E_d(tau) - base_reward_d| > 1e-6), and the gain has both signs.  A kernel that
    ignored the deviation or the switch at L cannot pass on these inputs."""
    config, tabs, tpol, cpol, w, d, K, L = inputs(name)
    out = reference(name)
    G = tpol.shape[0]
    move = np.abs(out["reward_rows"][:, d, :] - out["base_reward"][d][None, :]).max(axis=0)
    print("%s: T %d, J %d, W %d: dev_share > 0.1 in %d of %d, moved in %d, gain > 0 in %d, < 0 in %d"
          % (name, tabs["n_tuples"], tabs["n_cells"], tabs["band_w"], (out["dev_share"] > 0.1).sum(), G, (move > 1e-6).sum(),
             (out["gain"] > 0).sum(), (out["gain"] < 0).sum()))
    assert 2 * (out["dev_share"] > 0.1).sum() >= G and 2 * (move > 1e-6).sum() >= G
    assert (out["gain"] > 0).any() and (out["gain"] < 0).any()
    # the switch at L matters: with the deviation held for one period more the next row differs
    if L < K:
        longer = TD.analyse(tabs, tpol, cpol, 0.05, w, deviator=d, steps=K, dev_len=L + 1, gamma=gammas(config))
        assert not np.array_equal(longer["reward_rows"][L], out["reward_rows"][L])
    if name == "NINE":
        assert tabs["n_tuples"] > 64 and tabs["n_tuples"] % 64
    if name == "FINE":
        assert tabs["n_cells"] > 512
    if name == "W21":
        assert tabs["n_tuples"] == 441
    if name == "BIG":
        assert 28 * tabs["n_tuples"] + 10 * tabs["n_cells"] + 512 * 6 + 6 > 64 * 1024


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_with_noise():
    noisy = dict(MIXED, environment=dict(ENV, noise_prob=0.05))
    base = dict(steps=32, dev_len=1, action="best_response", horizon=None, agents=[0, 1])
    assert ta.parse_deviation_options(True, MIXED) == base                  # pinned: nothing appears unless given
    assert ta.parse_deviation_options({"noise": None}, MIXED) == base and ta.parse_deviation_options({"noise": False}, MIXED) == base
    assert ta.DEV_NOISE_DEFAULTS == dict(noise_prob=None, ret_tol=1e-6, tol=1e-12, max_iters=8192, resolution=1024)
    assert ta.parse_deviation_options({"noise": True}, noisy) == dict(base, noise=ta.DEV_NOISE_DEFAULTS)
    got = ta.parse_deviation_options({"agents": [1], "steps": 8, "noise": {"noise_prob": 0.2, "ret_tol": 0, "tol": 1e-9,
                                                                           "max_iters": 100, "resolution": 32}}, MIXED)
    assert got == dict(base, agents=[1], steps=8, noise=dict(noise_prob=0.2, ret_tol=0.0, tol=1e-9, max_iters=100, resolution=32))
    swept = dict(MIXED, training={"sweep": {"noise_prob": [0.1]}})
    assert ta.parse_deviation_options({"noise": True}, swept)["noise"]["noise_prob"] is None
    with pytest.raises(ValueError, match=r"training\.greedy_deviation\.noise: the environment has noise_prob = 0: give"):
        ta.parse_deviation_options({"noise": True}, MIXED)
    for bad in ({"tables": "final"}, {"noise_prob": 0}, {"noise_prob": 1.5}, {"noise_prob": "x"}, {"noise_prob": True},
                {"ret_tol": -1}, {"ret_tol": "a"}, {"ret_tol": True}, {"ret_tol": float("nan")}, {"tol": -1}, {"tol": True},
                {"max_iters": 0}, {"max_iters": 65537}, {"max_iters": 1.5}, {"max_iters": True}, {"resolution": -1},
                {"resolution": 1.5}, {"resolution": True}, {"resolution": 4096}, {"eval_tol": 1e-9}, 5, "yes"):
        with pytest.raises(ValueError, match="greedy_deviation"):
            ta.parse_deviation_options({"noise": bad}, noisy)
    with pytest.raises(ValueError, match="continuous"):
        ta.parse_deviation_options({"noise": True}, dict(CAC, environment=dict(ENV, noise_prob=0.05)))
    with pytest.raises(ValueError, match="4096"):
        ta.parse_deviation_options({"noise": True}, dict(WIDE, environment=dict(ENV, noise_prob=0.05)))
    # train_one refuses before it builds a batch (no GPU is touched)
    from th_rl_amd import trainer
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "c.json"), "w").write(json.dumps(dict(MIXED, training={"epochs": 1, "n_games": 4,
                                                                                      "greedy_deviation": {"noise": True}})))
        with pytest.raises(ValueError, match="noise_prob = 0"):
            trainer.train_one(os.path.join(d, "run"), os.path.join(d, "c.json"))


# ------------------------------------------------------------------------------------------------ the entry point
FAKE = 4096                           # never dereferenced: validation fails before any launch
TABLES = ("tuple_policy", "cell_policy", "reward", "scaled", "band_lo", "band", "noise_reward")
OUTPUTS = ("base_reward", "base_action", "dev_share", "gain", "gain_dev", "low", "low_step", "ret_step", "dist", "mass")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.TupleDeviationNoiseArgs()
    a.n_games, a.n_tuples, a.n_cells, a.band_w = 64, 441, 101, 31
    a.deviator, a.dev_len, a.n_steps, a.dev_action = 0, 1, 32, -1
    a.ret_tol, a.noise_prob = 1e-6, 0.05
    for f in TABLES + ("weights",) + OUTPUTS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k == "kind":
            for i, x in enumerate(v):
                a.kind[i] = x
        else:
            setattr(a, k, v)
    return a


BAD = [(dict(n_games=0), "n_games=0 must be >= 1"), (dict(n_games=-3), "n_games=-3"), (dict(flags=1), "unknown flags 0x1"),
       (dict(reserved=1), "reserved=1 must be 0"), (dict(kind=[0, 4]), "agent 1: kind=4"), (dict(kind=[-1, 0]), "agent 0: kind=-1"),
       (dict(n_tuples=0), "n_tuples=0 must be >= 1"), (dict(n_tuples=440), "is not the product"),
       (dict(deviator=2), "deviator=2 out of [0,2)"), (dict(deviator=-1), "deviator=-1"), (dict(dev_len=0), "dev_len=0 must be >= 1"),
       (dict(n_steps=0), "n_steps=0 out of [dev_len=1"), (dict(dev_len=5, n_steps=4), "n_steps=4 out of [dev_len=5"),
       (dict(n_steps=(1 << 20) + 1), "n_steps=1048577"), (dict(dev_action=21), "dev_action=21"), (dict(dev_action=-2), "dev_action=-2"),
       (dict(row_begin=-1), "rows [-1"), (dict(row_begin=30, row_count=3), "rows [30, 30 + 3) outside [0, n_steps=32)"),
       (dict(row_count=-1), "rows ["), (dict(n_cells=0), "n_cells=0 and band_w=31"), (dict(band_w=0), "band_w=0 must be"),
       (dict(ret_tol=-1e-9), "ret_tol=-1e-09 must be >= 0"), (dict(ret_tol=float("nan")), "ret_tol=nan"),
       (dict(noise_prob=0.0), "noise_prob=0 out of (0, 1]"), (dict(noise_prob=1.5), "noise_prob=1.5"),
       (dict(noise_prob=float("nan")), "noise_prob=nan"), (dict(noise_prob=-0.05), "noise_prob=-0.05")]


@pytest.mark.parametrize("bad,words", BAD)
def test_bad_arguments_are_bad_config(lib, bad, words):
    assert lib.thrl_tuple_deviation_noise(ctypes.byref(_cfg()), ctypes.byref(_args(**bad)), None) == -1
    assert words.encode() in lib.thrl_last_error(), lib.thrl_last_error()


@pytest.mark.parametrize("null", ("cfg", "args") + TABLES + ("weights",) + OUTPUTS)
def test_missing_pointers_are_null(lib, null):
    kw = {} if null in ("cfg", "args") else {null: None}
    c = None if null == "cfg" else ctypes.byref(_cfg())
    a = None if null == "args" else ctypes.byref(_args(**kw))
    assert lib.thrl_tuple_deviation_noise(c, a, None) == -2
    if null not in ("cfg", "args"):
        assert null.encode() in lib.thrl_last_error() and b"is NULL" in lib.thrl_last_error()


def test_order_of_the_checks_limits_and_working_set(lib):
    from th_rl_amd import _lib
    call = lambda a, c=None: lib.thrl_tuple_deviation_noise(ctypes.byref(c or _cfg()), ctypes.byref(a), None)
    err = lambda: lib.thrl_last_error().decode()
    # thrl_tuple_stationary's order, then the deviation and its rows as thrl_deviation_noise orders them: of two bad
    # arguments the earlier check speaks
    order = [dict(n_games=0), dict(flags=2), dict(reserved=3), dict(kind=[0, 5]), dict(n_tuples=7), dict(deviator=9),
             dict(dev_action=99), dict(row_count=99), dict(n_cells=0), dict(ret_tol=-1.0), dict(noise_prob=2.0),
             dict(n_cells=4097), dict(band=None), dict(weights=None), dict(mass=None)]
    words = ["n_games=0", "unknown flags 0x2", "reserved=3", "kind=5", "n_tuples=7", "deviator=9", "dev_action=99", "rows [",
             "n_cells=0", "ret_tol=-1", "noise_prob=2", "n_cells=4097", "noise_reward is NULL", "weights is NULL", "mass is NULL"]
    for i in range(len(order) - 1):
        if "n_cells" in order[i] and "n_cells" in order[i + 1]:
            continue
        rc = call(_args(**dict(order[i + 1], **order[i])))
        assert rc < 0 and words[i] in err(), (order[i], order[i + 1], err())
    # a per-game noise array takes the place of the scalar, a device gamma array that of cfg.gamma; the rows are optional
    assert call(_args(noise_prob=0.0, noise_prob_g=FAKE, mass=None)) == -2 and "mass" in err()
    assert call(_args(sweep_gamma=FAKE, reward_rows=FAKE, action_rows=FAKE, dist_rows=FAKE, row_count=32, gain=None)) == -2
    for unsupported, w in ((dict(kind=[0, 3]), "CAC"), (dict(n_tuples=4097), "n_tuples=4097, at most 4096"),
                           (dict(n_cells=4097), "thrl_tuple_deviation_noise: n_cells=4097, at most 4096")):
        assert call(_args(**unsupported)) == _lib.ERR_UNSUPPORTED and w in err(), unsupported
    wide = _cfg({"agents": [dict(AG, actions=129), dict(AG, actions=32)], "environment": dict(ENV)})
    assert call(_args(n_tuples=4128), wide) == _lib.ERR_UNSUPPORTED
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})
    assert call(_args(kind=[0, 1], n_tuples=21 * 40), forty) == -1 and "neural agent 1: actions=40" in err()
    # the working set, 28 T + 10 J + 512 (2 N + 2) + 6 rounded up to 16 bytes against 160 KB.  Two agents: the limits on
    # T and J themselves fit (158,736 bytes), the next refusal is a missing pointer
    need = lambda T, J, N: (28 * T + 10 * J + 512 * (2 * N + 2) + 6 + 15) // 16 * 16
    assert need(4096, 4096, 2) == 158736 <= _lib.TDN_MAX_LDS == 160 * 1024
    big = _cfg({"agents": [dict(AG, actions=128), dict(AG, actions=32)], "environment": dict(ENV)})
    assert call(_args(n_tuples=4096, n_cells=4096, mass=None), big) == -2 and "mass" in err()
    # seven agents (4^5 * 2^2 = 4096 tuples): the last J that fits, and one more
    acts = [4, 4, 4, 4, 4, 2, 2]
    seven = _cfg({"agents": [dict(AG, actions=a, states=4) for a in acts], "environment": dict(ENV, nplayers=7)})
    jmax = (_lib.TDN_MAX_LDS - 28 * 4096 - 512 * 16 - 6) // 10
    assert need(4096, jmax, 7) <= _lib.TDN_MAX_LDS < need(4096, jmax + 1, 7) and jmax == 4095
    assert call(_args(n_tuples=4096, n_cells=jmax, mass=None), seven) == -2 and "mass" in err()
    assert call(_args(n_tuples=4096, n_cells=jmax + 1, mass=None), seven) == _lib.ERR_UNSUPPORTED
    assert "thrl_tuple_deviation_noise: %d bytes of LDS per game (N=7, n_cells=%d)" % (need(4096, jmax + 1, 7), jmax + 1) in err()


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    got, mine = _offsets(_lib.TupleDeviationNoiseArgs, "thrl_tuple_deviation_noise_args",
                         ["THRL_TDN_MAX_LDS", "THRL_STAT_MAX_CELLS", "THRL_DEV_MAX_STEPS", "THRL_TP_MAX_TUPLES", "THRL_ABI_VERSION"])
    assert got == mine[:1] + [_lib.TDN_MAX_LDS, _lib.STAT_MAX_CELLS, _lib.DEV_MAX_STEPS, 4096, 4] + mine[1:]
    assert "thrl_tuple_deviation_noise" in _lib.SYMBOLS and _lib.ABI_VERSION == 4 and len(_lib.SYMBOLS) == 55


# ------------------------------------------------------------------------------------------------ summary, readers
def _games(G=10, seed=4):
    rs = np.random.RandomState(seed)
    g = dict(dev_share=rs.uniform(0, 1, G), gain=rs.uniform(-3, 3, G), gain_dev=rs.uniform(0, 3, G), low=rs.uniform(-2, 0, G),
             dist=rs.uniform(0, 1e-3, G), mass=np.ones(G), low_step=rs.randint(1, 9, G).astype(np.int32),
             ret_step=rs.randint(-1, 9, G).astype(np.int32), base_reward=rs.uniform(20, 25, (2, G)),
             base_action=rs.uniform(0.2, 0.4, (2, G)), noise_prob=np.full(G, 0.05),
             stat_iters=rs.randint(100, 900, G).astype(np.int32), n_switch=rs.randint(0, 7, G).astype(np.int32),
             unresolved=rs.uniform(0, 0.01, G))
    g["noise_prob"][2] = np.nan
    return g


def test_summary_artefacts_and_readers(tmp_path):
    from th_rl_amd import utils
    G = 10
    games = {0: _games(G, 4), 1: _games(G, 5)}
    ids = np.array([0] * 5 + [1] * 5)
    rows = ta.summarize_deviation_noise(games, ids, 2, [0, 1])
    base = dv.summarize_noise(games, ids, 2, [0, 1])
    assert [(r["group"], r["deviator"]) for r in rows] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for r, b in zip(rows, base):
        assert {k: r[k] for k in b} == b and set(r) - set(b) == {"n_switch_max", "unresolved_mean"}
    assert rows[0]["solved"] == 4 and rows[0]["games"] == 5
    assert rows[0]["n_switch_max"] == int(games[0]["n_switch"][:5].max())
    assert rows[3]["unresolved_mean"] == float(games[1]["unresolved"][5:].mean())
    d = tmp_path / "run"
    d.mkdir()
    for k in (0, 1):
        ta.save_deviation_noise_games(str(d), k, games[k])
    assert sorted(f.name for f in d.iterdir()) == ["gdevn0_base.npy", "gdevn0_games.npy", "gdevn0_steps.npy", "gdevn1_base.npy",
                                                   "gdevn1_games.npy", "gdevn1_steps.npy", "gdevn_prob.npy", "gdevn_stat.npy",
                                                   "gdevn_unresolved.npy"]
    assert np.load(d / "gdevn0_games.npy").shape == (6, G) and np.load(d / "gdevn1_steps.npy").dtype == np.int32
    assert np.load(d / "gdevn0_base.npy").shape == (2, 2, G) and np.load(d / "gdevn_stat.npy").shape == (2, G)
    back = ta.load_deviation_noise_games(str(d), 0)
    shared = ("noise_prob", "stat_iters", "n_switch", "unresolved")          # written by the last deviator saved
    assert set(back) == set(games[0])
    for f in games[0]:
        assert np.array_equal(back[f], games[1 if f in shared else 0][f], equal_nan=True), f
    noisy = dict(MIXED, environment=dict(ENV, noise_prob=0.05))
    opt = ta.parse_deviation_options({"noise": True}, noisy)
    (d / "config.json").write_text(json.dumps(dict(noisy, training={"n_games": G})))
    ta.an.save_json(str(d / "greedy_deviation_noise.json"),
                    {"options": opt, "n_cells": 26, "T": 25, "quantiles": [0.25, 0.5, 0.75], "summary": rows})
    df = utils.greedy_deviation_noise_summary(str(d))
    assert len(df) == 4 and df["n_cells"].tolist() == [26] * 4 and df["T"].tolist() == [25] * 4
    assert {"n_switch_max", "unresolved_mean", "gain_q50", "dist_mean", "solved", "deviates"} <= set(df.columns)
    a = utils.greedy_deviation_noise_games(str(d), 1)
    assert a.index.tolist() == list(range(G)) and a["gain"].tolist() == games[1]["gain"].tolist()
    assert a["solved"].tolist() == [True, True, False] + [True] * 7 and a["n_switch"].tolist() == games[1]["n_switch"].tolist()
    assert {"base_reward_0", "base_action_1", "stat_iters", "unresolved", "low_step", "ret_step"} <= set(a.columns)
    assert utils.greedy_deviation_noise_games(str(d))["low"].tolist() == games[0]["low"].tolist()
    with pytest.raises(KeyError, match="deviator 2 was not analysed"):
        utils.greedy_deviation_noise_games(str(d), 2)
    with pytest.raises(KeyError, match=r"\(gdevn_prob.npy\) under .* \(training\.greedy_deviation\.noise\)"):
        utils.greedy_deviation_noise_games(str(tmp_path / "none"), 0)
    with pytest.raises(KeyError, match=r"\(greedy_deviation_noise.json\)"):
        utils.greedy_deviation_noise_summary(str(tmp_path / "none"))


def test_batch_method_is_shared_and_documented():
    from th_rl_amd import analysis
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    fn = analysis.AnalysisMethods.greedy_deviation_noise
    assert GameBatch.greedy_deviation_noise is fn and MixedGameBatch.greedy_deviation_noise is fn
    assert "thrl_tuple_deviation_noise" in fn.__doc__ and len(analysis.REGISTRY) == 12
    rec = analysis.record("greedy_deviation")
    assert rec == analysis._a("greedy_deviation", "tuple_analysis", "greedy_deviation", "parse_deviation_options",
                              "write_deviation", tuple_policy="extract", rows=True)
