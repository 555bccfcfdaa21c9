"""Host side of the deviation test under demand noise (thrl_deviation_noise, th_rl_amd/deviation.py), no GPU: the args
struct against the header, the entry point's validation through the library, option parsing, the known answers through
hand-written policies on the mirror, the mirror against its dense route, the summary, the merge and the readers."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import deviation_noise_mirror as DN
import equilibrium_mirror as E
import stationary_mirror as S
from th_rl_amd import deviation as dv
from th_rl_amd import stationary as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG = dict(name="QTable", gamma=0.95, actions=21, states=100, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
NOISY = dict(CFG, environment=dict(ENV, noise_prob=0.05))
SMALL = {"agents": [dict(AG, states=20), dict(AG, states=20, gamma=0.9)], "environment": dict(ENV)}
MIXED = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
         "environment": dict(ENV)}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the entry point
TABLES = ("cell_rows", "det_cell", "band_lo", "band", "noise_reward")
OUTPUTS = ("base_reward", "base_action", "dev_share", "gain", "gain_dev", "low", "low_step", "ret_step", "dist", "mass")


def _args(**kw):
    from th_rl_amd import _lib
    a = _lib.DeviationNoiseArgs()
    a.n_games, a.n_cells, a.band_w, a.noise_prob, a.ret_tol = 64, 101, 31, 0.05, 1e-6
    a.deviator, a.dev_len, a.n_steps, a.dev_action = 0, 1, 32, -1
    fake = 4096                       # never dereferenced: validation fails before any launch
    for f in ("policy", "weights") + TABLES + OUTPUTS:
        setattr(a, f, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_games=0), dict(n_games=65), dict(flags=2), dict(flags=-1), dict(deviator=-1),
                                 dict(deviator=2), dict(dev_len=0), dict(n_steps=0), dict(dev_len=33),
                                 dict(n_steps=(1 << 20) + 1), dict(dev_action=-2), dict(dev_action=21),
                                 dict(row_begin=-1), dict(row_count=-1), dict(row_count=33),
                                 dict(row_begin=30, row_count=3), dict(n_cells=0), dict(band_w=0), dict(ret_tol=-1e-9),
                                 dict(ret_tol=float("nan")), dict(noise_prob=0.0), dict(noise_prob=1.5),
                                 dict(noise_prob=float("nan")), dict(noise_prob=-0.05)])
def test_bad_arguments_are_bad_config(lib, bad):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    assert lib.thrl_deviation_noise(ctypes.byref(cfg), ctypes.c_void_p(4096), ctypes.byref(_args(**bad)), None) == -1
    assert lib.thrl_last_error()


@pytest.mark.parametrize("null", ("q", "args", "policy", "weights") + TABLES + OUTPUTS)
def test_missing_pointers_are_null(lib, null):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    q = None if null == "q" else ctypes.c_void_p(4096)
    kw = {} if null in ("q", "args") else {null: None}
    a = None if null == "args" else ctypes.byref(_args(**kw))
    assert lib.thrl_deviation_noise(ctypes.byref(cfg), q, a, None) == -2
    if null not in ("q", "args"):
        assert null.encode() in lib.thrl_last_error()


def test_flags_limits_and_n_tuples(lib):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(CFG, 64, 0)
    call = lambda a, q=None: lib.thrl_deviation_noise(ctypes.byref(cfg), q, ctypes.byref(a), None)
    t = ctypes.c_int32(-1)
    assert call(_args(n_tuples=ctypes.pointer(t))) == -2 and b"q is NULL" in lib.thrl_last_error() and t.value == 441
    given = _args(flags=_lib.STAT_POLICY_GIVEN, gain=None)
    assert call(given) == -2 and b"q is NULL" not in lib.thrl_last_error() and b"gain" in lib.thrl_last_error()
    # the rows are optional, and a row range inside [0, n_steps) is accepted: the call gets as far as q
    assert call(_args(row_begin=29, row_count=3)) == -2 and b"q is NULL" in lib.thrl_last_error()
    # K == L is allowed
    assert call(_args(dev_len=32)) == -2 and b"q is NULL" in lib.thrl_last_error()
    # a per-game array replaces the scalar, which is then not read
    assert call(_args(noise_prob=0.0, noise_prob_g=4096)) == -2 and b"q is NULL" in lib.thrl_last_error()
    # the limits: cells, and LDS (20 J + 512 (2 N + 2) + 16 bytes against 64 KB: with N = 2, J = 3,122 fits)
    q = ctypes.c_void_p(4096)
    assert call(_args(n_cells=4097), q) == _lib.ERR_UNSUPPORTED and b"4096" in lib.thrl_last_error()
    assert call(_args(n_cells=3123), q) == _lib.ERR_UNSUPPORTED and b"LDS" in lib.thrl_last_error()
    assert b"thrl_deviation_noise" in lib.thrl_last_error()
    assert 20 * 3122 + 3088 <= 65536 < 20 * 3123 + 3088 and 20 * 3001 + 3088 == 63108
    assert call(_args(n_cells=3122, gain=None), q) == -2 and b"gain" in lib.thrl_last_error()
    wide = {"agents": [dict(AG, actions=65), dict(AG, actions=64)], "environment": dict(ENV)}       # 4,160 tuples
    wcfg, _ = _lib.cfg_from_config(wide, 64, 0)
    assert lib.thrl_deviation_noise(ctypes.byref(wcfg), q, ctypes.byref(_args()), None) == _lib.ERR_UNSUPPORTED


def test_args_struct_and_limits_match_header():
    from th_rl_amd import _lib
    fields = [f for f, _ in _lib.DeviationNoiseArgs._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "thrl.h"\nint main(){printf("%zu %d %d %d %d"'
           + "".join(' " %zu"' for _ in fields) + ',sizeof(thrl_deviation_noise_args),THRL_STAT_POLICY_GIVEN,'
           'THRL_STAT_MAX_CELLS,THRL_DEV_MAX_STEPS,THRL_ABI_VERSION'
           + "".join(",offsetof(thrl_deviation_noise_args,%s)" % f for f in fields) + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    want = [ctypes.sizeof(_lib.DeviationNoiseArgs), _lib.STAT_POLICY_GIVEN, _lib.STAT_MAX_CELLS, _lib.DEV_MAX_STEPS, 4]
    assert got == want + [getattr(_lib.DeviationNoiseArgs, f).offset for f in fields]
    assert "thrl_deviation_noise" in _lib.SYMBOLS and _lib.ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------ options
def test_parse_options_with_noise():
    old = [True, {}, {"agents": [1], "steps": 8, "dev_len": 2, "action": 3, "horizon": 50, "tables": "converged"}]
    want = [dict(agents=[0, 1], steps=32, dev_len=1, action="best_response", horizon=None)] * 2 \
        + [dict(agents=[1], steps=8, dev_len=2, action=3, horizon=50, tables="converged")]
    for o, w in zip(old, want):         # every option dict valid before parses to what it did
        assert dv.parse_options(o, CFG) == w and dv.parse_options(o, NOISY) == w
    assert dv.parse_options(True, NOISY) == dv.parse_options({}, NOISY) and "noise" not in dv.parse_options(True, NOISY)
    assert dv.parse_options({"noise": None}, CFG) == want[0] and dv.parse_options({"noise": False}, CFG) == want[0]
    assert dv.NOISE_DEFAULTS == dict(noise_prob=None, ret_tol=1e-6, tol=1e-12, max_iters=8192)
    assert dv.parse_options({"noise": True}, NOISY) == dict(want[0], noise=dv.NOISE_DEFAULTS)
    assert dv.parse_options({"noise": True}, NOISY) == dv.parse_options({"noise": {}}, NOISY)
    got = dv.parse_options({"agents": [1], "noise": {"noise_prob": 0.2, "ret_tol": 0, "tol": 1e-9, "max_iters": 100}}, CFG)
    assert got == dict(want[0], agents=[1], noise=dict(noise_prob=0.2, ret_tol=0.0, tol=1e-9, max_iters=100))
    swept = dict(CFG, training={"sweep": {"noise_prob": [0.1]}})
    assert dv.parse_options({"noise": True}, swept)["noise"]["noise_prob"] is None
    # the refusal on a noise-free run, with stationary's wording
    with pytest.raises(ValueError, match="the environment has noise_prob = 0: give the noise_prob to analyse"):
        dv.parse_options({"noise": True}, CFG)
    for bad in ({"resolution": 8}, {"eval_tol": 1e-9}, {"noise_prob": 0}, {"noise_prob": 1.5}, {"noise_prob": "x"},
                {"noise_prob": True}, {"ret_tol": -1}, {"ret_tol": "a"}, {"ret_tol": True}, {"ret_tol": float("nan")},
                {"tol": -1}, {"tol": True}, {"max_iters": 0}, {"max_iters": 65537}, {"max_iters": 1.5},
                {"max_iters": True}, 5, "yes"):
        with pytest.raises(ValueError):
            dv.parse_options({"noise": bad}, NOISY)
    with pytest.raises(ValueError, match="follow-up"):
        dv.parse_options({"noise": True}, MIXED)
    # train_one refuses before it builds a batch (no GPU is touched)
    from th_rl_amd import trainer
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "c.json"), "w").write(json.dumps(dict(CFG, training={"epochs": 1, "n_games": 4,
                                                                                    "deviation": {"noise": True}})))
        with pytest.raises(ValueError, match="noise_prob = 0"):
            trainer.train_one(os.path.join(d, "run"), os.path.join(d, "c.json"))


# ------------------------------------------------------------------------------------------------ known answers
def _constant(config, a0, a1):
    return S.policies(config, E.strategy_tables(config, [a0, a1]))


def test_known_answers_constant_policies_fixed_action():
    """(a) Every agent plays one action in every cell, so every row of P is the row of t* and every row of P' the row
    of t'.  With m_0 = that row of P: m_1 is the row of t' (times the mass), m_2 = m_0, ret_step = 2 when the rows
    differ, and gain = R_d(t') - R_d(t*).

    Bound.  With mass <= 1 + J u a sum E(tau) carries at most (tau + 1) (J + 2) 2^-52 max|R| of rounding (tau steps and
    its own J products, as DN.dense_bound counts them) and the baseline (J + 2) 2^-52 max|R|; the gain adds K such
    differences with weights <= 1: (K + 2)^2 (J + 2) 2^-52 max|R| covers their sum."""
    tabs, pl = sn.tables(SMALL), E.plan(SMALL)
    J, K, p = tabs["n_cells"], 6, 0.05
    star, rival = 5, 12
    pol = _constant(SMALL, star, rival)
    tup = S.cell_tuples(SMALL, pol, tabs, 1)
    assert (tup == star * 21 + rival).all()
    m0 = S.chain(tabs, tup[0], p)[0][None, :]
    Rd = 0.95 * pl["rew"][0].reshape(21, 21)[:, rival] + 0.05 * tabs["noise_reward"][0].reshape(21, 21)[:, rival]
    rmax = float(np.abs(DN.expected_rewards(SMALL, tabs, np.array([p]))).max())
    bound = (K + 2) ** 2 * (J + 2) * 2.0 ** -52 * rmax
    for dev in (17, 0, star):
        out = DN.analyse(SMALL, tabs, pol, p, m0, deviator=0, steps=K, dev_len=1, dev_action=dev)
        assert (out["tupd"] == dev * 21 + rival).all()
        row_dev = S.chain(tabs, out["tupd"][0], p)[0]
        assert out["dev_share"][0] == (S.ordered_sum(m0)[0] if dev != star else 0.0)
        assert abs(out["mass"][0] - 1.0) <= bound / rmax and abs(out["gain"][0] - (Rd[dev] - Rd[star])) <= bound
        assert abs(out["base_reward"][0, 0] - Rd[star]) <= bound
        if dev != star:
            assert abs(out["dev_share"][0] - out["mass"][0]) <= bound / rmax
            differ = 0.5 * np.abs(row_dev - m0[0]).sum()
            assert differ > 1e-3                                   # the two rows differ: play leaves and comes back
            assert abs(out["dist_rows"][1, 0] - differ) <= bound / rmax and out["dist_rows"][0, 0] == 0.0
            assert out["ret_step"][0] == 2 and out["dist"][0] <= bound / rmax
            assert abs(out["gain_dev"][0] - (Rd[dev] - Rd[star])) <= bound
            # the aftermath is nothing: from period 1 on everyone is greedy on a chain whose rows are all equal
            assert np.abs(out["reward_rows"][1:, 0, 0] - Rd[star]).max() <= bound
            assert abs(out["low"][0]) <= bound and 1 <= out["low_step"][0] < K
        else:
            assert out["gain_dev"][0] == 0.0 and abs(out["gain_dev"][0]) <= bound
            assert out["ret_step"][0] == 1 and (out["dist_rows"][:, 0] <= bound / rmax).all()
    # K == L: no period after the deviation
    out = DN.analyse(SMALL, tabs, pol, p, m0, deviator=0, steps=2, dev_len=2, dev_action=17)
    assert out["low"][0] == 0.0 and out["low_step"][0] == -1 and out["gain"][0] == out["gain_dev"][0]
    assert out["ret_step"][0] == -1                                # D(2) is the row of t' against the row of t*


def test_known_answers_best_response_against_constant_rival():
    """(b) dev_action = -1: t' is the brute-force argmax of R_d against the rival's one action, for either deviator."""
    tabs, pl = sn.tables(SMALL), E.plan(SMALL)
    p = 0.05
    for d, own, rival in ((0, 3, 12), (0, 2, 0), (1, 7, 15)):
        acts = [own, rival] if d == 0 else [rival, own]
        pol = _constant(SMALL, *acts)
        m0 = np.tile(tabs["cell_w"], (1, 1))
        grid = (1.0 - p) * pl["rew"][d].reshape(21, 21) + p * tabs["noise_reward"][d].reshape(21, 21)
        Rv = grid[:, rival] if d == 0 else grid[rival, :]
        best = 0
        for a in range(1, 21):
            if Rv[a] > Rv[best]:
                best = a
        out = DN.analyse(SMALL, tabs, pol, p, m0, deviator=d, steps=4, dev_len=1)
        t_best = best * 21 + rival if d == 0 else rival * 21 + best
        assert (out["tupd"] == t_best).all() and best != own
        assert out["gain_dev"][0] > 0                              # the best response earns more in its own period
    # bad noise probabilities: zeros and -1, the neighbours untouched
    pol = S.policies(SMALL, S.fresh_tables(SMALL, 4, 2))
    w = np.tile(tabs["cell_w"], (4, 1))
    out = DN.analyse(SMALL, tabs, pol, np.array([0.05, 0.0, np.nan, 0.05]), w, steps=4)
    ref = DN.analyse(SMALL, tabs, pol, 0.05, w, steps=4)
    for f in DN.FLOAT_FIELDS + DN.INT_FIELDS + DN.AGENT_FIELDS + DN.ROW_FIELDS:
        assert (out[f][..., 1:3] == (-1 if f in DN.INT_FIELDS else 0)).all(), f
        assert np.array_equal(out[f][..., [0, 3]], ref[f][..., [0, 3]]), f


@pytest.mark.parametrize("dev_len,action", [(1, -1), (3, 4)])
def test_mirror_against_dense_route(dev_len, action):
    """The ordered recurrence against numpy's dense products on the headline grid, from the stationary distribution."""
    tabs = sn.tables(CFG)
    G, K, J = 3, 12, tabs["n_cells"]
    pol = S.policies(CFG, S.fresh_tables(CFG, G, 3))
    st = S.iterate(CFG, tabs, pol, 0.05)
    out = DN.analyse(CFG, tabs, pol, 0.05, st["pi"], steps=K, dev_len=dev_len, dev_action=action)
    assert np.array_equal(out["base_reward"], st["stat_reward"]) and np.array_equal(out["base_action"], st["stat_action"])
    assert (out["dist_rows"][0] == 0.0).all()
    worst = 0.0
    for g in range(G):
        Ed, rmax = DN.dense(CFG, tabs, pol, 0.05, st["pi"], g, steps=K, dev_len=dev_len, dev_action=action)
        for tau in range(K):
            err = np.abs(Ed[tau] - out["reward_rows"][tau, :, g]).max()
            worst = max(worst, err / DN.dense_bound(tau, J, rmax))
            assert err <= DN.dense_bound(tau, J, rmax), (g, tau, err)
    print("max |E - dense| / bound = %.3f" % worst)


# ------------------------------------------------------------------------------------------------ summary, shards
def _games(G=10, seed=4):
    rs = np.random.RandomState(seed)
    g = dict(base_reward=rs.uniform(10, 12, (2, G)), base_action=rs.uniform(0.2, 0.4, (2, G)),
             dev_share=rs.uniform(0, 1, G), gain=rs.uniform(-2, 2, G), gain_dev=rs.uniform(0, 1, G),
             low=rs.uniform(-1, 0, G), dist=rs.uniform(0, 0.1, G), mass=np.ones(G),
             low_step=rs.randint(1, 32, G).astype(np.int32), ret_step=rs.randint(-1, 32, G).astype(np.int32),
             noise_prob=np.full(G, 0.05), stat_iters=rs.randint(50, 900, G).astype(np.int32))
    g["dev_share"][[0, 6]] = 0.0
    g["ret_step"][[1, 2]] = -1
    g["ret_step"][0] = 1
    g["noise_prob"][3] = 0.0                    # not solved
    for f in DN.FLOAT_FIELDS:
        g[f][3] = 0.0
    g["low_step"][3] = g["ret_step"][3] = -1
    return g


def test_summary_arithmetic():
    g0, g1 = _games(), _games(seed=5)
    ids = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1])
    assert dv.solved_noise(g0).tolist() == [True] * 3 + [False] + [True] * 6
    rows = dv.summarize_noise({0: g0, 1: g1}, ids, 3, [0, 1])
    assert [(r["group"], r["deviator"]) for r in rows] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    r = rows[0]
    sel = [0, 1, 2, 4]
    assert r["games"] == 5 and r["solved"] == 4 and r["deviates"] == 3 / 4
    assert r["dev_share_mean"] == float(g0["dev_share"][sel].mean())
    assert r["unprofitable"] == float((g0["gain"][sel] < 0).mean()) and r["gain_mean"] == float(g0["gain"][sel].mean())
    for qq in (25, 50, 75):
        assert r["gain_q%d" % qq] == float(np.quantile(g0["gain"][sel], qq / 100))
    assert r["gain_dev_mean"] == float(g0["gain_dev"][sel].mean()) and r["low_mean"] == float(g0["low"][sel].mean())
    back = g0["ret_step"][sel]
    assert r["returned"] == float((back >= 0).mean()) and r["ret_step_mean"] == float(back[back >= 0].mean())
    assert r["dist_mean"] == float(g0["dist"][sel].mean())
    assert rows[1]["gain_mean"] == float(g1["gain"][sel].mean()) and rows[3]["solved"] == 5
    empty = rows[4]
    assert empty["games"] == 0 and empty["solved"] == 0
    assert all(empty[k] is None for k in empty if k not in ("group", "deviator", "games", "solved"))
    none_back = dict(g0, ret_step=np.full(10, -1, np.int32))
    assert dv.summarize_noise({0: none_back}, ids, 1, [0])[0]["ret_step_mean"] is None
    json.dumps(rows)


def test_shards_merge_to_the_unsharded_run_and_readers(tmp_path):
    from th_rl_amd import utils
    import deviation_mirror as M
    G = 10
    games = {0: _games(G), 1: dict(_games(G, seed=7), noise_prob=_games(G)["noise_prob"], stat_iters=_games(G)["stat_iters"])}
    ids = np.arange(G) % 2
    config = dict(NOISY, training={"n_games": G, "n_groups": 2, "groups": ids.tolist(), "deviation": {"noise": True}})
    opt = dv.parse_options(config["training"]["deviation"], config)
    nash, cartel = dv.optimal(config)
    # save / load
    one = tmp_path / "one"
    one.mkdir()
    for d in (0, 1):
        dv.save_noise_games(str(one), d, games[d])
        back = dv.load_noise_games(str(one), d)
        assert set(back) == set(games[d])
        for f in games[d]:
            assert np.array_equal(back[f], games[d][f]) and back[f].dtype == games[d][f].dtype, f
    assert sorted(f.name for f in one.iterdir()) == ["devn0_base.npy", "devn0_games.npy", "devn0_steps.npy", "devn1_base.npy",
                                                     "devn1_games.npy", "devn1_steps.npy", "devn_prob.npy",
                                                     "devn_stat_iters.npy"]
    # two fabricated shards (the noise-free arrays of the same games beside them) against the unsharded arrays
    rs = np.random.RandomState(6)
    q = rs.rand(G, 2 * 101 * 21)
    s0 = rs.uniform(0, 10, G)
    two = tmp_path / "two"
    shards = []
    for r, (lo, hi) in enumerate(((0, 4), (4, G))):
        sd = two / ("shard%d" % r)
        sd.mkdir(parents=True)
        shards.append(str(sd))
        summary = []
        for d in (0, 1):
            part = M.analyse(CFG, q[lo:hi], s0[lo:hi], deviator=d)
            if d == 0:
                np.save(sd / "dev_cycle.npy", np.stack([part["mu"], part["lam"]]).astype(np.int32))
                np.save(sd / "dev_cycle_reward.npy", part["cycle_reward"])
                np.save(sd / "dev_cycle_action.npy", part["cycle_action"])
            np.save(sd / ("dev%d_post.npy" % d),
                    np.stack([part["mu_post"], part["lam_post"], part["ret_step"], part["act_dev"]]).astype(np.int32))
            np.save(sd / ("dev%d_gain.npy" % d), part["gain"])
            summary += dv.summarize(part, ids[lo:hi], 2, nash, cartel, d)
        dv.save_json(str(sd / "deviation.json"), dv.describe(dict(opt, horizon_used=442), nash, cartel, summary))
        cut = {d: {f: v[..., lo:hi] for f, v in games[d].items()} for d in (0, 1)}
        for d in (0, 1):
            dv.save_noise_games(str(sd), d, cut[d])
        dv.save_json(str(sd / "deviation_noise.json"),
                     dv.describe_noise(opt, 101, dv.summarize_noise(cut, ids[lo:hi], 2, [0, 1])))
        (sd / "shard_config.json").write_text(json.dumps(dict(config, training=dict(config["training"], n_games=hi - lo,
                                                                                      game_offset=lo))))
    first = json.load(open(os.path.join(shards[0], "deviation.json")))
    assert "noise" not in first["options"]                  # deviation.json is what it is without the option
    desc = dv.merged(shards, str(two), config, opt, ids, 2, first)
    plain = dv.merged(shards, str(tmp_path), config, dv.parse_options(True, config), ids, 2, first)
    assert "noise" not in desc["options"] and desc == plain and len(desc["summary"]) == 4
    for d in (0, 1):
        both = dv.load_noise_games(str(two), d)
        for f in games[d]:
            assert np.array_equal(both[f], games[d][f]), (d, f)
    nd = json.load(open(two / "deviation_noise.json"))
    assert nd["options"]["noise"] == dv.NOISE_DEFAULTS and nd["n_cells"] == 101
    assert nd["summary"] == json.loads(json.dumps(dv.summarize_noise(games, ids, 2, [0, 1])))
    # without the option the merge writes nothing of it
    assert not any(f.name.startswith("devn") or f.name == "deviation_noise.json" for f in tmp_path.iterdir() if f.is_file())
    # the readers: per game from the shards (before and after the merge), the summary from the merged directory
    dv.save_json(str(one / "deviation_noise.json"), dv.describe_noise(opt, 101, dv.summarize_noise(games, ids, 2, [0, 1])))
    (one / "config.json").write_text(json.dumps(config))
    a, b = utils.deviation_noise_games(str(one), 1), utils.deviation_noise_games(str(two), 1)
    os.remove(two / "devn_prob.npy")                        # back to the shards alone
    c = utils.deviation_noise_games(str(two), 1)
    assert a.index.tolist() == b.index.tolist() == c.index.tolist() == list(range(G))
    for col in a.columns:
        assert np.array_equal(a[col].to_numpy(), b[col].to_numpy()) and np.array_equal(a[col].to_numpy(), c[col].to_numpy()), col
    assert a["gain"].tolist() == games[1]["gain"].tolist() and a["solved"].tolist() == dv.solved_noise(games[1]).tolist()
    assert a["base_reward_1"].tolist() == games[1]["base_reward"][1].tolist()
    df = utils.deviation_noise_summary(str(two))
    assert len(df) == 4 and df["n_cells"].tolist() == [101] * 4 and df["deviator"].tolist() == [0, 1, 0, 1]
    with pytest.raises(KeyError, match=r"no deviation test under noise \(devn_prob.npy\) under .* \(training.deviation.noise\)"):
        utils.deviation_noise_games(str(tmp_path / "none"), 0)
    with pytest.raises(KeyError, match=r"no deviation test under noise \(deviation_noise.json\) under .* \(training.deviation.noise\)"):
        utils.deviation_noise_summary(str(tmp_path / "none"))


def test_batch_method_is_shared_and_documented():
    from th_rl_amd import analysis
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    fn = analysis.AnalysisMethods.deviation_noise
    assert GameBatch.deviation_noise is fn and MixedGameBatch.deviation_noise is fn and "thrl_deviation_noise" in fn.__doc__
    assert [a.key for a in analysis.REGISTRY].count("deviation") == 1 and len(analysis.REGISTRY) == 12
