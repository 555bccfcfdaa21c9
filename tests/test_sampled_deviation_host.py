"""Host side of the deviation test of sampled play (th_rl_amd.sampled_deviation, thrl_sampled_deviation): the numpy mirror
against an independent dense solution, against an integer walk in the deterministic limit and against the best responses
of sampled_response_mirror, its exact identities, the kernel's own source as a stand-alone host program under sanitizers,
the args struct against the header, the exported symbol, every refusal of the entry point through the library loaded
without a GPU, option parsing, the summary and the readers.  No GPU."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sampled_deviation_mirror as SDM
import sampled_host_checks as HC
import sampled_mirror as SPM
import sampled_response_mirror as SRM
from sampled_mirror import AG, ENV, QQ, RF, SHIP
from th_rl_amd import sampled_deviation as sd
from th_rl_amd import sampled_play as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096                           # never dereferenced: validation fails before any launch
# the rounding allowance of an output, in units of ulp(the largest |entry| of the table it sums: reward, scaled, price; 1.0
# for a distance, a mass or a share).  The mirror's largest observed deviation from the dense solution on DENSE_CASES over
# both deviators, (K, L) = (12, 3), (12, 1), (12, 12) and a fixed action was 52 such units (SHIP, deviator 0, K = 12,
# L = 3: twelve steps of 441-term sums against matrix products of normalised rows); times 4
ROUNDING_UNITS = 208.0
DENSE_CASES = ("QQ", "QR", "QRA", "RR", "SHIP")
DENSE_MODES = ((12, 3, -1), (12, 1, -1), (12, 12, -1), (12, 3, 0))     # (K, L, action)


def allow(scale):
    return ROUNDING_UNITS * np.spacing(float(scale))


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _rows(tabs, probs, pol, eps, g):
    P, _, greedy = SPM.rows_of(tabs, {i: p[g:g + 1] for i, p in probs.items()}, pol[g:g + 1], eps[:, g:g + 1])
    return [p[0] for p in P], greedy[0]


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("name", DENSE_CASES)
def test_the_mirror_against_a_dense_solution(name):
    """Every period's rewards, actions, price, distance and mass, the baseline and dev_share against T x T matrices of
    normalised probabilities, numpy matrix products and numpy sums.  The tolerance is a rounding allowance only
    (ROUNDING_UNITS); the code under test never enters it."""
    tabs, probs, pol, eps, x0 = SDM.case_inputs(name)
    G, N = pol.shape[0], pol.shape[1]
    scale = {f: np.abs(np.asarray(tabs[f])).max() for f in ("reward", "scaled", "price")}
    worst = 0.0
    for dv in range(N):
        for K, L, action in DENSE_MODES:
            ref = SDM.analyse(tabs, probs, pol, eps, x0, deviator=dv, steps=K, dev_len=L, action=action, gamma=0.9)
            for g in range(G):
                P, _ = _rows(tabs, probs, pol, eps, g)
                dn = SDM.dense(tabs, P, ref["ad"][g], x0[g], dv, K, L)
                errs = ((np.abs(ref["reward_rows"][:, :, g] - dn["reward"]).max(), scale["reward"]),
                        (np.abs(ref["action_rows"][:, :, g] - dn["action"]).max(), scale["scaled"]),
                        (np.abs(ref["price_rows"][:, g] - dn["price"]).max(), scale["price"]),
                        (np.abs(ref["base_reward"][:, g] - dn["base_reward"]).max(), scale["reward"]),
                        (np.abs(ref["dist_rows"][:, g] - dn["dist"]).max(), 1.0),
                        (abs(ref["mass"][g] - dn["mass"][-1]), 1.0), (abs(ref["dist"][g] - dn["dist"][-1]), 1.0),
                        (abs(ref["dev_share"][g] - dn["dev_share"]), 1.0))
                for e, s in errs:
                    worst = max(worst, e / np.spacing(s))
                    assert e <= allow(s), (name, dv, K, L, action, g, e, allow(s))
                # what is derived from the rows: the gain, the low and the return, from the mirror's own rows
                diff = ref["reward_rows"][:, dv, g] - ref["base_reward"][dv, g]
                assert abs(ref["gain"][g] - (diff * 0.9 ** np.arange(K)).sum()) <= K * allow(np.abs(diff).max())
                assert abs(ref["gain_dev"][g] - (diff[:L] * 0.9 ** np.arange(L)).sum()) <= K * allow(np.abs(diff).max())
                if L < K:
                    assert ref["low"][g] == diff[L:].min() and ref["low_step"][g] == L + diff[L:].argmin()
                else:
                    assert ref["low"][g] == 0.0 and ref["low_step"][g] == -1 and ref["ret_step"][g] == -1
    print("%s: largest deviation %.1f units" % (name, worst))


def test_the_deterministic_limit_is_an_integer_walk():
    """All-QTable at eps = 0 with x_0 a unit mass: every x_tau is the unit mass on the tuple of the walk below, and the
    rewards, dist, ret_step, low and gain are that walk's, exactly."""
    config = {"agents": [dict(AG, actions=4), dict(AG, actions=3)], "environment": dict(ENV)}
    tabs, probs, pol, _, _ = SRM.make_inputs(config, 6, 61)
    G, T, D = 6, 12, int(tabs["n_prices"])
    rs = np.random.RandomState(62)
    row, R = np.asarray(tabs["row"]), np.asarray(tabs["reward"])
    greedy = np.minimum(pol.astype(np.int64), np.array([4, 3])[None, :, None] - 1)
    start = rs.randint(0, T, G)
    for _ in range(T):                                   # onto the cycle of greedy play, so that play can come back to it
        d = row[start]
        start = greedy[np.arange(G), 0, d] * 3 + greedy[np.arange(G), 1, d]
    x0 = np.zeros((G, T))
    x0[np.arange(G), start] = 1.0
    K, L, gam, dv = 10, 2, 0.75, 1
    devpol = rs.randint(0, 3, (G, D)).astype(np.uint16)
    out = SDM.analyse(tabs, probs, pol, [0.0, 0.0], x0, deviator=dv, steps=K, dev_len=L, dev_policy=devpol, gamma=gam, ret_tol=0.0)
    for g in range(G):
        t, w, gain, gain_dev, low, low_step, ret = int(start[g]), 1.0, 0.0, 0.0, 0.0, -1, -1
        for tau in range(K):
            d = row[t]
            a = [int(greedy[g, 0, d]), int(greedy[g, 1, d])]
            if tau < L:
                a[dv] = int(devpol[g, d])
            t = a[0] * 3 + a[1]
            assert out["reward_rows"][tau, :, g].tolist() == R[:, t].tolist()
            assert out["price_rows"][tau, g] == tabs["price"][t]
            assert out["dist_rows"][tau, g] == (0.0 if t == start[g] else 1.0)
            diff = R[dv, t] - R[dv, start[g]]
            term = w * diff
            gain += term
            if tau < L:
                gain_dev += term
            else:
                if tau == L or diff < low:
                    low, low_step = diff, tau
                if ret < 0 and t == start[g]:
                    ret = tau
            w *= gam
        assert (out["gain"][g], out["gain_dev"][g], out["low"][g]) == (gain, gain_dev, low)
        assert (out["low_step"][g], out["ret_step"][g], out["mass"][g]) == (low_step, ret, 1.0)
    assert (out["ret_step"] >= 0).any() and (out["low"] != 0.0).any()


@pytest.mark.parametrize("name", ("QQ", "QRA", "SHIP"))
def test_a_lasting_deviation_to_the_best_reply_earns_its_value(name):
    """ad = sampled_response_mirror's sigma* for the deviator, L = K = 48, gamma = 0.5: sum_tau gamma^tau r_delta(tau)
    against sum_d M_0(d) V*(d).  The tolerance is the sum of three terms: the truncation of the series after K periods,
    gamma^K max|reward_delta| / (1 - gamma); the Jacobi stopping bound of V*, gamma eval_tol / (1 - gamma); and the
    rounding allowance at the scale of a value, max|reward_delta| / (1 - gamma)."""
    tabs, probs, pol, eps, x0 = SDM.case_inputs(name)
    G, N, D = pol.shape[0], pol.shape[1], int(tabs["n_prices"])
    K, gam, eval_tol = 48, 0.5, 1e-12
    M0 = SPM.weights(tabs, np.ones((G, D)), x0)
    for dv in range(N):
        br = SRM.analyse(tabs, probs, pol, eps, gam, agents=[dv], eval_tol=eval_tol)
        assert (br["iters"][dv] >= 0).all()
        out = SDM.analyse(tabs, probs, pol, eps, x0, deviator=dv, steps=K, dev_len=K, dev_policy=br["br_policy"][dv], gamma=gam)
        got = (out["reward_rows"][:, dv, :] * (gam ** np.arange(K))[:, None]).sum(axis=0)
        want = (M0 * br["v_opt"][dv]).sum(axis=1)
        rmax = np.abs(np.asarray(tabs["reward"])[dv]).max()
        truncation = gam ** K * rmax / (1.0 - gam)
        jacobi = gam * eval_tol / (1.0 - gam)
        rounding = allow(rmax / (1.0 - gam))
        assert np.abs(got - want).max() <= truncation + jacobi + rounding, (name, dv, np.abs(got - want).max())
        # and the gain is that sum less the baseline's
        base = out["base_reward"][dv] * (gam ** np.arange(K)).sum()
        assert np.abs(out["gain"] - (got - base)).max() <= K * allow(rmax)
        assert np.array_equal(out["gain"], out["gain_dev"])


def test_the_own_greedy_row_of_an_exact_table_is_no_deviation():
    """A QTable deviator at eps 0 "deviated" to its own greedy row: dev_share == 0.0 exactly, and every row equals plain
    propagation, bit for bit, whatever the length of the deviation."""
    tabs, probs, pol, eps, x0 = SDM.case_inputs("QRA")
    eps = eps.copy()
    eps[0] = 0.0
    own = np.minimum(pol[:, 0].astype(np.int64), 1).astype(np.uint16)
    one = SDM.analyse(tabs, probs, pol, eps, x0, deviator=0, steps=8, dev_len=1, dev_policy=own, gamma=0.9)
    all8 = SDM.analyse(tabs, probs, pol, eps, x0, deviator=0, steps=8, dev_len=8, dev_policy=own, gamma=0.9)
    assert (one["dev_share"] == 0.0).all() and (all8["dev_share"] == 0.0).all()
    P, Z, _ = SPM.rows_of(tabs, probs, pol, eps)
    act = SPM.actions_of(tabs)
    x = x0
    for tau in range(8):
        x = SDM.price_sums(tabs, P, Z, act, x)
        rew, sca, price, dist, _ = SDM.outcome(tabs, x, x0)
        for out in (one, all8):
            assert np.array_equal(out["reward_rows"][tau], rew) and np.array_equal(out["action_rows"][tau], sca)
            assert np.array_equal(out["price_rows"][tau], price) and np.array_equal(out["dist_rows"][tau], dist)
    # against a mixing rival the same strategy does deviate from an exploring table
    eps[0] = 0.1
    assert (SDM.analyse(tabs, probs, pol, eps, x0, deviator=0, steps=2, dev_len=1, dev_policy=own)["dev_share"] > 0.0).all()


@pytest.mark.parametrize("name", ("QR", "RR"))
def test_the_baseline_is_sampled_plays_long_run_profit_bit_for_bit(name):
    tabs, probs, pol, eps, _ = SDM.case_inputs(name)
    st = SPM.analyse(tabs, probs, pol, eps, max_iters=40)
    out = SDM.analyse(tabs, probs, pol, eps, st["pi"], deviator=1, steps=1, dev_len=1)
    assert np.array_equal(out["base_reward"], st["samp_reward"]) and np.array_equal(out["base_action"], st["samp_action"])
    assert np.array_equal(out["base_price"], st["samp_price"]) and (st["iters"] > 0).all()


# ------------------------------------------------------------------------------------------------ the kernel on the host
def build_check(path, sanitizer):
    HC.build_check("sampled_deviation_check.cpp", path, sanitizer)


def host_cases():
    """(what, case, dict of analyse()'s and write_case()'s shared arguments, per-game epsilon with a bad entry, rows)."""
    out = []
    for name in ("QQ", "QRA", "RR"):
        tabs, probs, pol, eps, x0 = SDM.case_inputs(name)
        G, N, D = pol.shape[0], pol.shape[1], int(tabs["n_prices"])
        rs = np.random.RandomState(len(name))
        bad = eps.copy()
        if G > 2:
            bad[0, 1] = np.nan                               # agent 0 is a QTable agent in each of them: game 1 is not solved
        out.append(("%s best response" % name, name, dict(deviator=N - 1, steps=12, dev_len=3, action=-1, gamma=0.9), bad, (0, None)))
        out.append(("%s a fixed action, per-game gamma, the second row chunk" % name, name,
                    dict(deviator=0, steps=12, dev_len=1, action=1, gamma=rs.uniform(0.0, 1.0, G)), eps, (5, 7)))
        A = int(tabs["n_actions"][N - 1])
        devpol = rs.randint(0, A + 2, (G, D)).astype(np.uint16)         # entries at and above A: clamped
        out.append(("%s a given strategy while all steps last, scalar epsilon" % name, name,
                    dict(deviator=N - 1, steps=5, dev_len=5, action=-1, dev_policy=devpol, gamma=1.0), eps[:, 0].copy(), (0, None)))
        out.append(("%s one step" % name, name, dict(deviator=0, steps=1, dev_len=1, action=-1, gamma=0.0), eps, (0, None)))
    return out


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
def test_the_kernels_source_on_the_host_equals_the_mirror_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sampled_deviation_check")
    build_check(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    unsolved = 0
    for k, (what, name, kw, eps, (rb, rc)) in enumerate(host_cases()):
        tabs, probs, pol, _, x0 = SDM.case_inputs(name)
        ref = SDM.analyse(tabs, probs, pol, eps, x0, **kw)
        path = str(tmp_path / ("case%d.bin" % k))
        SDM.write_case(path, tabs, probs, pol, eps, x0, ref, 2, row_begin=rb, row_count=rc, **kw)
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert p.returncode == 0 and "equal to the mirror bit for bit" in p.stdout, (what, p.stdout[-3000:])
        if np.ndim(eps) == 2 and np.isnan(eps).any():       # the case is what it claims: an unsolved game beside solved ones
            assert ref["low_step"][1] == -1 and not ref["reward_rows"][:, :, 1].any() and ref["reward_rows"][:, :, 0].all()
            unsolved += 1
    assert unsolved == 2


# ------------------------------------------------------------------------------------------------ the entry point
def test_args_struct_matches_the_header():
    from th_rl_amd import _lib
    HC.assert_struct_matches_header(
        _lib.SampledDeviationArgs, "thrl_sampled_deviation_args", "thrl_sampled_deviation.h",
        [("THRL_SD_MAX_LDS", _lib.SD_MAX_LDS), ("THRL_SD_POLICY", _lib.SD_POLICY), ("THRL_TP_MAX_TUPLES", 4096),
         ("THRL_DEV_MAX_STEPS", _lib.DEV_MAX_STEPS), ("THRL_ABI_VERSION", 4)])
    assert sd.MAX_LDS == _lib.SD_MAX_LDS == 160 * 1024 and _lib.ABI_VERSION == 4


def test_the_library_exports_the_call_beside_the_55(lib):
    from th_rl_amd import _lib
    assert _lib.SAMPLED_DEVIATION_SYMBOLS == ["thrl_sampled_deviation"] and len(_lib.SYMBOLS) == 55
    assert not set(_lib.SAMPLED_DEVIATION_SYMBOLS) & set(_lib.SYMBOLS + _lib.RESPONSE_SYMBOLS + _lib.RESPONSE_NOISE_SYMBOLS)
    assert hasattr(lib, "thrl_sampled_deviation")
    header = open(os.path.join(ROOT, "include", "thrl_sampled_deviation.h")).read()
    assert re.findall(r"^\w[\w\s\*]*?\b(thrl_\w+)\(", header, flags=re.M) == _lib.SAMPLED_DEVIATION_SYMBOLS
    assert lib.thrl_version() == 4


SD_TABLES = ("dpolicy", "grp_first", "grp_perm", "reward", "scaled", "price", "weights")
SD_OUTPUTS = ("base_reward", "base_action", "base_price", "dev_share", "gain", "gain_dev", "low", "low_step", "ret_step", "dist",
              "mass")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    c = config or SHIP
    qt = {"agents": [dict(AG, actions=a.get("actions", 21)) for a in c["agents"]], "environment": c["environment"]}
    return _lib.cfg_from_config(qt, n_games, 0)[0]


def sd_args(**kw):
    from th_rl_amd import _lib
    a = _lib.SampledDeviationArgs()
    a.n_games, a.n_tuples, a.n_prices, a.deviator, a.dev_len, a.n_steps, a.dev_action = 64, 441, 441, 1, 1, 32, -1
    a.kind[1], a.prob[1], a.eps[0], a.gamma, a.ret_tol = 1, FAKE, 0.01, 0.95, 1e-6
    for f in SD_TABLES + SD_OUTPUTS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k in ("kind", "eps", "prob", "reserved"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


NAN = float("nan")
SD_BAD = [dict(n_games=0), dict(flags=2), dict(flags=-1), dict(reserved=[1]), dict(reserved=[0, 1]), dict(kind=[0, 4]),
          dict(kind=[-1, 0]), dict(kind=[0, 1], n_tuples=21 * 40, n_prices=21), dict(n_tuples=0), dict(n_tuples=440),
          dict(n_prices=0), dict(n_prices=442), dict(deviator=-1), dict(deviator=2), dict(dev_len=0), dict(n_steps=0),
          dict(dev_len=33), dict(n_steps=1 << 30), dict(dev_action=-2), dict(dev_action=21), dict(flags=1, dev_action=0),
          dict(flags=1, dev_action=-2), dict(row_begin=-1), dict(row_count=-1), dict(row_begin=30, row_count=3), dict(ret_tol=-1e-9),
          dict(ret_tol=NAN), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=NAN), dict(eps=[-0.1]), dict(eps=[1.5]), dict(eps=[NAN])]


def test_the_entry_point_validates_before_any_launch(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path that the host can see, with its code; none touches a device."""
    from th_rl_amd import _lib
    cfg = _cfg()
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})           # a network has at most 32
    call = lib.thrl_sampled_deviation
    assert (1 << 30) > _lib.DEV_MAX_STEPS
    for bad in SD_BAD:
        c = forty if bad.get("n_tuples") == 21 * 40 else cfg
        assert call(ctypes.byref(c), ctypes.byref(sd_args(**bad)), None) == -1, bad
        assert lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sd_args(flags=1, dev_action=3)), None) == -1
    assert b"dev_action=3" in lib.thrl_last_error() and b"[0,0)" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sd_args(gamma=1.5)), None) == -1 and b"1 - gamma=-0.5" in lib.thrl_last_error()
    # both ends of gamma's range are allowed; a neural agent's epsilon is not read; the per-game arrays take the place of
    # the scalars: each of these passes every check of the arguments and stops at a missing pointer
    for fine in (dict(gamma=0.0), dict(gamma=1.0), dict(eps=[0.0, 7.0]), dict(gamma=7.0, sweep_gamma=FAKE), dict(eps=[7.0], eps_g=FAKE),
                 dict(dev_action=20, deviator=0), dict(row_begin=29, row_count=3), dict(flags=1, dev_policy=FAKE), dict(dev_len=32)):
        assert call(ctypes.byref(cfg), ctypes.byref(sd_args(mass=None, **fine)), None) == -2, fine
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097, n_prices=1)):
        assert call(ctypes.byref(cfg), ctypes.byref(sd_args(**unsupported)), None) == -3, unsupported
    # the working set: refused from the shape alone, before any pointer is looked at, exactly where working_set says (the
    # heaviest accepted and the lightest refused of QTable 20..39 x Reinforce 21 / 24 / 28 / 32)
    shape = lambda A, B: {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}
    for (A, B), rc, nbytes in (((28, 32), -2, 161552), ((35, 32), -3, 171904)):
        ws = sd.working_set(shape(A, B))
        assert ws["bytes"] == nbytes and ws["fits"] == (rc == -2)
        a = sd_args(n_tuples=ws["T"], n_prices=ws["D"], gain=None)
        assert call(ctypes.byref(_cfg(shape(A, B))), ctypes.byref(a), None) == rc, (A, B, ws)
    assert b"171904 bytes of LDS" in lib.thrl_last_error()
    for null in SD_TABLES + SD_OUTPUTS:
        assert call(ctypes.byref(cfg), ctypes.byref(sd_args(**{null: None})), None) == -2, null
        assert null.encode() in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sd_args(prob=[None, None])), None) == -2
    assert b"prob[1]" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sd_args(flags=1)), None) == -2 and b"dev_policy" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), None, None) == -2
    assert call(None, ctypes.byref(sd_args()), None) == -2


def test_the_new_entry_point_adds_no_refusal_words():
    """thrl_api_analysis.hip's fail( format strings are recorded (tests/test_api_refusals_host.py): the new entry point
    words its refusals through the shared helpers and the forms that were there."""
    src = open(os.path.join(ROOT, "th_rl_amd", "csrc", "thrl_api_analysis.hip")).read()
    body = src[src.index("int thrl_sampled_deviation("):]
    body = body[:body.index("\n}\n")]
    before = src[:src.index("int thrl_sampled_deviation(")]
    for fmt in re.findall(r'\bfail\(THRL_ERR_\w+,\s*"((?:[^"\\]|\\.)*)"', body):
        assert 'fail(THRL_ERR_' in before and '"%s"' % fmt in before, fmt


# ------------------------------------------------------------------------------------------------ options and artefacts
OLD_OPTIONS = [True, {}, {"pi": True}, {"epsilon": 0.1, "start": "state"}, {"epsilon": [0.1, 0.2], "tol": 1e-9, "max_iters": 100},
               {"noise": True}, {"noise": {"noise_prob": 0.1, "resolution": 64}, "start": "reset"}, {"noise": None},
               {"response": True}, {"response": {"agents": [1], "policies": True}, "pi": True}]


def test_parse_options():
    noisy = dict(SHIP, environment=dict(ENV, noise_prob=0.05))
    for opt in OLD_OPTIONS:                              # without the key every option dict parses to what it did
        c = noisy if isinstance(opt, dict) and opt.get("noise") is True else SHIP
        got = sp.parse_options(opt, c)
        assert "deviation" not in got
        if isinstance(opt, dict):
            assert sp.parse_options(dict(opt, deviation=None), c) == got and sp.parse_options(dict(opt, deviation=False), c) == got
            if not opt.get("noise"):
                assert sp.parse_options(dict(opt, deviation=True), c) == dict(got, deviation=dict(sd.DEFAULTS, agents=[0, 1]))
    assert sp.parse_options(True, SHIP) == dict(sp.DEFAULTS)
    full = {"agents": [1, 0, 1], "steps": 16, "dev_len": 4, "action": 3, "ret_tol": 1e-5}
    assert sp.parse_options({"deviation": full}, SHIP)["deviation"] == dict(full, agents=[0, 1])
    assert sp.parse_options({"deviation": {"action": "best_reply"}}, SHIP)["deviation"]["action"] == "best_reply"
    for opt in ({"deviation": True, "noise": True}, {"deviation": {}, "noise": {"noise_prob": 0.1}}):
        with pytest.raises(ValueError, match="follow-up"):
            sp.parse_options(opt, noisy)
    for bad in ({"agents": []}, {"agents": [2]}, {"agents": [True]}, {"agents": 0}, {"steps": 0}, {"steps": 1.5}, {"dev_len": 0},
                {"dev_len": 33}, {"steps": 1 << 30}, {"action": 21}, {"action": -1}, {"action": "worst"}, {"action": True},
                {"ret_tol": -1.0}, {"ret_tol": "x"}, {"tol": 0.1}, 7):
        with pytest.raises(ValueError):
            sp.parse_options({"deviation": bad}, SHIP)
    big = {"agents": [dict(AG, actions=40), dict(RF, actions=32)], "environment": dict(ENV)}
    with pytest.raises(ValueError, match="working set"):
        sd.parse_options(True, big)


def test_working_set_follows_the_layout():
    assert sd.working_set(SHIP) == dict(bytes=62160, T=441, D=441, fits=True)
    for config in (QQ, SPM.QRA, SPM.RR, SHIP):
        ws, base = sd.working_set(config), sp.working_set(config)
        r16 = lambda x: (x + 15) // 16 * 16
        assert ws["bytes"] == base["bytes"] + r16(2 * ws["D"]) + r16(8 * ws["D"]) + 512


def test_summary_rows_and_readers(tmp_path):
    from th_rl_amd import utils
    N, G = 2, 6
    rs = np.random.RandomState(5)
    games = {}
    for d in (0, 1):
        r = {f: rs.uniform(-1, 1, G) for f in sd.FLOAT}
        r.update({f: rs.uniform(1, 2, (N, G)) for f in sd.AGENT})
        r.update(low_step=rs.randint(1, 8, G).astype(np.int32), ret_step=np.array([3, -1, 5, -1, -1, 7], np.int32),
                 gamma=np.full(G, 0.9), epsilon=np.zeros((N, G)), stat_iters=np.arange(G, dtype=np.int32),
                 solved=np.array([True, True, False, True, True, True]))
        r["dev_share"] = np.abs(r["dev_share"])
        r["dev_share"][0] = 0.0
        games[d] = r
    ids = np.array([0, 0, 0, 1, 1, 1])
    rows = sd.summarize(games, ids, 2, [0, 1])
    assert [(x["group"], x["deviator"]) for x in rows] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    a = rows[0]
    g0 = games[0]
    assert a["games"] == 3 and a["solved"] == 2 and a["deviates"] == 0.5
    assert abs(a["gain_mean"] - g0["gain"][:2].mean()) < 1e-12 and abs(a["gain_q50"] - np.median(g0["gain"][:2])) < 1e-12
    assert a["unprofitable"] == float((g0["gain"][:2] < 0).mean()) and a["returned"] == 0.5 and a["ret_step_mean"] == 3.0
    assert abs(a["low_mean"] - g0["low"][:2].mean()) < 1e-12 and abs(rows[2]["dist_mean"] - g0["dist"][3:].mean()) < 1e-12
    from th_rl_amd import deviation as dv
    noise_cols = set(dv.summarize_noise({0: dict(g0, noise_prob=np.full(G, 0.5))}, ids, 2, [0])[0])
    assert set(a) == noise_cols                          # deviation_noise_summary's columns
    for d in (0, 1):
        sd.save_games(str(tmp_path), d, games[d])
    for d in (0, 1):
        back = sd.load_games(str(tmp_path), d)
        for f in sd.PER_GAME:
            assert np.array_equal(back[f], games[d][f]), f
    with pytest.raises(KeyError, match=r"training\.sampled_play\.deviation"):
        utils.sampled_deviation_summary(str(tmp_path))
    desc = sd.describe(dict(sd.DEFAULTS, agents=[0, 1]), 9, 5, rows)
    assert json.loads(json.dumps(desc)) == desc
    json.dump(desc, open(tmp_path / "sampled_deviation.json", "w"))
    df = utils.sampled_deviation_summary(str(tmp_path))
    assert len(df) == 4 and df["T"][0] == 9 and df["n_prices"][0] == 5 and "gain_q50" in df.columns
    gm = utils.sampled_deviation_games(str(tmp_path), 1)
    assert len(gm) == G and np.array_equal(gm["gain"], games[1]["gain"]) and np.array_equal(gm["solved"], games[1]["solved"])
    assert np.array_equal(gm["base_reward_1"], games[1]["base_reward"][1]) and list(gm.index) == list(range(G))
    json.dump(dict(desc, options=dict(desc["options"], agents=[0])), open(tmp_path / "sampled_deviation.json", "w"))
    with pytest.raises(KeyError, match="deviator 1 was not analysed"):
        utils.sampled_deviation_games(str(tmp_path), 1)
