"""Host side of the best responses to sampled play (th_rl_amd.sampled_response, thrl_sampled_response): the numpy mirror
against an independent dense solution and against closed forms, the kernel's own source as a stand-alone host program
under sanitizers, the args struct against the header, the exported symbol, every refusal of the entry point through the
library loaded without a GPU, option parsing, the summary and the readers.  No GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import sampled_host_checks as HC
import sampled_mirror as SPM
import sampled_response_mirror as SRM
from sampled_mirror import AG, ENV, QQ, QR, QRA, RF, RR, SHIP
from th_rl_amd import sampled_play as sp
from th_rl_amd import sampled_response as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096                           # never dereferenced: validation fails before any launch
# the rounding allowance beside the Jacobi stopping bound, in units of ulp(max |V|) / (1 - gamma) (a sweep's rounding error,
# carried through the geometric series): the mirror's largest observed excess over the bound against the dense solution on
# DENSE_CASES was 0.975 units (QQ at gamma 0.95: error 1.96e-11 against a bound of 1.90e-11, max |V| = 166); times 4
ROUNDING_UNITS = 3.9
# (config, games, seed, gamma per agent)
DENSE_CASES = {"QQ": (QQ, 4, 41, [0.95, 0.9]), "QR": (QR, 4, 42, [0.95, 0.995]), "QRA": (QRA, 3, 43, [0.95, 0.99, 0.9]),
               "RR": (RR, 1, 44, [0.95, 0.9]), "SHIP": (SHIP, 1, 45, [0.5, 0.6])}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _rows(tabs, probs, pol, eps, g):
    P, _, greedy = SPM.rows_of(tabs, {i: p[g:g + 1] for i, p in probs.items()}, pol[g:g + 1], eps[:, g:g + 1])
    return [p[0] for p in P], greedy[0]


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_the_mirror_against_a_dense_solution(name):
    """V_pi against numpy.linalg.solve on the D x D chain of normalised probabilities, V* against dense value iteration
    run to a fixed point.  Tolerance: the Jacobi stopping bound gamma eval_tol / (1 - gamma) plus the rounding allowance
    ROUNDING_UNITS ulp(max |V|) / (1 - gamma): the mirror's largest observed excess over the stopping bound on these cases,
    0.975 such units (the largest error / bound ratio was 1.21, QR at gamma 0.995), with a margin of 4.  The code under
    test never enters this number."""
    config, G, seed, gammas = DENSE_CASES[name]
    tabs, probs, pol, eps, pi = SRM.make_inputs(config, G, seed)
    out = SRM.analyse(tabs, probs, pol, eps, gammas)
    assert (out["iters"] >= 0).all()
    worst = 0.0
    for g in range(G):
        P, _ = _rows(tabs, probs, pol, eps, g)
        for i, gam in enumerate(gammas):
            Vpi, Vs = SRM.dense(tabs, P, i, gam)
            bound = gam * 1e-12 / (1.0 - gam)
            allow = ROUNDING_UNITS * np.spacing(np.abs(Vs).max()) / (1.0 - gam)
            e_pi, e_s = np.abs(out["v_pi"][i, g] - Vpi).max(), np.abs(out["v_opt"][i, g] - Vs).max()
            worst = max(worst, e_pi / bound, e_s / bound)
            assert e_pi <= bound + allow and e_s <= bound + allow, (name, g, i, e_pi, e_s, bound, allow)
            assert (Vs >= Vpi - bound - allow).all()
    print("%s: largest error / stopping bound %.3f" % (name, worst))


def test_gamma_zero_is_the_one_period_best_response():
    tabs, probs, pol, eps, pi = SRM.make_inputs(QRA, 3, 51)
    out = SRM.analyse(tabs, probs, pol, eps, 0.0)
    act = SPM.actions_of(tabs)
    R = np.asarray(tabs["reward"])
    for g in range(3):
        P, _ = _rows(tabs, probs, pol, eps, g)
        norm = [p / p.sum(axis=1, keepdims=True) for p in P]
        for i in range(3):
            w = np.ones((P[0].shape[0], act.shape[1]))
            for j in range(3):
                if j != i:
                    w = w * norm[j][:, act[j]]
            q = np.stack([(w * R[i] * (act[i] == k)).sum(axis=1) for k in range(P[i].shape[1])], axis=1)
            assert np.abs(out["v_opt"][i, g] - q.max(axis=1)).max() <= 1e-12 * np.abs(q).max()
            assert out["sweeps"][i, g] >= 3 and out["iters"][i, g] >= 0


def test_a_uniform_rival_gives_one_value_at_every_price():
    """A QTable rival at epsilon = 1 plays uniformly whatever the price: V* is max_k mean_a R_i(k, a) / (1 - gamma) at
    every price, to the stopping bound and the rounding allowance of the dense comparison."""
    config = {"agents": [dict(AG, actions=4), dict(AG, actions=3)], "environment": dict(ENV)}
    tabs, probs, pol, eps, pi = SRM.make_inputs(config, 2, 52)
    gam = 0.9
    out = SRM.analyse(tabs, probs, pol, [0.1, 1.0], gam, agents=[0])
    R = np.asarray(tabs["reward"])[0].reshape(4, 3)
    want = R.mean(axis=1).max() / (1.0 - gam)
    assert np.abs(out["v_opt"][0] - want).max() <= gam * 1e-12 / (1.0 - gam) + ROUNDING_UNITS * np.spacing(want) / (1.0 - gam)
    assert (out["br_policy"][0] == R.mean(axis=1).argmax()).all()


def test_the_best_response_fed_back_loses_nothing():
    tabs, probs, pol, eps, pi = SRM.make_inputs(QR, 4, 53)
    first = SRM.analyse(tabs, probs, pol, eps, 0.9, agents=[0], pi=pi)
    assert (first["n_diff"][0] > 0).any()
    back = pol.copy()
    back[:, 0] = first["br_policy"][0]
    e0 = eps.copy()
    e0[0] = 0.0
    again = SRM.analyse(tabs, probs, back, e0, 0.9, agents=[0], pi=pi)
    assert not again["n_diff"][0].any() and not again["iters"][0].any()
    assert (again["loss_all"][0] <= 0.9 * 1e-12 / 0.1 / np.abs(again["v_opt"][0]).min(axis=1) * 4).all()
    assert np.allclose(again["br_prob_w"][0], pi.sum(axis=1))


# ------------------------------------------------------------------------------------------------ the kernel on the host
def build_check(path, sanitizer):
    HC.build_check("sampled_response_check.cpp", path, sanitizer)


def run_cases(exe, d):
    """Every case of sampled_response_mirror.host_cases() through the program: the return codes and the outputs."""
    res = []
    for k, (what, kw, blocks) in enumerate(SRM.host_cases()):
        ref = SRM.analyse(**kw)
        path = os.path.join(d, "case%d.bin" % k)
        SRM.write_case(path, kw["tabs"], kw["probs"], kw["dpolicy"], kw["eps"], kw["gamma"], kw["agents"], kw["eval_tol"],
                       kw["max_sweeps"], kw["pi"], ref, blocks)
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        res.append((what, p.returncode, p.stdout, ref))
    return res


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
def test_the_kernels_source_on_the_host_equals_the_mirror_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sampled_response_check")
    build_check(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    res = run_cases(exe, str(tmp_path))
    for what, rc, text, ref in res:
        assert rc == 0 and "equal to the mirror bit for bit" in text, (what, text[-3000:])
    # the cases are what they claim: unsolved games of each kind, a team split and D > 256
    first, capped = res[0][3], res[1][3]
    assert (first["iters"][:, 1] == -1).all() and not first["sweeps"][:, 1].any()                  # the bad epsilon
    assert first["iters"][1, 2] == -1 and np.isnan(first["loss_all"][1, 2]) and np.isnan(first["loss_all"][0, 4])
    assert (first["iters"][:, [0, 3, 5]] >= 0).all()
    assert (capped["iters"][1] == -1).all() and (capped["sweeps"][1] == 3).all()
    assert "team=4" in res[3][2] and "D=441" in res[4][2] and "team=1" in res[4][2]
    assert max(r[3]["iters"].max() for r in res) >= 1 and max(r[3]["n_diff"].max() for r in res) >= 1


# ------------------------------------------------------------------------------------------------ the entry point
def test_args_struct_matches_the_header():
    from th_rl_amd import _lib
    HC.assert_struct_matches_header(
        _lib.SampledResponseArgs, "thrl_sampled_response_args", "thrl_response.h",
        [("THRL_SR_MAX_LDS", _lib.SR_MAX_LDS), ("THRL_STAT_MAX_ITERS", _lib.STAT_MAX_ITERS), ("THRL_TP_MAX_TUPLES", 4096),
         ("THRL_EQ_MAX_ITERS", SRM.EQ_MAX_ITERS), ("THRL_ABI_VERSION", 4)])
    assert sr.MAX_LDS == _lib.SR_MAX_LDS == 160 * 1024 and _lib.ABI_VERSION == 4


def test_the_library_exports_the_call_beside_the_55(lib):
    from th_rl_amd import _lib
    assert _lib.RESPONSE_SYMBOLS == ["thrl_sampled_response"] and len(_lib.SYMBOLS) == 55
    assert not set(_lib.RESPONSE_SYMBOLS) & set(_lib.SYMBOLS)
    for name in _lib.RESPONSE_SYMBOLS:
        assert hasattr(lib, name), name
    import re
    header = open(os.path.join(ROOT, "include", "thrl_response.h")).read()
    assert re.findall(r"^\w[\w\s\*]*?\b(thrl_\w+)\(", header, flags=re.M) == _lib.RESPONSE_SYMBOLS
    assert lib.thrl_version() == 4


SR_REQUIRED = ("dpolicy", "grp_first", "grp_perm", "reward", "iters", "sweeps", "n_diff", "loss_all", "loss_mean")
SR_WEIGHTED = ("loss_w", "gain_w", "v_w", "br_prob_w")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    c = config or SHIP
    qt = {"agents": [dict(AG, actions=a.get("actions", 21)) for a in c["agents"]], "environment": c["environment"]}
    return _lib.cfg_from_config(qt, n_games, 0)[0]


def sr_args(**kw):
    from th_rl_amd import _lib
    a = _lib.SampledResponseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.agents, a.max_sweeps, a.eval_tol = 64, 441, 441, 3, 100, 1e-12
    a.kind[1], a.prob[1], a.eps[0], a.gamma[0], a.gamma[1] = 1, FAKE, 0.01, 0.95, 0.995
    for f in SR_REQUIRED:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k in ("kind", "eps", "prob", "gamma", "reserved"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


SR_BAD = [dict(n_games=0), dict(flags=1), dict(flags=-1), dict(reserved=[1]), dict(reserved=[0, 1]), dict(agents=0),
          dict(agents=4), dict(agents=-1), dict(n_tuples=0), dict(n_tuples=440), dict(n_prices=0), dict(n_prices=442),
          dict(gamma=[1.0]), dict(gamma=[0.5, -0.1]), dict(gamma=[float("nan")]), dict(max_sweeps=0), dict(max_sweeps=65537),
          dict(eval_tol=-1e-9), dict(eval_tol=float("nan")), dict(eps=[-0.1]), dict(eps=[1.5]), dict(eps=[float("nan")]),
          dict(kind=[0, 4]), dict(kind=[-1, 0]), dict(kind=[0, 1], n_tuples=21 * 40, n_prices=21)]


def test_the_entry_point_validates_before_any_launch(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path that the host can see; none touches a device."""
    cfg = _cfg()
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})           # a network has at most 32
    call = lib.thrl_sampled_response
    for bad in SR_BAD:
        c = forty if bad.get("n_tuples") == 21 * 40 else cfg
        assert call(ctypes.byref(c), ctypes.byref(sr_args(**bad)), None) == -1, bad
        assert lib.thrl_last_error()
    # the gamma of an agent that is not solved and a neural agent's epsilon are not read; the per-game arrays take the
    # place of the scalars
    assert call(ctypes.byref(cfg), ctypes.byref(sr_args(agents=1, gamma=[0.5, 7.0], iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(sr_args(eps=[0.0, 7.0], iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(sr_args(gamma=[7.0], sweep_gamma=FAKE, iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(sr_args(eps=[7.0], eps_g=FAKE, iters=None)), None) == -2
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097, n_prices=1)):
        assert call(ctypes.byref(cfg), ctypes.byref(sr_args(**unsupported)), None) == -3, unsupported
    # the working set: refused from the shape alone, before any pointer is looked at, exactly where working_set says (the
    # heaviest accepted and the lightest refused of QTable 20..35 x Reinforce 24..32)
    shape = lambda A, B: {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}
    for (A, B), rc, nbytes in (((33, 30), -2, 163616), ((26, 32), -3, 165392)):
        ws = sr.working_set(shape(A, B))
        assert ws["bytes"] == nbytes and ws["fits"] == (rc == -2)
        a = sr_args(n_tuples=ws["T"], n_prices=ws["D"], loss_all=None)
        assert call(ctypes.byref(_cfg(shape(A, B))), ctypes.byref(a), None) == rc, (A, B, ws)
    assert b"165392 bytes of LDS" in lib.thrl_last_error()
    for null in SR_REQUIRED:
        assert call(ctypes.byref(cfg), ctypes.byref(sr_args(**{null: None})), None) == -2, null
    assert call(ctypes.byref(cfg), ctypes.byref(sr_args(prob=[None, None])), None) == -2
    assert b"prob[1]" in lib.thrl_last_error()
    full = {f: FAKE for f in SR_WEIGHTED}
    for null in SR_WEIGHTED:
        assert call(ctypes.byref(cfg), ctypes.byref(sr_args(pi=FAKE, **dict(full, **{null: None}))), None) == -2, null
        assert b"with pi" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), None, None) == -2
    assert call(None, ctypes.byref(sr_args()), None) == -2


# ------------------------------------------------------------------------------------------------ options and artefacts
OLD_OPTIONS = [True, {}, {"pi": True}, {"epsilon": 0.1, "start": "state"}, {"epsilon": [0.1, 0.2], "tol": 1e-9, "max_iters": 100},
               {"noise": True}, {"noise": {"noise_prob": 0.1, "resolution": 64}, "start": "reset"}, {"noise": None}]


def test_parse_options():
    noisy = dict(SHIP, environment=dict(ENV, noise_prob=0.05))
    for opt in OLD_OPTIONS:
        c = noisy if isinstance(opt, dict) and opt.get("noise") is True else SHIP
        got = sp.parse_options(opt, c)
        assert "response" not in got
        want = dict(sp.DEFAULTS)
        if isinstance(opt, dict):
            want.update({k: v for k, v in opt.items() if k != "noise"})
            if opt.get("noise"):
                want["noise"] = dict(sp.NOISE_DEFAULTS, **(opt["noise"] if isinstance(opt["noise"], dict) else {}))
        want["tol"] = float(want["tol"])
        assert got == want, (opt, got, want)
        if isinstance(opt, dict):
            assert sp.parse_options(dict(opt, response=None), c) == got and sp.parse_options(dict(opt, response=False), c) == got
    assert sp.parse_options({"response": True}, SHIP) == dict(sp.DEFAULTS, response=dict(sr.DEFAULTS))
    full = {"agents": [1, 0, 1], "eval_tol": 1e-10, "max_sweeps": 512, "policies": True}
    assert sp.parse_options({"pi": True, "response": full}, SHIP)["response"] == dict(full, agents=[0, 1])
    for opt in ({"response": True, "noise": True}, {"response": {}, "noise": {"noise_prob": 0.1}}):
        with pytest.raises(ValueError, match="follow-up"):
            sp.parse_options(opt, noisy)
    for bad in ({"agents": []}, {"agents": [2]}, {"agents": [True]}, {"agents": 0}, {"eval_tol": -1.0}, {"eval_tol": "x"},
                {"max_sweeps": 0}, {"max_sweeps": 65537}, {"max_sweeps": 1.5}, {"policies": 1}, {"tol": 0.1}, 7):
        with pytest.raises(ValueError):
            sp.parse_options({"response": bad}, SHIP)
    big = {"agents": [dict(AG, actions=40), dict(RF, actions=32)], "environment": dict(ENV)}
    with pytest.raises(ValueError, match="working set"):
        sr.parse_options(True, big)


def test_working_set_follows_the_layout():
    ws = sr.working_set(SHIP)
    assert ws == dict(bytes=69488, T=441, D=441, team=1, fits=True)
    assert sr.working_set(RR)["team"] == 4 and sr.working_set(RR)["D"] == 41 and sr.working_set(QQ)["team"] == 2
    assert sr.team_of(128, 21) == 2 and sr.team_of(129, 21) == 1 and sr.team_of(1, 2) == 2 and sr.team_of(100, 64) == 1


def test_summary_rows_and_readers(tmp_path):
    from th_rl_amd import utils
    N, G, D = 2, 6, 5
    rs = np.random.RandomState(3)
    r = {"iters": rs.randint(0, 3, (N, G)).astype(np.int32), "sweeps": rs.randint(10, 99, (N, G)).astype(np.int32),
         "n_diff": rs.randint(0, D, (N, G)).astype(np.int32), "loss_all": rs.uniform(0, 0.1, (N, G)),
         "loss_mean": rs.uniform(0, 0.05, (N, G)), "loss_w": rs.uniform(0, 0.05, (N, G)), "gain_w": rs.uniform(0, 2, (N, G)),
         "v_w": rs.uniform(10, 20, (N, G)), "br_prob_w": rs.uniform(0, 1, (N, G)),
         "gamma": np.repeat(np.array([[0.9], [0.5]]), G, axis=1), "epsilon": np.zeros((N, G)),
         "agents": [0, 1], "T": 9, "n_prices": D}
    r["iters"][0, 2] = -1
    r["loss_all"][1, :3] = 0.0
    for f in ("loss_all", "loss_mean", "loss_w", "gain_w", "v_w", "br_prob_w"):
        r[f][0, 2] = np.nan
    ids = np.array([0, 0, 0, 1, 1, 1])
    rows = sr.summarize(r, [0, 1], ids, 2, nash=10.0, cartel=12.0)
    assert len(rows) == 6 and [x["agent"] for x in rows] == [0, 1, None, 0, 1, None]
    a0 = rows[0]
    assert a0["games"] == 3 and abs(a0["capped"] - 1 / 3) < 1e-12 and a0["br_all"] == 0.0
    assert abs(a0["exploit_mean"] - (0.1 * r["gain_w"][0, :2]).mean()) < 1e-12
    assert abs(a0["loss_all_q50"] - np.median(r["loss_all"][0, :2])) < 1e-12
    assert rows[1]["br_all"] == 1.0 and rows[1]["capped"] == 0.0
    nc = 0.1 * r["gain_w"][0] + 0.5 * r["gain_w"][1]
    assert rows[2]["solved"] == 2 and abs(rows[2]["nashconv_mean"] - nc[:2].mean()) < 1e-12
    assert abs(rows[5]["nashconv_mean"] - nc[3:].mean()) < 1e-12
    assert rows[5]["nashconv_small"] == float((nc[3:] < 0.02).mean())
    sr.save_games(str(tmp_path), r)
    back = sr.load_games(str(tmp_path))
    for f in sr.INT + sr.FLOAT + sr.WEIGHTED + ("gamma", "epsilon"):
        assert np.array_equal(back[f], r[f], equal_nan=True), f
    assert "br_policy" not in back
    desc = sr.describe(dict(sr.DEFAULTS), r, 10.0, 12.0, rows)
    assert json.loads(json.dumps(desc)) == desc
    json.dump(desc, open(tmp_path / "sampled_response.json", "w"))
    df = utils.sampled_response_summary(str(tmp_path))
    assert len(df) == 6 and df["T"][0] == 9 and "nashconv_mean" in df.columns
    # policies on a second save, then off again: the optional files go
    sr.save_games(str(tmp_path), dict(r, br_policy=np.zeros((N, G, D), np.uint16), v_opt=np.ones((N, G, D)), v_pi=np.ones((N, G, D))))
    assert sr.load_games(str(tmp_path))["v_opt"].shape == (N, G, D)
    sr.save_games(str(tmp_path), r)
    assert not (tmp_path / "sresp_v_opt.npy").exists()
