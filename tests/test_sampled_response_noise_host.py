"""Host side of the best responses to sampled play under demand noise (th_rl_amd.sampled_response.run_noise,
thrl_sampled_response_noise): the numpy mirror against an independent dense solution on the S x S chain and against closed
forms, the kernel's own source as a stand-alone host program under sanitizers, the args struct against the header, the
exported symbol, every refusal of the entry point through the library loaded without a GPU, the working-set formula at its
edge, option parsing, the summary and the readers.  No GPU."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sampled_host_checks as HC
import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import sampled_response_noise_mirror as SRNM
from sampled_mirror import AG, ENV, QQ, QR, RF, RR, SHIP
from th_rl_amd import sampled_play as sp
from th_rl_amd import sampled_response as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096                           # never dereferenced: validation fails before any launch
EVAL_TOL = 1e-12
# (config, resolution, games, seed, gamma per agent)
DENSE_CASES = {"QQ": (QQ, 8, 3, 61, [0.95, 0.9]), "QR": (QR, 8, 3, 62, [0.95, 0.9]),
               "three": (SNM.three_agents(), 8, 2, 63, [0.9, 0.95, 0.8]), "RR": (RR, 8, 1, 64, [0.9, 0.8])}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _allow(tabs, vmax, gam):
    """The rounding allowance beside a stopping bound.  A value of one sweep is the end of chains of at most W (the band
    row) + T (a state's tuples, all of them for the mixed policy) + A (the own actions) additions of products, each
    rounded to half an ulp of a partial sum that stays below max |V| / (1 - gamma) times a probability: fewer than
    W + T + 16 ulp(max |V|) per sweep, and a per-sweep error e settles at e / (1 - gamma) in the fixed point."""
    n = int(tabs["band_w"]) + int(tabs["n_tuples"]) + 16
    return n * np.spacing(vmax) / (1.0 - gam)


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_the_mirror_against_a_dense_solution(name):
    """V_pi against numpy.linalg.solve of (I - gamma P_pi) V = R_pi over the S states of the chain of normalised
    probabilities; V* against the Bellman optimality residual of the same dense model.  Tolerances: the Jacobi stopping
    bound gamma eval_tol / (1 - gamma) plus _allow's rounding allowance for V_pi; for the residual max_k Q_V*(s, k) -
    V*(s), the margin an improvement must beat plus eval_tol (the last sweep's change) plus the allowance."""
    config, res, G, seed, gammas = DENSE_CASES[name]
    kw = SRNM.make_inputs(config, res, G, seed)
    tabs = kw["tabs"]
    out = SRNM.analyse(gamma=gammas, **kw)
    assert (out["iters"] >= 0).all()
    eps = np.asarray(kw["eps"])
    for g in range(G):
        PS, _ = SRNM.state_rows(tabs, kw["probs"], np.asarray(kw["dpolicy"]), kw["nprobs"], np.asarray(kw["npolicy"]), eps, g)
        for i, gam in enumerate(gammas):
            p = float(kw["noise_prob"][g])
            Vpi, Vs, Ppi = SRNM.dense(tabs, PS, i, gam, p)
            assert np.abs(Ppi.sum(axis=1) - 1.0).max() < 1e-12          # the dense chain is a chain
            allow = _allow(tabs, np.abs(Vs).max(), gam)
            bound = gam * EVAL_TOL / (1.0 - gam)
            e_pi = np.abs(out["v_pi"][i, g] - Vpi).max()
            assert e_pi <= bound + allow, (name, g, i, e_pi, bound, allow)
            # the Bellman optimality residual of the mirror's V*, in the dense model
            V = out["v_opt"][i, g]
            resid = _bellman_residual(tabs, PS, i, gam, p, V)
            margin = 2.0 * gam * gam * EVAL_TOL / (1.0 - gam)
            assert resid <= margin + EVAL_TOL + allow, (name, g, i, resid, margin, allow)
            assert np.abs(V - Vs).max() <= (margin + EVAL_TOL) / (1.0 - gam) + allow
            assert (V >= out["v_pi"][i, g] - bound - allow).all()


def _bellman_residual(tabs, PS, i, gam, p, V):
    act = SPM.actions_of(tabs)
    N, T = act.shape
    D = int(tabs["n_prices"])
    q = 1.0 - p
    R = q * np.asarray(tabs["reward"])[i] + p * np.asarray(tabs["noise_reward"])[i]
    norm = [x / x.sum(axis=1, keepdims=True) for x in PS]
    rival = np.ones((PS[0].shape[0], T))
    for j in range(N):
        if j != i:
            rival = rival * norm[j][:, act[j]]
    cont = q * V[:D][np.asarray(tabs["row"])] + p * (np.asarray(tabs["nn"]) @ V[D:])
    U = R + gam * cont
    Q = np.stack([(rival * (act[i] == k)) @ U for k in range(PS[i].shape[1])], axis=1)
    return np.abs(Q.max(axis=1) - V).max()


def test_gamma_zero_is_the_one_period_best_response():
    kw = SRNM.make_inputs(SNM.three_agents(), 8, 2, 71)
    tabs = kw["tabs"]
    out = SRNM.analyse(gamma=0.0, **kw)
    act = SPM.actions_of(tabs)
    for g in range(2):
        PS, _ = SRNM.state_rows(tabs, kw["probs"], np.asarray(kw["dpolicy"]), kw["nprobs"], np.asarray(kw["npolicy"]), kw["eps"], g)
        p = float(kw["noise_prob"][g])
        norm = [x / x.sum(axis=1, keepdims=True) for x in PS]
        for i in range(3):
            Rn = (1.0 - p) * np.asarray(tabs["reward"])[i] + p * np.asarray(tabs["noise_reward"])[i]
            w = np.ones((PS[0].shape[0], act.shape[1]))
            for j in range(3):
                if j != i:
                    w = w * norm[j][:, act[j]]
            qv = np.stack([(w * Rn * (act[i] == k)).sum(axis=1) for k in range(PS[i].shape[1])], axis=1)
            assert np.abs(out["v_opt"][i, g] - qv.max(axis=1)).max() <= 1e-12 * np.abs(qv).max()
            assert out["sweeps"][i, g] >= 3 and out["iters"][i, g] >= 0


def test_the_best_response_fed_back_loses_nothing():
    kw = SRNM.make_inputs(QR, 8, 3, 72)
    D = int(kw["tabs"]["n_prices"])
    first = SRNM.analyse(gamma=0.9, agents=[0], **kw)
    assert (first["n_diff_prices"][0] + first["n_diff_nodes"][0] > 0).any()
    back, nback = np.asarray(kw["dpolicy"]).copy(), np.asarray(kw["npolicy"]).copy()
    back[:, 0], nback[:, 0] = first["br_policy"][0][:, :D], first["br_policy"][0][:, D:]
    e0 = kw["eps"].copy()
    e0[0] = 0.0
    again = SRNM.analyse(gamma=0.9, agents=[0], **dict(kw, dpolicy=back, npolicy=nback, eps=e0))
    assert not again["n_diff_prices"][0].any() and not again["n_diff_nodes"][0].any() and not again["iters"][0].any()
    assert (again["loss_all"][0] <= 0.9 * EVAL_TOL / 0.1 / np.abs(again["v_opt"][0]).min(axis=1) * 4).all()
    w = np.stack([SRNM.weights(kw["tabs"], kw["pi"][g], float(kw["noise_prob"][g])) for g in range(3)])
    assert np.allclose(again["br_prob_w"][0], w.sum(axis=1), rtol=1e-12)


def test_the_weights_are_a_distribution():
    """w(d) = q M(d), w(D + j) = p nu(j) with pi the chain's long-run distribution: the long-run distribution of the
    state in which a decision is made.  They add up to 1 within the rounding of S + T additions."""
    kw = SRNM.make_inputs(QR, 12, 4, 73)
    tabs = kw["tabs"]
    chain = SNM.analyse(tabs, kw["probs"], kw["dpolicy"], kw["nprobs"], kw["npolicy"], kw["eps"], kw["noise_prob"])
    assert (chain["iters"] >= 0).all()
    S, T = int(tabs["n_prices"]) + int(tabs["n_nodes"]), int(tabs["n_tuples"])
    for g in range(4):
        w = SRNM.weights(tabs, chain["pi"][g], float(kw["noise_prob"][g]))
        assert w.shape == (S,) and (w >= 0.0).all()
        assert abs(SPM._ordered_sum(w) - chain["mass"][g]) <= (S + T) * np.spacing(1.0)
        assert abs(SPM._ordered_sum(w) - 1.0) <= 1e-9            # the chain's own mass, to its tolerance
    out = SRNM.analyse(gamma=0.8, **dict(kw, pi=chain["pi"]))
    assert (out["br_prob_w"] > 0.0).all() and (out["br_prob_w"] <= 1.0 + 1e-9).all()
    assert (out["gain_w"] >= -1e-9).all()


# ------------------------------------------------------------------------------------------------ the kernel on the host
def build_check(path, sanitizer):
    HC.build_check("sampled_response_noise_check.cpp", path, sanitizer)


def run_cases(exe, d):
    """Every case of sampled_response_noise_mirror.host_cases() through the program: the return codes and the outputs."""
    res = []
    for k, (what, kw, blocks) in enumerate(SRNM.host_cases()):
        ref = SRNM.analyse(**kw)
        path = os.path.join(d, "case%d.bin" % k)
        SRNM.write_case(path, kw, ref, blocks)
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        res.append((what, p.returncode, p.stdout, ref, kw))
    return res


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
def test_the_kernels_source_on_the_host_equals_the_mirror_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sampled_response_noise_check")
    build_check(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    res = run_cases(exe, str(tmp_path))
    for what, rc, text, ref, kw in res:
        assert rc == 0 and "equal to the mirror bit for bit" in text, (what, text[-3000:])
        # the layout the program planned is the one working_set_noise states
        tabs = kw["tabs"]
        ws = sr.working_set_noise(None, tabs=tabs, n_nodes=int(tabs["n_nodes"]))
        assert "%d bytes of LDS" % ws["bytes"] in text, (what, ws, text[:300])
    # the cases are what they claim: unsolved games of each kind, three agents, D < T and S > 256
    first, capped = res[0][3], res[1][3]
    assert (first["iters"][:, 1] == -1).all() and not first["sweeps"][:, 1].any()                  # the bad epsilon
    assert (first["iters"][:, 5] == -1).all() and not first["sweeps"][:, 5].any()                  # the bad noise_prob
    assert not first["loss_all"][:, [1, 5]].any()
    assert first["iters"][1, 2] == -1 and np.isnan(first["loss_all"][1, 2]) and np.isnan(first["loss_all"][0, 4])
    assert (first["iters"][:, [0, 3, 6]] >= 0).all()
    assert (capped["iters"][1] == -1).all() and (capped["sweeps"][1] == 3).all()
    assert "N=3" in res[2][2] and "D=41 " in res[4][2] and "S=554" in res[5][2]
    assert max(r[3]["iters"].max() for r in res) >= 1
    assert max(r[3]["n_diff_prices"].max() for r in res) >= 1 and max(r[3]["n_diff_nodes"].max() for r in res) >= 1


# ------------------------------------------------------------------------------------------------ the entry point
def test_args_struct_matches_the_header():
    from th_rl_amd import _lib
    struct, cname = _lib.SampledResponseNoiseArgs, "thrl_sampled_response_noise_args"
    fields = [n for n, _ in struct._fields_]
    HC.assert_struct_matches_header(
        struct, cname, "thrl_response_noise.h",
        [("THRL_SRN_MAX_LDS", _lib.SRN_MAX_LDS), ("THRL_STAT_MAX_ITERS", _lib.STAT_MAX_ITERS), ("THRL_STAT_MAX_CELLS", _lib.STAT_MAX_CELLS),
         ("THRL_TP_MAX_TUPLES", 4096), ("THRL_EQ_MAX_ITERS", SRNM.EQ_MAX_ITERS), ("THRL_ABI_VERSION", 4)])
    assert sr.MAX_LDS == _lib.SRN_MAX_LDS == 160 * 1024 and _lib.ABI_VERSION == 4
    # thrl_sampled_response_args' fields, with the four that are split
    old = [n for n, _ in _lib.SampledResponseArgs._fields_]
    renamed = {"n_diff": ["n_diff_prices", "n_diff_nodes"], "loss_mean": ["loss_prices_mean", "loss_nodes_mean"]}
    assert [f for f in fields if f in old or any(f in v for v in renamed.values())] \
        == [x for f in old for x in renamed.get(f, [f])]
    assert set(fields) - set(old) - {x for v in renamed.values() for x in v} \
        == {"n_nodes", "band_w", "noise_prob", "noise_prob_g", "nprob", "npolicy", "band_lo", "band", "noise_reward"}


def test_the_library_exports_the_call_in_its_own_list(lib):
    from th_rl_amd import _lib
    assert _lib.RESPONSE_NOISE_SYMBOLS == ["thrl_sampled_response_noise"]
    assert _lib.RESPONSE_SYMBOLS == ["thrl_sampled_response"] and len(_lib.SYMBOLS) == 55
    assert not set(_lib.RESPONSE_NOISE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.RESPONSE_SYMBOLS))
    for name in _lib.RESPONSE_NOISE_SYMBOLS:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "thrl_response_noise.h")).read()
    assert re.findall(r"^\w[\w\s\*]*?\b(thrl_\w+)\(", header, flags=re.M) == _lib.RESPONSE_NOISE_SYMBOLS
    assert '#include "thrl_response.h"' in header
    assert lib.thrl_version() == 4


SRN_INPUTS = ("dpolicy", "npolicy", "grp_first", "grp_perm", "reward", "band_lo", "band", "noise_reward")
SRN_OUTPUTS = ("iters", "sweeps", "n_diff_prices", "n_diff_nodes", "loss_all", "loss_prices_mean", "loss_nodes_mean")
SRN_WEIGHTED = ("loss_w", "gain_w", "v_w", "br_prob_w")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    c = config or SHIP
    qt = {"agents": [dict(AG, actions=a.get("actions", 21)) for a in c["agents"]], "environment": c["environment"]}
    return _lib.cfg_from_config(qt, n_games, 0)[0]


def srn_args(**kw):
    from th_rl_amd import _lib
    a = _lib.SampledResponseNoiseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.n_nodes, a.band_w, a.agents, a.max_sweeps, a.eval_tol = 64, 441, 441, 1121, 310, 3, 100, 1e-12
    a.kind[1], a.prob[1], a.nprob[1], a.eps[0], a.gamma[0], a.gamma[1], a.noise_prob = 1, FAKE, FAKE, 0.01, 0.95, 0.995, 0.05
    for f in SRN_INPUTS + SRN_OUTPUTS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k in ("kind", "eps", "prob", "nprob", "gamma", "reserved"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


SRN_BAD = [dict(n_games=0), dict(flags=1), dict(flags=-1), dict(reserved=[1]), dict(reserved=[0, 1]), dict(agents=0),
           dict(agents=4), dict(agents=-1), dict(n_tuples=0), dict(n_tuples=440), dict(n_prices=0), dict(n_prices=442),
           dict(n_nodes=1), dict(n_nodes=0), dict(band_w=0), dict(band_w=-3),
           dict(gamma=[1.0]), dict(gamma=[0.5, -0.1]), dict(gamma=[float("nan")]), dict(max_sweeps=0), dict(max_sweeps=65537),
           dict(eval_tol=-1e-9), dict(eval_tol=float("nan")), dict(eps=[-0.1]), dict(eps=[1.5]), dict(eps=[float("nan")]),
           dict(noise_prob=0.0), dict(noise_prob=-0.1), dict(noise_prob=1.5), dict(noise_prob=float("nan")),
           dict(kind=[0, 4]), dict(kind=[-1, 0]), dict(kind=[0, 1], n_tuples=21 * 40, n_prices=21)]


def test_the_entry_point_validates_before_any_launch(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path that the host can see; none touches a device (the pointers are fake, and
    the machine of this test has no GPU to launch on)."""
    from th_rl_amd import _lib
    cfg = _cfg()
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})           # a network has at most 32
    call = lib.thrl_sampled_response_noise
    for bad in SRN_BAD:
        c = forty if bad.get("n_tuples") == 21 * 40 else cfg
        assert call(ctypes.byref(c), ctypes.byref(srn_args(**bad)), None) == -1, bad
        assert lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(srn_args(noise_prob=0.0)), None) == -1
    assert b"out of (0, 1]" in lib.thrl_last_error()
    # the gamma of an agent that is not solved and a neural agent's epsilon are not read; the per-game arrays take the
    # place of the scalars
    assert call(ctypes.byref(cfg), ctypes.byref(srn_args(agents=1, gamma=[0.5, 7.0], iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(srn_args(eps=[0.0, 7.0], iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(srn_args(gamma=[7.0], sweep_gamma=FAKE, iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(srn_args(eps=[7.0], eps_g=FAKE, iters=None)), None) == -2
    assert call(ctypes.byref(cfg), ctypes.byref(srn_args(noise_prob=7.0, noise_prob_g=FAKE, iters=None)), None) == -2
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097, n_prices=1), dict(n_nodes=_lib.STAT_MAX_CELLS + 1)):
        assert call(ctypes.byref(cfg), ctypes.byref(srn_args(**unsupported)), None) == -3, unsupported
    assert b"n_nodes=%d, at most %d" % (_lib.STAT_MAX_CELLS + 1, _lib.STAT_MAX_CELLS) in lib.thrl_last_error()
    # the working set: refused from the shape alone, before any pointer is looked at, exactly where working_set_noise says
    for (A, B), rc, nbytes in EDGE:
        ws = sr.working_set_noise(_shape(A, B))
        assert ws["bytes"] == nbytes and ws["fits"] == (rc == -2) and ws["Jn"] == 1121
        a = srn_args(n_tuples=ws["T"], n_prices=ws["D"], n_nodes=ws["Jn"], loss_all=None, prob=[None, None], dpolicy=None)
        assert call(ctypes.byref(_cfg(_shape(A, B))), ctypes.byref(a), None) == rc, (A, B, ws)
    assert b"165632 bytes of LDS" in lib.thrl_last_error()
    for null in SRN_INPUTS + SRN_OUTPUTS:
        assert call(ctypes.byref(cfg), ctypes.byref(srn_args(**{null: None})), None) == -2, null
        assert null.encode() in lib.thrl_last_error()
    for which in ("prob", "nprob"):
        assert call(ctypes.byref(cfg), ctypes.byref(srn_args(**{which: [None, None]})), None) == -2
        assert b"prob[1] / nprob[1]" in lib.thrl_last_error()
    full = {f: FAKE for f in SRN_WEIGHTED}
    for null in SRN_WEIGHTED:
        assert call(ctypes.byref(cfg), ctypes.byref(srn_args(pi=FAKE, **dict(full, **{null: None}))), None) == -2, null
        assert b"with pi" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), None, None) == -2
    assert call(None, ctypes.byref(srn_args()), None) == -2


def test_the_new_entry_point_adds_no_refusal_words():
    """thrl_api_analysis.hip's fail( format strings are recorded (tests/test_api_refusals_host.py): the new entry point
    goes through the shared helpers, and the three checks it shares with thrl_sampled_noise_chain became helpers."""
    src = open(os.path.join(ROOT, "th_rl_amd", "csrc", "thrl_api_analysis.hip")).read()
    body = src[src.index("int thrl_sampled_response_noise("):]
    body = body[:body.index("\n}\n")]
    sites = re.findall(r'\bfail\(THRL_ERR_\w+,\s*"((?:[^"\\]|\\.)*)"', body)
    assert sorted(sites) == sorted(["args is NULL", "unknown flags 0x%x", "reserved=%d must be 0"])
    for fmt in ("n_prices=%d out of [1, n_tuples=%d]", "n_nodes=%d must be >= 2 and band_w=%d >= 1", "prob[%d] / nprob[%d] is NULL"):
        assert src.count('"%s"' % fmt) == 1, fmt


# ------------------------------------------------------------------------------------------------ the working set
def _shape(A, B):
    return {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}


# the heaviest accepted and the lightest refused of QTable 20..39 x Reinforce {21, 24, 28, 32} at the default resolution
EDGE = (((33, 28), -2, 161216), ((35, 21), -3, 165632))


def test_working_set_noise_follows_the_layout():
    ws = sr.working_set_noise(SHIP)
    assert ws == dict(bytes=121024, T=441, D=441, Jn=1121, fits=True)
    # by hand for QQ at resolution 8: T = 4, D = 3, Jn = 105, S = 108, two QTable agents
    r16 = lambda x: (x + 15) & ~15
    want = 5 * r16(8 * 108) + 2 * r16(8 * 4) + 2 * r16(2 * 3) + r16(2 * 4) + 2 * r16(2 * 4) + 2 * r16(2 * 108) + 2 * r16(2 * 105) \
        + 2048 + 256
    assert sr.working_set_noise(QQ, 8) == dict(bytes=want, T=4, D=3, Jn=105, fits=True)
    best, worst = None, None
    for A in range(20, 40):
        for B in (21, 24, 28, 32):
            w = sr.working_set_noise(_shape(A, B))
            if w["fits"] and (best is None or w["bytes"] > best[1]["bytes"]):
                best = ((A, B), w)
            if not w["fits"] and (worst is None or w["bytes"] < worst[1]["bytes"]):
                worst = ((A, B), w)
    assert (best[0], best[1]["bytes"]) == (EDGE[0][0], EDGE[0][2]) and (worst[0], worst[1]["bytes"]) == (EDGE[1][0], EDGE[1][2])
    assert best[1]["bytes"] <= sr.MAX_LDS < worst[1]["bytes"]
    # n_nodes in place of a resolution; the networks' node rows are no part of it
    assert sr.working_set_noise(SHIP, n_nodes=1121)["bytes"] == 121024
    # one node more: each of the five arrays of 8 S passes a multiple of 16, the arrays of 2 S and 2 Jn do not
    assert sr.working_set_noise(SHIP, n_nodes=1122)["bytes"] - 121024 == 5 * 16
    with pytest.raises(ValueError):
        sr.working_set_noise(SHIP, 1 << 20)


# ------------------------------------------------------------------------------------------------ options and artefacts
def test_parse_options():
    noisy = dict(SHIP, environment=dict(ENV, noise_prob=0.05))
    got = sp.parse_options({"noise": True, "response": {"noise": True}}, noisy)
    assert got == dict(sp.DEFAULTS, noise=dict(sp.NOISE_DEFAULTS), response=dict(sr.DEFAULTS, noise=True))
    full = {"agents": [1], "eval_tol": 1e-10, "max_sweeps": 512, "policies": True, "noise": True}
    got = sp.parse_options({"pi": True, "noise": {"noise_prob": 0.1, "resolution": 64}, "response": full}, SHIP)
    assert got["response"] == full and got["noise"] == {"noise_prob": 0.1, "resolution": 64}
    # the pinned refusals: "response" beside "noise" without the opt-in, and the opt-in without "noise"
    for opt in ({"response": True, "noise": True}, {"response": {}, "noise": {"noise_prob": 0.1}},
                {"response": {"noise": False}, "noise": True}):
        with pytest.raises(ValueError, match="follow-up"):
            sp.parse_options(opt, noisy)
    for opt in ({"response": {"noise": True}}, {"response": {"noise": True}, "noise": None}, {"response": {"noise": True}, "noise": False}):
        with pytest.raises(ValueError, match='has no "noise"'):
            sp.parse_options(opt, noisy)
    for bad in (1, "yes", {}):
        with pytest.raises(ValueError, match="response.noise must be true or false"):
            sp.parse_options({"noise": True, "response": {"noise": bad}}, noisy)
    # the key stays only when given: every earlier parse result is what it was
    assert sp.parse_options({"response": True}, SHIP) == dict(sp.DEFAULTS, response=dict(sr.DEFAULTS))
    assert "noise" not in sr.DEFAULTS and "noise" not in sr.parse_options({"policies": True}, SHIP)
    assert sp.parse_options({"response": {"noise": False}}, SHIP)["response"] == dict(sr.DEFAULTS, noise=False)
    # the working set of the noisy mode decides: at 1,121 nodes QTable 35 x Reinforce 21 fits the noise-free call only
    big = _shape(35, 21)
    assert sr.working_set(big)["fits"] and sp.working_set(big, resolution=1024)["fits"]
    with pytest.raises(ValueError, match="working set"):
        sp.parse_options({"noise": {"noise_prob": 0.05}, "response": {"noise": True}}, big)


def test_summary_rows_and_readers(tmp_path):
    from th_rl_amd import utils
    N, G, S = 2, 6, 7
    rs = np.random.RandomState(5)
    r = {"iters": rs.randint(0, 3, (N, G)).astype(np.int32), "sweeps": rs.randint(10, 99, (N, G)).astype(np.int32),
         "n_diff_prices": rs.randint(0, 3, (N, G)).astype(np.int32), "n_diff_nodes": rs.randint(0, 4, (N, G)).astype(np.int32),
         "loss_all": rs.uniform(0, 0.1, (N, G)), "loss_prices_mean": rs.uniform(0, 0.05, (N, G)),
         "loss_nodes_mean": rs.uniform(0, 0.05, (N, G)), "loss_w": rs.uniform(0, 0.05, (N, G)), "gain_w": rs.uniform(0, 2, (N, G)),
         "v_w": rs.uniform(10, 20, (N, G)), "br_prob_w": rs.uniform(0, 1, (N, G)),
         "gamma": np.repeat(np.array([[0.9], [0.5]]), G, axis=1), "epsilon": np.zeros((N, G)), "noise_prob": np.full(G, 0.05),
         "agents": [0, 1], "T": 9, "n_prices": 3, "n_nodes": 4, "resolution": 8}
    r["iters"][0, 2] = -1
    for f in sr.NOISE_FLOAT + sr.WEIGHTED:
        r[f][0, 2] = np.nan
    ids = np.array([0, 0, 0, 1, 1, 1])
    jump = np.array([0.1, 0.3, 0.2, 0.0, 0.05, 0.01])
    rows = sr.summarize_noise(r, [0, 1], ids, 2, nash=10.0, cartel=12.0, max_jump=jump)
    plain = sr.summarize(r, [0, 1], ids, 2, nash=10.0, cartel=12.0)
    assert len(rows) == 6 and [x["agent"] for x in rows] == [0, 1, None, 0, 1, None]
    for row, old in zip(rows, plain):                        # sampled_response's rows, plus one key each
        extra = "diff_nodes_mean" if row["agent"] is not None else "max_jump_max"
        assert {k: v for k, v in row.items() if k != extra} == old and extra in row
    assert abs(rows[0]["diff_nodes_mean"] - r["n_diff_nodes"][0, :2].mean()) < 1e-12
    assert abs(rows[4]["diff_nodes_mean"] - r["n_diff_nodes"][1, 3:].mean()) < 1e-12
    assert rows[2]["max_jump_max"] == 0.3 and rows[5]["max_jump_max"] == 0.05
    assert abs(rows[0]["exploit_mean"] - (0.1 * r["gain_w"][0, :2]).mean()) < 1e-12
    assert "max_jump_max" not in sr.summarize_noise(r, [0, 1], ids, 2, 10.0, 12.0)[2]
    sr.save_games_noise(str(tmp_path), r)
    assert np.load(tmp_path / "srespn_counts.npy").shape == (4, N, G) and np.load(tmp_path / "srespn_counts.npy").dtype == np.int32
    assert np.load(tmp_path / "srespn_loss.npy").shape == (3, N, G) and np.load(tmp_path / "srespn_weighted.npy").shape == (4, N, G)
    back = sr.load_games_noise(str(tmp_path))
    for f in sr.NOISE_INT + sr.NOISE_FLOAT + sr.WEIGHTED + ("gamma", "epsilon", "noise_prob"):
        assert np.array_equal(back[f], r[f], equal_nan=True), f
    assert "br_policy" not in back and not (tmp_path / "sresp_counts.npy").exists()
    desc = sr.describe_noise(dict(sr.DEFAULTS, noise=True), r, 10.0, 12.0, rows)
    assert json.loads(json.dumps(desc)) == desc and desc["n_nodes"] == 4
    json.dump(desc, open(tmp_path / "sampled_response_noise.json", "w"))
    df = utils.sampled_response_noise_summary(str(tmp_path))
    assert len(df) == 6 and df["T"][0] == 9 and df["n_nodes"][0] == 4 and "diff_nodes_mean" in df.columns
    games = utils.sampled_response_noise_games(str(tmp_path))
    assert len(games) == G and "n_diff_nodes_1" in games.columns and "noise_prob" in games.columns
    assert np.allclose(games["nashconv"][3:], 0.1 * r["gain_w"][0, 3:] + 0.5 * r["gain_w"][1, 3:])
    # policies on a second save, then off again: the optional files go
    sr.save_games_noise(str(tmp_path), dict(r, br_policy=np.zeros((N, G, S), np.uint16), v_opt=np.ones((N, G, S)), v_pi=np.ones((N, G, S))))
    assert sr.load_games_noise(str(tmp_path))["v_opt"].shape == (N, G, S)
    sr.save_games_noise(str(tmp_path), r)
    assert not (tmp_path / "srespn_v_opt.npy").exists()
