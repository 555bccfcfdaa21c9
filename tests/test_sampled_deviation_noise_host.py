"""Host side of the deviation test of sampled play under demand noise (th_rl_amd.sampled_deviation.run_noise,
thrl_sampled_deviation_noise): the numpy mirror against an independent dense solution on T x T matrices, against
sampled_deviation_mirror at p = 0, against the noise chain's long-run profit and against the best responses of
sampled_response_noise_mirror, its exact identities, the kernel's own source as a stand-alone host program, plain and under
sanitizers, the args struct against the header, the exported symbol, every refusal of the entry point through the library
loaded without a GPU, option parsing, the working set, the summary and the readers.  No GPU."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sampled_deviation_mirror as SDM
import sampled_deviation_noise_mirror as SDNM
import sampled_host_checks as HC
import sampled_mirror as SPM
import sampled_noise_mirror as SNM
import sampled_response_noise_mirror as SRNM
from sampled_mirror import AG, ENV, RF, SHIP
from th_rl_amd import sampled_deviation as sd
from th_rl_amd import sampled_play as sp
from th_rl_amd import sampled_response as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096                           # never dereferenced: validation fails before any launch
# The rounding allowance between the two references, in units of ulp(the largest |entry| of the table an output sums: q *
# reward + p * noise_reward's bound max|reward| + max|noise_reward|, scaled, max(price) + max(noise_price); 1.0 for a
# distance, a mass or a share).  The mirror's largest observed deviation from the dense solution on DENSE_CASES over every
# deviator and DENSE_MODES was 47.0 such units (SHIP, deviator 1, K = 12, L = 1, best response, the scaled action of game 0:
# twelve steps of sums over 441 prices and 161 nodes against matrix products of normalised rows); twice that
ROUNDING_UNITS = 94.0
DENSE_CASES = ("QQ", "QQ0", "QR", "QR0", "QRA", "SHIP")
DENSE_MODES = ((12, 3, -1), (12, 1, -1), (12, 12, -1), (12, 3, 0))     # (K, L, action): the noise-free test's


def allow(scale):
    return ROUNDING_UNITS * np.spacing(float(scale))


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def _analyse(c, p, x0, **kw):
    return SDNM.analyse(c["tabs"], c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], c["eps"], p, x0, **kw)


def _rows(c, g):
    tabs = c["tabs"]
    e = c["eps"][:, g:g + 1]
    P, _, _ = SPM.rows_of(tabs, {i: p[g:g + 1] for i, p in c["probs"].items()}, c["dpolicy"][g:g + 1], e)
    Pn, _, _ = SPM.rows_of(SNM.node_tabs(tabs), {i: p[g:g + 1] for i, p in c["nprobs"].items()}, c["npolicy"][g:g + 1], e)
    return [p[0] for p in P], [p[0] for p in Pn]


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("name", DENSE_CASES)
def test_the_mirror_against_a_dense_solution(name):
    """Every period's rewards, actions, price, distance and mass, the baseline and dev_share against T x T matrices
    q * (normalised price rows) + p * (nn . normalised node rows), numpy matrix products and numpy sums.  The tolerance is
    a rounding allowance between two references only (ROUNDING_UNITS); the kernel never enters it."""
    c = SDNM.case_inputs(name)
    tabs, p, x0 = c["tabs"], c["noise_prob"], c["x0"]
    G, N = c["dpolicy"].shape[0], c["dpolicy"].shape[1]
    assert (np.asarray(tabs["nn"])[:, 0] > 0).any() == (not name.endswith("0"))      # the atom is hit / never hit
    top = lambda f: np.abs(np.asarray(tabs[f])).max()
    scale = {"reward": top("reward") + top("noise_reward"), "scaled": top("scaled"), "price": top("price") + top("noise_price")}
    worst = 0.0
    for dv in range(N):
        for K, L, action in DENSE_MODES:
            ref = _analyse(c, p, x0, deviator=dv, steps=K, dev_len=L, action=action, gamma=0.9)
            for g in range(G):
                P, Pn = _rows(c, g)
                dn = SDNM.dense(tabs, P, Pn, ref["ad"][g], x0[g], float(p[g]), dv, K, L)
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


@pytest.mark.parametrize("name", ("QQ", "QR", "QRA"))
def test_without_noise_the_mirror_is_the_noise_free_one_bit_for_bit(name):
    """p = 0 per game: q * Sd + p * Sn = Sd, Rn = reward, the price-states' best response is the noise-free one, so every
    output and row has sampled_deviation_mirror's bits; a given strategy's first D entries are the noise-free strategy."""
    c = SDNM.case_inputs(name)
    tabs, x0 = c["tabs"], c["x0"]
    G, N, D, Jn = c["dpolicy"].shape[0], c["dpolicy"].shape[1], int(tabs["n_prices"]), int(tabs["n_nodes"])
    rs = np.random.RandomState(11)
    for dv in range(N):
        A = int(tabs["n_actions"][dv])
        devpol = rs.randint(0, A + 2, (G, D + Jn)).astype(np.uint16)
        for kw in (dict(steps=12, dev_len=3, action=-1, gamma=0.9), dict(steps=6, dev_len=1, action=A - 1, gamma=rs.uniform(0, 1, G)),
                   dict(steps=5, dev_len=5, action=-1, dev_policy=devpol, gamma=1.0)):
            got = _analyse(c, np.zeros(G), x0, deviator=dv, **kw)
            if "dev_policy" in kw:
                kw = dict(kw, dev_policy=devpol[:, :D])
            want = SDM.analyse(tabs, c["probs"], c["dpolicy"], c["eps"], x0, deviator=dv, **kw)
            for f in SDM.AGENT + SDM.FLOAT + SDM.INT + SDM.ROWS_AGENT + SDM.ROWS_GAME:
                assert np.array_equal(got[f], want[f]), (name, dv, f)
            assert np.array_equal(got["ad"][:, :D], want["ad"])


@pytest.mark.parametrize("name", ("QR", "QRA"))
def test_the_baseline_is_the_noise_chains_long_run_profit_bit_for_bit(name):
    c = SDNM.case_inputs(name)
    st = SNM.analyse(c["tabs"], c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], c["eps"], c["noise_prob"], max_iters=40)
    out = _analyse(c, c["noise_prob"], st["pi"], deviator=1, steps=1, dev_len=1)
    assert np.array_equal(out["base_reward"], st["samp_reward"]) and np.array_equal(out["base_action"], st["samp_action"])
    assert np.array_equal(out["base_price"], st["samp_price"]) and (st["iters"] > 0).all()


def test_the_own_greedy_strategy_of_an_exact_table_is_no_deviation():
    """A QTable deviator at eps 0 "deviated" to its own greedy strategy on every state, prices and nodes: dev_share == 0.0
    exactly and every row equals plain propagation bit for bit (hi = 1.0 and lo = 0.0 are the replaced row's values), so
    the response is zero throughout, whatever the length of the deviation."""
    c = dict(SDNM.case_inputs("QRA"))
    tabs, x0, p = c["tabs"], c["x0"], c["noise_prob"]
    q = [i for i, k in enumerate(tabs["kinds"]) if k == "QTable"][0]
    A = int(tabs["n_actions"][q])
    c["eps"] = c["eps"].copy()
    c["eps"][q] = 0.0
    own = np.concatenate([np.minimum(c["dpolicy"][:, q].astype(np.int64), A - 1),
                          np.minimum(c["npolicy"][:, q].astype(np.int64), A - 1)], axis=1).astype(np.uint16)
    plain = _analyse(c, p, x0, deviator=q, steps=8, dev_len=1, action=-1, gamma=0.9)
    for L in (1, 8):
        out = _analyse(c, p, x0, deviator=q, steps=8, dev_len=L, dev_policy=own, gamma=0.9)
        assert (out["dev_share"] == 0.0).all()
        # the first period's distribution is the plain step's: the rows from tau >= 1 of a one-period deviation are plain
        # propagation of it, so a deviation of any length to the own strategy gives the rows of any other
        one = _analyse(c, p, x0, deviator=q, steps=8, dev_len=1, dev_policy=own, gamma=0.9)
        for f in SDM.ROWS_AGENT + SDM.ROWS_GAME:
            assert np.array_equal(out[f], one[f]), f
    P, Z, _ = SPM.rows_of(tabs, c["probs"], c["dpolicy"], c["eps"])
    Pn, Zn, _ = SPM.rows_of(SNM.node_tabs(tabs), c["nprobs"], c["npolicy"], c["eps"])
    act = SPM.actions_of(tabs)
    x = x0
    for tau in range(8):
        x = SDNM.step(tabs, P, Z, Pn, Zn, act, x, p, 1.0 - p)
        rew, sca, price, dist, _ = SDNM.outcome(tabs, x, x0, p, 1.0 - p)
        assert np.array_equal(one["reward_rows"][tau], rew) and np.array_equal(one["action_rows"][tau], sca)
        assert np.array_equal(one["price_rows"][tau], price) and np.array_equal(one["dist_rows"][tau], dist)
    assert (plain["dev_share"] >= 0.0).all()
    # from the chain's long-run distribution the response to that "deviation" is zero to the chain's own tolerance
    st = SNM.analyse(tabs, c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], c["eps"], p, tol=1e-14)
    flat = _analyse(c, p, st["pi"], deviator=q, steps=8, dev_len=8, dev_policy=own, gamma=0.9)
    T = int(tabs["n_tuples"])
    assert (flat["dev_share"] == 0.0).all() and (flat["dist_rows"] <= 8 * 2 * T * st["change"][None, :] + 1e-15).all()
    # against a mixing rival the same strategy does deviate from an exploring table
    c["eps"][q] = 0.1
    assert (_analyse(c, p, x0, deviator=q, steps=2, dev_len=1, dev_policy=own)["dev_share"] > 0.0).all()


@pytest.mark.parametrize("name", ("QQ", "QRA", "SHIP"))
def test_a_lasting_deviation_to_the_best_reply_earns_its_value(name):
    """ad = sampled_response_noise_mirror's sigma* for the deviator, L = K = 48, gamma = 0.5.  From any x_0 the state in
    which the first decision is made has the distribution w(d) = q M_0(d), w(D + j) = p nu_0(j), so sum_tau gamma^tau
    r_delta(tau) = sum_s w(s) V*(s).  The tolerance is the sum of three terms, as in the noise-free test: the truncation of
    the series after K periods, gamma^K rmax / (1 - gamma); the Jacobi stopping bound of V*, gamma eval_tol / (1 - gamma);
    and the rounding allowance at the scale of a value, rmax / (1 - gamma); rmax = max|reward| + max|noise_reward|.  From
    the chain's long-run distribution pi the same sum less the baseline's, the gain, is sum_s w(s) (V*(s) - V_pi(s)): there
    the plain chain moves x_0 by at most delta = 2 T change in L1 per step (m' - m = (s - m) / 2), so period tau's plain
    reward is within rmax (tau + 1) delta of the baseline and V_pi's sum within rmax delta / (1 - gamma)^2 of the
    baseline's; V_pi adds its own truncation and Jacobi terms."""
    c = SDNM.case_inputs(name)
    tabs = c["tabs"]
    G, N, D = c["dpolicy"].shape[0], c["dpolicy"].shape[1], int(tabs["n_prices"])
    K, gam, eval_tol = 48, 0.5, 1e-12
    p = np.maximum(c["noise_prob"], 0.01)                # the best responses under noise need p > 0
    st = SNM.analyse(tabs, c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], c["eps"], p, tol=1e-13)
    assert (st["iters"] > 0).all()
    for dv in range(N):
        rmax = np.abs(np.asarray(tabs["reward"])[dv]).max() + np.abs(np.asarray(tabs["noise_reward"])[dv]).max()
        truncation = gam ** K * rmax / (1.0 - gam)
        jacobi = gam * eval_tol / (1.0 - gam)
        rounding = allow(rmax / (1.0 - gam))
        br = SRNM.analyse(tabs, c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], c["eps"], gam, p, agents=[dv], eval_tol=eval_tol)
        assert (br["iters"][dv] >= 0).all()
        for x0, stationary in ((c["x0"], False), (st["pi"], True)):
            out = _analyse(c, p, x0, deviator=dv, steps=K, dev_len=K, dev_policy=br["br_policy"][dv], gamma=gam)
            w = np.stack([SRNM.weights(tabs, x0[g], float(p[g])) for g in range(G)])
            got = (out["reward_rows"][:, dv, :] * (gam ** np.arange(K))[:, None]).sum(axis=0)
            want = (w * br["v_opt"][dv]).sum(axis=1)
            assert np.abs(got - want).max() <= truncation + jacobi + rounding, (name, dv, np.abs(got - want).max())
            base = out["base_reward"][dv] * (gam ** np.arange(K)).sum()
            assert np.abs(out["gain"] - (got - base)).max() <= K * allow(rmax)
            assert np.array_equal(out["gain"], out["gain_dev"])
            if stationary:
                delta = 2.0 * int(tabs["n_tuples"]) * st["change"]
                want = (w * (br["v_opt"][dv] - br["v_pi"][dv])).sum(axis=1)
                tol = 2.0 * (truncation + jacobi + rounding) + rmax * delta / (1.0 - gam) ** 2 + K * allow(rmax)
                assert (np.abs(out["gain"] - want) <= tol).all(), (name, dv, np.abs(out["gain"] - want).max())
                assert (out["gain"] >= -tol).all()


# ------------------------------------------------------------------------------------------------ the kernel on the host
def build_check(path, sanitizer):
    HC.build_check("sampled_deviation_noise_check.cpp", path, sanitizer)


RR5 = SNM.two_agents("Reinforce", 5, "Reinforce", 5)


def host_cases():
    """(what, inputs, per-game noise, epsilon, analyse()'s and write_case()'s shared arguments, rows, blocks): both kinds
    of deviator, three agents, a node count that is no multiple of the tile (every case) and one past two tiles, row ranges,
    two blocks and three, a bad epsilon and a bad noise_prob beside solved games, noise at exactly 0 and 1."""
    out = []
    for name in ("QQ", "QR", "QRA"):
        c = SDNM.case_inputs(name)
        tabs = c["tabs"]
        G, N, S = c["dpolicy"].shape[0], c["dpolicy"].shape[1], int(tabs["n_prices"]) + int(tabs["n_nodes"])
        rs = np.random.RandomState(len(name))
        p = c["noise_prob"].copy()
        p[0], p[-1] = 0.0, 1.0
        bad_e, bad_p = c["eps"].copy(), p.copy()
        bad_e[0, 1] = np.nan                             # agent 0 is a QTable agent in QQ and QR: game 1 is not solved
        bad_p[1] = -0.25
        q = [i for i, k in enumerate(tabs["kinds"]) if k == "QTable"][0]
        if q != 0:
            bad_e[0, 1], bad_e[q, 1] = c["eps"][0, 1], np.nan
        out.append(("%s best response, a bad epsilon" % name, c, p, bad_e,
                    dict(deviator=N - 1, steps=12, dev_len=3, action=-1, gamma=0.9), (0, None), 2))
        out.append(("%s a fixed action, per-game gamma, the second row chunk, a bad noise_prob" % name, c, bad_p, c["eps"],
                    dict(deviator=0, steps=12, dev_len=1, action=1, gamma=rs.uniform(0.0, 1.0, G)), (5, 7), 3))
        A = int(tabs["n_actions"][N - 1])
        devpol = rs.randint(0, A + 2, (G, S)).astype(np.uint16)         # entries at and above A: clamped
        out.append(("%s a given strategy while all steps last, scalars" % name, c, 0.05, c["eps"][:, 0].copy(),
                    dict(deviator=N - 1, steps=5, dev_len=5, action=-1, dev_policy=devpol, gamma=1.0), (0, None), 2))
        out.append(("%s one step" % name, c, p, c["eps"], dict(deviator=0, steps=1, dev_len=1, action=-1, gamma=0.0), (0, None), 2))
    # two networks past two tiles of nodes: the deviator's replaced node row and the best-response pass cross tile edges
    c = dict(SNM.make_inputs(RR5, 2 * SDNM.TILE, 3, 91))
    c["x0"] = np.random.RandomState(92).dirichlet(np.ones(25), 3)
    assert c["tabs"]["n_nodes"] == 2 * SDNM.TILE + 1
    for dv in (0, 1):
        out.append(("RR5 deviator %d" % dv, c, c["noise_prob"], c["eps"], dict(deviator=dv, steps=6, dev_len=2, action=-1, gamma=0.9),
                    (0, None), 2))
    return out


def run_cases(exe, d):
    res = []
    for k, (what, c, p, eps, kw, (rb, rc), blocks) in enumerate(host_cases()):
        ref = SDNM.analyse(c["tabs"], c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], eps, p, c["x0"], **kw)
        path = os.path.join(d, "case%d.bin" % k)
        SDNM.write_case(path, c["tabs"], c["probs"], c["dpolicy"], c["nprobs"], c["npolicy"], eps, p, c["x0"], ref, blocks,
                        row_begin=rb, row_count=rc, **kw)
        r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
        res.append((what, r.returncode, r.stdout, ref, c, eps, p))
    return res


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
@pytest.mark.parametrize("sanitizer", ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitizers"))
def test_the_kernels_source_on_the_host_equals_the_mirror(tmp_path, sanitizer):
    exe = str(tmp_path / "sampled_deviation_noise_check")
    build_check(exe, sanitizer)
    unsolved = 0
    for what, rc, text, ref, c, eps, p in run_cases(exe, str(tmp_path)):
        assert rc == 0 and "equal to the mirror bit for bit" in text, (what, text[-3000:])
        tabs = c["tabs"]
        ws = sd.working_set_noise(None, tabs=tabs, n_nodes=int(tabs["n_nodes"]))     # the layout the program planned
        assert "%d bytes of LDS" % ws["bytes"] in text, (what, ws, text[:300])
        assert int(tabs["n_nodes"]) % SDNM.TILE != 0
        bad = (np.ndim(eps) == 2 and np.isnan(eps).any()) or (np.ndim(p) == 1 and (np.asarray(p) < 0).any())
        if bad:                                          # the case is what it claims: an unsolved game beside solved ones
            assert ref["low_step"][1] == -1 and not ref["reward_rows"][:, :, 1].any() and ref["reward_rows"][:, :, 0].all()
            unsolved += 1
    assert unsolved == 6


# ------------------------------------------------------------------------------------------------ the entry point
def test_args_struct_matches_the_header():
    from th_rl_amd import _lib
    HC.assert_struct_matches_header(
        _lib.SampledDeviationNoiseArgs, "thrl_sampled_deviation_noise_args", "thrl_sampled_deviation_noise.h",
        [("THRL_SDN_MAX_LDS", _lib.SDN_MAX_LDS), ("THRL_SDN_POLICY", _lib.SDN_POLICY), ("THRL_TP_MAX_TUPLES", 4096),
         ("THRL_DEV_MAX_STEPS", _lib.DEV_MAX_STEPS), ("THRL_STAT_MAX_CELLS", _lib.STAT_MAX_CELLS), ("THRL_SPN_TILE", SDNM.TILE),
         ("THRL_ABI_VERSION", 4)])
    assert sd.MAX_LDS == _lib.SDN_MAX_LDS == 160 * 1024 and _lib.SDN_POLICY == _lib.SD_POLICY and _lib.ABI_VERSION == 4


def test_the_library_exports_the_call_beside_the_others(lib):
    from th_rl_amd import _lib
    assert _lib.SAMPLED_DEVIATION_NOISE_SYMBOLS == ["thrl_sampled_deviation_noise"]
    others = _lib.SYMBOLS + _lib.RESPONSE_SYMBOLS + _lib.RESPONSE_NOISE_SYMBOLS + _lib.SAMPLED_DEVIATION_SYMBOLS
    assert not set(_lib.SAMPLED_DEVIATION_NOISE_SYMBOLS) & set(others) and len(_lib.SYMBOLS) == 55
    assert hasattr(lib, "thrl_sampled_deviation_noise")
    header = open(os.path.join(ROOT, "include", "thrl_sampled_deviation_noise.h")).read()
    assert re.findall(r"^\w[\w\s\*]*?\b(thrl_\w+)\(", header, flags=re.M) == _lib.SAMPLED_DEVIATION_NOISE_SYMBOLS
    assert "p = 0" in header and "bits of thrl_sampled_deviation" in header      # the rule for p = 0 is stated
    assert lib.thrl_version() == 4
    old = open(os.path.join(ROOT, "include", "thrl_sampled_deviation.h")).read()
    assert "thrl_sampled_deviation_noise.h" in old and "Noise-free play only" not in old


SDN_TABLES = ("dpolicy", "npolicy", "grp_first", "grp_perm", "reward", "scaled", "price", "band_lo", "band", "noise_price",
              "noise_reward", "weights")
SDN_OUTPUTS = ("base_reward", "base_action", "base_price", "dev_share", "gain", "gain_dev", "low", "low_step", "ret_step", "dist",
               "mass")


def _cfg(config=None, n_games=64):
    from th_rl_amd import _lib
    c = config or SHIP
    qt = {"agents": [dict(AG, actions=a.get("actions", 21)) for a in c["agents"]], "environment": c["environment"]}
    return _lib.cfg_from_config(qt, n_games, 0)[0]


def sdn_args(**kw):
    from th_rl_amd import _lib
    a = _lib.SampledDeviationNoiseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.deviator, a.dev_len, a.n_steps, a.dev_action = 64, 441, 441, 1, 1, 32, -1
    a.n_nodes, a.band_w, a.noise_prob = 1121, 338, 0.05
    a.kind[1], a.prob[1], a.nprob[1], a.eps[0], a.gamma, a.ret_tol = 1, FAKE, FAKE, 0.01, 0.95, 1e-6
    for f in SDN_TABLES + SDN_OUTPUTS:
        setattr(a, f, FAKE)
    for k, v in kw.items():
        if k in ("kind", "eps", "prob", "nprob", "reserved"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


NAN = float("nan")
SDN_BAD = [dict(n_games=0), dict(flags=2), dict(flags=-1), dict(reserved=[1]), dict(reserved=[0, 1]), dict(kind=[0, 4]),
           dict(kind=[-1, 0]), dict(kind=[0, 1], n_tuples=21 * 40, n_prices=21), dict(n_tuples=0), dict(n_tuples=440),
           dict(n_prices=0), dict(n_prices=442), dict(n_nodes=1), dict(n_nodes=0), dict(band_w=0), dict(deviator=-1), dict(deviator=2),
           dict(dev_len=0), dict(n_steps=0), dict(dev_len=33), dict(n_steps=1 << 30), dict(dev_action=-2), dict(dev_action=21),
           dict(flags=1, dev_action=0), dict(flags=1, dev_action=-2), dict(row_begin=-1), dict(row_count=-1),
           dict(row_begin=30, row_count=3), dict(ret_tol=-1e-9), dict(ret_tol=NAN), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=NAN),
           dict(eps=[-0.1]), dict(eps=[1.5]), dict(eps=[NAN]), dict(noise_prob=-0.01), dict(noise_prob=1.01), dict(noise_prob=NAN)]


def _shape(A, B):
    return {"agents": [dict(AG, actions=A), dict(RF, actions=B)], "environment": dict(ENV)}


# the heaviest accepted and the lightest refused of QTable 20..39 x Reinforce {21, 24, 28, 32} at the default resolution
EDGE = (((27, 32), -2, 163696), ((35, 28), -3, 164544))


def test_the_entry_point_validates_before_any_launch(lib):
    """Every BAD_CONFIG / UNSUPPORTED / NULL path that the host can see, with its code; none touches a device."""
    from th_rl_amd import _lib
    cfg = _cfg()
    forty = _cfg({"agents": [dict(AG), dict(AG, actions=40)], "environment": dict(ENV)})           # a network has at most 32
    call = lib.thrl_sampled_deviation_noise
    assert (1 << 30) > _lib.DEV_MAX_STEPS
    for bad in SDN_BAD:
        c = forty if bad.get("n_tuples") == 21 * 40 else cfg
        assert call(ctypes.byref(c), ctypes.byref(sdn_args(**bad)), None) == -1, bad
        assert lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(flags=1, dev_action=3)), None) == -1
    assert b"dev_action=3" in lib.thrl_last_error() and b"[0,0)" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(noise_prob=1.5)), None) == -1 and b"out of [0, 1]" in lib.thrl_last_error()
    # both ends of gamma's and of noise_prob's range are allowed; a neural agent's epsilon is not read; the per-game arrays
    # take the place of the scalars: each of these passes every check of the arguments and stops at a missing pointer
    for fine in (dict(gamma=0.0), dict(gamma=1.0), dict(noise_prob=0.0), dict(noise_prob=1.0), dict(eps=[0.0, 7.0]),
                 dict(gamma=7.0, sweep_gamma=FAKE), dict(eps=[7.0], eps_g=FAKE), dict(noise_prob=7.0, noise_prob_g=FAKE),
                 dict(dev_action=20, deviator=0), dict(row_begin=29, row_count=3), dict(flags=1, dev_policy=FAKE), dict(dev_len=32),
                 dict(n_nodes=2, band_w=1)):
        assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(mass=None, **fine)), None) == -2, fine
    for unsupported in (dict(kind=[0, 3]), dict(n_tuples=4097, n_prices=1), dict(n_nodes=_lib.STAT_MAX_CELLS + 1)):
        assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(**unsupported)), None) == -3, unsupported
    assert b"n_nodes=" in lib.thrl_last_error()
    # the working set: refused from the shape alone, before any pointer is looked at, exactly where working_set_noise says
    for (A, B), rc, nbytes in EDGE:
        ws = sd.working_set_noise(_shape(A, B))
        assert ws["bytes"] == nbytes and ws["fits"] == (rc == -2)
        a = sdn_args(n_tuples=ws["T"], n_prices=ws["D"], n_nodes=ws["Jn"], gain=None)
        assert call(ctypes.byref(_cfg(_shape(A, B))), ctypes.byref(a), None) == rc, (A, B, ws)
    assert ("%d bytes of LDS" % EDGE[1][2]).encode() in lib.thrl_last_error()
    for null in SDN_TABLES + SDN_OUTPUTS:
        assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(**{null: None})), None) == -2, null
        assert null.encode() in lib.thrl_last_error()
    for rows in ("prob", "nprob"):
        assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(**{rows: [None, None]})), None) == -2
        assert b"prob[1] / nprob[1]" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), ctypes.byref(sdn_args(flags=1)), None) == -2 and b"dev_policy" in lib.thrl_last_error()
    assert call(ctypes.byref(cfg), None, None) == -2
    assert call(None, ctypes.byref(sdn_args()), None) == -2


def test_the_new_entry_point_adds_no_refusal_words():
    """thrl_api_analysis.hip's fail( format strings are recorded (tests/test_api_refusals_host.py): the new entry point
    words its refusals through the shared helpers and the forms that were there, and the check of a noise probability in
    [0, 1] that it shares with thrl_sampled_noise_chain became a helper, its words kept once."""
    src = open(os.path.join(ROOT, "th_rl_amd", "csrc", "thrl_api_analysis.hip")).read()
    body = src[src.index("int thrl_sampled_deviation_noise("):]
    body = body[:body.index("\n}\n")]
    sites = re.findall(r'\bfail\(THRL_ERR_\w+,\s*"((?:[^"\\]|\\.)*)"', body)
    assert sorted(sites) == sorted(["args is NULL", "unknown flags 0x%x", "reserved=%d must be 0"])
    before = src[:src.index("int thrl_sampled_deviation_noise(")]
    for fmt in sites:
        assert '"%s"' % fmt in before, fmt
    for fmt in ("noise_prob=%g out of [0, 1]", "n_nodes=%d must be >= 2 and band_w=%d >= 1", "prob[%d] / nprob[%d] is NULL"):
        assert src.count('"%s"' % fmt) == 1, fmt


# ------------------------------------------------------------------------------------------------ options and artefacts
OLD_OPTIONS = [True, {}, {"pi": True}, {"epsilon": 0.1, "start": "state"}, {"epsilon": [0.1, 0.2], "tol": 1e-9, "max_iters": 100},
               {"noise": True}, {"noise": {"noise_prob": 0.1, "resolution": 64}, "start": "reset"}, {"noise": None},
               {"response": True}, {"response": {"agents": [1], "policies": True}, "pi": True},
               {"noise": {"noise_prob": 0.1}, "response": {"noise": True}}, {"deviation": True},
               {"deviation": {"agents": [1, 0, 1], "steps": 16, "dev_len": 4, "action": 3, "ret_tol": 1e-5}, "response": True},
               {"deviation": {"action": "best_reply"}, "noise": None}]
# what they parsed to on the parent commit
OLD_PARSED = [{}, {}, {"pi": True}, {"epsilon": 0.1, "start": "state"}, {"epsilon": [0.1, 0.2], "tol": 1e-9, "max_iters": 100},
              {"noise": {"noise_prob": None, "resolution": 1024}}, {"noise": {"noise_prob": 0.1, "resolution": 64}, "start": "reset"}, {},
              {"response": dict(sr.DEFAULTS)}, {"response": dict(sr.DEFAULTS, agents=[1], policies=True), "pi": True},
              {"noise": {"noise_prob": 0.1, "resolution": 1024}, "response": dict(sr.DEFAULTS, noise=True)},
              {"deviation": dict(sd.DEFAULTS, agents=[0, 1])},
              {"deviation": dict(agents=[0, 1], steps=16, dev_len=4, action=3, ret_tol=1e-5), "response": dict(sr.DEFAULTS)},
              {"deviation": dict(sd.DEFAULTS, agents=[0, 1], action="best_reply")}]


def test_parse_options():
    noisy = dict(SHIP, environment=dict(ENV, noise_prob=0.05))
    for opt, want in zip(OLD_OPTIONS, OLD_PARSED):       # every option dict that parsed before parses to what it did
        c = noisy if isinstance(opt, dict) and opt.get("noise") is True else SHIP
        assert sp.parse_options(opt, c) == dict(sp.DEFAULTS, **want), opt
    # the opt-in follows "response": at sampled_play's own noise_prob and resolution
    noise = {"noise_prob": 0.1, "resolution": 64}
    got = sp.parse_options({"noise": noise, "deviation": {"noise": True}}, SHIP)
    assert got == dict(sp.DEFAULTS, noise=noise, deviation=dict(sd.DEFAULTS, agents=[0, 1], noise=True))
    got = sp.parse_options({"noise": True, "deviation": {"noise": True, "agents": [1], "action": "best_reply", "steps": 8}}, noisy)
    assert got["deviation"] == dict(sd.DEFAULTS, agents=[1], action="best_reply", steps=8, noise=True)
    assert got["noise"] == {"noise_prob": None, "resolution": 1024}
    # "noise": false inside the key is the noise-free test and stays in the result
    assert sp.parse_options({"deviation": {"noise": False}}, SHIP)["deviation"] == dict(sd.DEFAULTS, agents=[0, 1], noise=False)
    # beside "noise" without the opt-in: refused, and the message still says what to do
    for opt in ({"deviation": True, "noise": True}, {"deviation": {}, "noise": {"noise_prob": 0.1}},
                {"deviation": {"noise": False}, "noise": True}, {"deviation": {"steps": 4}, "noise": True}):
        with pytest.raises(ValueError, match="follow-up.*\"noise\": true inside \"deviation\""):
            sp.parse_options(opt, noisy)
    # the opt-in without sampled_play's "noise": refused
    for opt in ({"deviation": {"noise": True}}, {"deviation": {"noise": True}, "noise": None}, {"deviation": {"noise": True}, "noise": False}):
        with pytest.raises(ValueError, match="training.sampled_play has no \"noise\""):
            sp.parse_options(opt, SHIP)
    for bad in ({"noise": 1}, {"noise": "yes"}, {"noise": True, "steps": 0}, {"noise": True, "action": 21}, {"noise": True, "tol": 0.1}):
        with pytest.raises(ValueError):
            sp.parse_options({"noise": noise, "deviation": bad}, SHIP)
    # the working sets: the test's own, and with "best_reply" the best responses' under noise (121,024 bytes for SHIP fit;
    # QTable 20 x Reinforce 32 fits the test with 146,400 bytes, the best responses take 179,408, more than a CU's LDS)
    ws, wr = sd.working_set_noise(_shape(20, 32)), sr.working_set_noise(_shape(20, 32))
    assert (ws["bytes"], ws["fits"], wr["bytes"], wr["fits"]) == (146400, True, 179408, False)
    assert sd.parse_options({"noise": True}, _shape(20, 32), noise=dict(noise, resolution=1024))["noise"] is True
    with pytest.raises(ValueError, match="best_reply.*working set is %d bytes" % wr["bytes"]):
        sd.parse_options({"noise": True, "action": "best_reply"}, _shape(20, 32), noise=dict(noise, resolution=1024))
    with pytest.raises(ValueError, match="under noise a game's working set is %d bytes" % EDGE[1][2]):
        sd.parse_options({"noise": True}, _shape(*EDGE[1][0]), noise=dict(noise, resolution=1024))


def test_working_set_noise_follows_the_layout():
    ws = sd.working_set_noise(SHIP)
    assert ws == dict(bytes=86416, T=441, D=441, Jn=1121, fits=True)
    r16 = lambda x: (x + 15) // 16 * 16
    for config, res in ((SDNM.CASES["QQ"][0], 0), (SDNM.CASES["QRA"][0], 8), (RR5, 2 * SDNM.TILE), (SHIP, 64), (SHIP, 1024)):
        ws, base = sd.working_set_noise(config, res), sp.working_set(config, resolution=res)
        assert ws["Jn"] == base["Jn"] == sp.n_nodes_of(config, res)
        assert ws["bytes"] == base["bytes"] + r16(2 * (ws["D"] + ws["Jn"])) + r16(8 * ws["D"]) + 512
    # by hand for QQ at resolution 8: T = 4, D = 3, two QTable agents
    Jn = sp.n_nodes_of(SDNM.CASES["QQ"][0], 8)
    chain = 2 * r16(32) + 2 * r16(24) + 2 * r16(6) + r16(8) + r16(8) + r16(512 * 6) + 256 + r16(8 * Jn) + 2 * r16(2 * Jn)
    assert sd.working_set_noise(SDNM.CASES["QQ"][0], 8)["bytes"] == chain + r16(2 * (3 + Jn)) + r16(24) + 512
    # the edge of the plan: the heaviest accepted and the lightest refused of the scanned shapes
    sizes = {(A, B): sd.working_set_noise(_shape(A, B)) for A in range(20, 40) for B in (21, 24, 28, 32)}
    fit = max((w["bytes"], k) for k, w in sizes.items() if w["fits"])
    out = min((w["bytes"], k) for k, w in sizes.items() if not w["fits"])
    assert (fit[1], fit[0]) == (EDGE[0][0], EDGE[0][2]) and (out[1], out[0]) == (EDGE[1][0], EDGE[1][2])
    assert fit[0] <= sd.MAX_LDS < out[0]


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
                 solved=np.array([True, True, False, True, True, True]), noise_prob=np.full(G, 0.05),
                 max_jump=np.array([0.1, 0.3, 0.9, 0.2, 0.05, 0.4]))
        r["dev_share"] = np.abs(r["dev_share"])
        games[d] = r
    ids = np.array([0, 0, 0, 1, 1, 1])
    rows = sd.summarize_noise(games, ids, 2, [0, 1])
    plain = sd.summarize(games, ids, 2, [0, 1])
    assert [(x["group"], x["deviator"]) for x in rows] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for a, b in zip(rows, plain):                        # sampled_deviation_summary's columns plus max_jump_max
        assert list(a) == list(b) + ["max_jump_max"] and all(a[k] == b[k] or (a[k] is None and b[k] is None) for k in b)
    assert rows[0]["max_jump_max"] == 0.9 and rows[3]["max_jump_max"] == 0.4      # over the group's games, solved or not
    assert sd.solved(np.zeros((2, 4)), ["QTable", "Reinforce"], np.array([0.0, 1.0, np.nan, 1.5])).tolist() == [True, True, False, False]
    for d in (0, 1):
        sd.save_games(str(tmp_path), d, games[d], sd.NOISE_PREFIX)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("sdev") and not f.startswith("sdevn")]
    for d in (0, 1):
        back = sd.load_games(str(tmp_path), d, sd.NOISE_PREFIX)
        for f in sd.NOISE_PER_GAME:
            assert np.array_equal(back[f], games[d][f]), f
    with pytest.raises(KeyError, match=r"training\.sampled_play\.deviation with \"noise\""):
        utils.sampled_deviation_noise_summary(str(tmp_path))
    r = dict(games[0], T=9, n_prices=5, n_nodes=70, resolution=64)
    desc = sd.describe_noise(dict(sd.DEFAULTS, agents=[0, 1], noise=True), r, rows)
    assert json.loads(json.dumps(desc)) == desc
    json.dump(desc, open(tmp_path / "sampled_deviation_noise.json", "w"))
    df = utils.sampled_deviation_noise_summary(str(tmp_path))
    assert len(df) == 4 and df["T"][0] == 9 and df["n_nodes"][0] == 70 and df["resolution"][0] == 64
    assert "gain_q50" in df.columns and df["max_jump_max"][0] == 0.9
    gm = utils.sampled_deviation_noise_games(str(tmp_path), 1)
    assert len(gm) == G and np.array_equal(gm["gain"], games[1]["gain"]) and np.array_equal(gm["solved"], games[1]["solved"])
    assert np.array_equal(gm["noise_prob"], games[1]["noise_prob"]) and np.array_equal(gm["max_jump"], games[1]["max_jump"])
    assert np.array_equal(gm["base_reward_1"], games[1]["base_reward"][1]) and list(gm.index) == list(range(G))
    with pytest.raises(KeyError):                        # the noise-free readers see no noise-free run here
        utils.sampled_deviation_summary(str(tmp_path))
    json.dump(dict(desc, options=dict(desc["options"], agents=[0])), open(tmp_path / "sampled_deviation_noise.json", "w"))
    with pytest.raises(KeyError, match="deviator 1 was not analysed"):
        utils.sampled_deviation_noise_games(str(tmp_path), 1)
