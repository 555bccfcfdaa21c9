"""Host side of the limit table (limits_table.py): every case sits exactly on the limit it is named after, by a numpy
restatement of the plans' window / cycle / tuple-count / action-word / LDS arithmetic; the library's own selection
(thrl_select_kernel, loaded without a GPU) agrees; the table names every NO(...) reason the four plans have in the
source; the refusals that no configuration can reach are proved unreachable by enumeration; and the CPU oracle runs
every accepted all-QTable case for one training cycle with the visit count the cycle implies.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import limits_table as LT
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "th_rl_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("case", LT.CASES, ids=[c["id"] for c in LT.CASES])
def test_case_sits_on_its_limit(case):
    m = LT.measure(case)
    for k, want in case["expect"].items():
        assert m[k] == want, "%s: %s is %r, the table says %r" % (case["id"], k, m[k], want)


def test_limits_named_by_the_table():
    """The figures the issue states, spelled out: a failure here names the limit that moved."""
    m = {c["id"]: LT.measure(c) for c in LT.CASES}
    assert m["wave-rows-126"]["win_rows"] + 2 == 128 and m["wave-rows-127"]["win_rows"] + 2 == 129
    assert m["wave-rows-126-A32-f64"]["wave_game_lds"] == 64 * 1024
    assert m["wave-256-transitions"]["transitions"] == 256 < m["wave-320-transitions"]["transitions"]
    assert m["wave-epk32-T7"]["epk"] == m["wave-epk32-T1"]["epk"] == 32 and m["wave-epk33-T7"]["epk"] == 33
    assert m["wave-epk33-T7"]["transitions"] <= 256                  # refused for its episodes, not its transitions
    assert m["wave-cycle-128"]["transitions"] == 128 and m["wave-cycle-129"]["transitions"] == 129
    assert m["wave-keep-all"]["keep"] == m["wave-keep-all"]["transitions"]
    assert m["wave-keep-all-but-one"]["keep"] == m["wave-keep-all-but-one"]["transitions"] - 1
    assert m["wave-trains"]["keep"] == 25 and m["wave-never-trains"]["epk"] == 0
    assert m["tuple-4096"]["tuples"] == m["tuple-4096-four-agents"]["tuples"] == m["tuple-T256-4096"]["tuples"] == 4096
    assert m["tuple-word-16-bits"]["word_bits"] == 16 and m["tuple-word-16-bits"]["tuples"] <= 4096
    assert m["tuple-rows-254"]["win_rows"] + 2 == 256 and m["tuple-rows-255"]["win_rows"] + 2 == 257
    assert m["tuple-lds-one-wave"]["tuple_lds_one_wave"] <= LT.LDS_PER_CU < m["tuple-lds-none"]["tuple_lds_one_wave"]
    assert m["tuple-lds-one-wave"]["tuple_waves"] == 1
    for k in ("Reinforce", "ActorCritic"):
        assert m["ptuple-2048-pairs-2048-prices-" + k]["prices"] == m["ptuple-2048-pairs-2048-prices-" + k]["tuples"] == 2048
        assert m["ptuple-rows-254-" + k]["win_rows"] + 2 == 256
        assert m["ptuple-lds-fits-" + k]["ptuple_lds_one_wave"] <= LT.LDS_PER_CU < m["ptuple-lds-over-" + k]["ptuple_lds_one_wave"]
    assert m["ptuple-cdf-24KiB-ActorCritic"]["cdf_bytes"] == 24 * 1024 < m["ptuple-cdf-over-ActorCritic"]["cdf_bytes"]
    for dt in ("f32", "f64"):
        assert m["mixed-64KiB-" + dt]["mixed_lds"] == 64 * 1024 < m["mixed-over-64KiB-" + dt]["mixed_lds"]


QCASES = [c for c in LT.CASES if c["plan"] in ("wave", "tuple")]


@pytest.mark.parametrize("case", QCASES, ids=[c["id"] for c in QCASES])
def test_library_selects_what_the_table_says(lib, case):
    """thrl_select_kernel / thrl_training_cycle on the host: the accepted side is the plan's kernel, the refused side the
    kernel the table names, with the limit's reason in thrl_last_error when that is the generic one."""
    from th_rl_amd import _lib
    for dt in case["dtypes"]:
        cfg, _ = _lib.cfg_from_config(case["config"], case["G"], 1 if dt == "float64" else 0)
        got = _lib.KERNEL_NAMES[lib.thrl_select_kernel(ctypes.byref(cfg), 0)]
        why = lib.thrl_last_error().decode()
        if case["side"] == "accept":
            assert got == case["plan"], (case["id"], dt, got, why)
            if case["plan"] == "wave":
                assert lib.thrl_training_cycle(ctypes.byref(cfg)) == max(case["expect"].get("epk", LT.cycle(case["config"])[0]), 1)
        elif case["id"] == "wave-partial-cycle":
            assert got == "wave"                      # the config is the wave kernel's; only this call's episode count is not
        else:
            assert got == (case["falls_to"] or "generic"), (case["id"], dt, got, why)
            if got == "generic":
                assert case["reason"] in why, (case["id"], why)


def _plan_reasons():
    api = open(os.path.join(CSRC, "thrl_api.hip")).read()
    mixed = open(os.path.join(CSRC, "thrl_mixed.hip")).read()
    out = {}
    for plan, head in (("wave", "WavePlan plan_wave("), ("tuple", "TuplePlan plan_tuple("), ("ptuple", "PTuplePlan plan_ptuple(")):
        body = api[api.index(head):]
        body = body[:body.index("#undef NO")]
        out[plan] = set(re.findall(r'\bNO\("([^"]+)"\)', body))
    body = mixed[mixed.index("int plan_mixed("):]
    out["mixed"] = set(re.findall(r'\*why = "([^"]+)"', body[:body.index("int launch_mixed(")]))
    return out


def test_every_refusal_of_the_four_plans_is_in_the_table():
    src = _plan_reasons()
    assert all(len(v) >= 4 for v in src.values()), src
    for plan, reasons in src.items():
        assert reasons == {r for p, r in LT.REASONS if p == plan}, plan
    for (plan, reason), entry in LT.REASONS.items():
        assert entry[0] in ("pair", "note", "unreachable") and all(entry[1:]), (plan, reason)
        if entry[0] == "pair":
            acc, ref = LT.BY_ID[entry[1]], LT.BY_ID[entry[2]]
            assert acc["side"] == "accept" and ref["side"] == "refuse", (plan, reason)
            # (a policy-tuple refusal is silent: the message of a forced call is the general kernel's or the constructor's)
            if ref["plan"] == plan and plan != "ptuple":
                assert ref["reason"] in reason, (plan, reason, ref["reason"])


def test_unreachable_refusals():
    """No configuration reaches these NO(...) checks: each sits behind the limits checked before it."""
    # action word wider than 16 bits: exhaustive over 1-4 agents of 2..64 actions with at most 4,096 tuples; the widest
    # word is the 16 bits of tuple-word-16-bits
    assert LT.word_bits_worst_case() == 16 == LT.measure(LT.BY_ID["tuple-word-16-bits"])["word_bits"]
    # more than 65,535 resident cells per agent: at most 254 + 2 rows x 64 actions
    assert max((W + 2) * A for W in range(1, 255) for A in range(2, 65)) == 16384 <= 65535
    # the visit histogram (2 B per cell, in dwords) fits the table region (>= 4 B per cell, padded to 4 cells)
    assert all(4 * ((c + 1) // 2) <= 4 * ((c + 3) & ~3) for c in range(1, 16385))
    # LUT images: the tuple kernel's at 4,096 tuples and 4 agents, the policy-tuple kernel's at 2,048 pairs and prices
    assert LT._up(4096 * 8, 16) + 4 * 64 * 8 * 2 + 2 * 8 * 4096 <= 160 * 1024 - 64
    aq = LT._up(LT._up(LT._up(2048 * 2, 16) + 2048 * 2, 16) + 2048 * 4, 16)
    assert aq + 2 * 128 * 8 + 2 * 8 * 2048 == 51200 <= 64 * 1024 - 64
    # the policy-tuple kernel: at most 64 x 32 or 32 x 32 pairs pass the action checks, and a pair has one price
    assert max(64 * 32, 32 * 32) == 2048 <= 4096
    # the wave kernel's window: 128 rows x 32 actions x 8 B x 2 agents (+ 256 B in float32) and a LUT image under 16 KiB
    assert 2 * 128 * 32 * 8 + 256 + 16 * 1024 <= LT.LDS_PER_CU


ORACLE_CASES = [c for c in LT.cases(side="accept") if c["plan"] != "ptuple"]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c["id"] for c in ORACLE_CASES])
def test_oracle_runs_every_accepted_case_for_one_cycle(case):
    """G = 2, one training cycle on the CPU oracle (games with a neural agent have no CPU episode oracle: their reference
    is the operator loop on the device).  Every agent makes one table update per kept transition: E * T visits, less
    what a capacity below the cycle drops, none when the buffer never reaches min_memory."""
    config, G = case["config"], 2
    T = config["environment"]["max_steps"]
    for dt in case["dtypes"]:
        cfg, eps = O.cfg_from_config(config, n_games=G, q_dtype=1 if dt == "float64" else 0)
        q, c, s = O.init(cfg, seed=3)
        q0 = q.copy()
        epk, keep = LT.cycle(config)
        E = max(epk, 1)
        out = O.episodes(cfg, q, c, s, eps, O.Memory(cfg), E, seed=3)
        assert np.isfinite(out["reward_log"]).all() and np.isfinite(q).all()
        for i in range(cfg.n_agents):
            lo, n = O.table_offset(cfg, i), (cfg.n_states[i] + 1) * cfg.n_actions[i]
            visits = c[:, lo:lo + n].sum(axis=1)
            assert (visits == keep).all(), (case["id"], dt, i, visits, keep)
            if keep == E * T:
                assert (visits == E * T).all()
        if epk == 0:
            assert np.array_equal(q, q0)
