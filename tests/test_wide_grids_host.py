"""Wide action grids on the host: what the oracle's runs of tests/wide_grids_cases.py contain, and what an 8-bit choice
would have made of them.

The device tests (tests/test_gpu_wide_grids.py) compare against these oracle runs bit for bit.  A comparison of that kind
only has teeth if the run holds what the narrow fields lose: explored steps whose random choice is 128 or more (256 or
more for agents past 256 actions) and trained transitions with such an action.  The conditions are asserted here, per
case and per agent, so a later edit of a seed or a size cannot empty a case without a failure.  No GPU is needed."""
import numpy as np
import pytest

import wide_grids_cases as W
from oracle import oracle as O

MIN_WIDE = 5            # explored steps at or past each threshold that a wide agent must have


def _explored(name, dtype):
    config, G, E, seed, off = W.CASES[name]
    cfg, eps0 = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    u, ch = W.run_draws(name)
    eps = W.eps_schedule(cfg, eps0, E)                      # [E, N]
    return u < eps[:, None, :, None], ch


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("name", list(W.CASES))
def test_oracle_run_holds_wide_choices_and_trains_on_them(name, dtype):
    config, G, E, seed, off = W.CASES[name]
    A = W.n_actions(name)
    run = W.oracle_run(name, dtype)
    explored, ch = _explored(name, dtype)
    act = run["trace_actions"]
    # the trace is the draws' doing: an explored step took the choice, 64-bit product and all
    assert np.array_equal(act[explored], ch[explored])
    assert all(0 <= act[:, :, i].min() and act[:, :, i].max() < A[i] for i in range(len(A)))
    trained = W.trained_steps(config, E)
    assert all(len(t) >= 1 for t in trained), "every agent of every case trains"
    for i, a in enumerate(A):
        for bound in (128, 256):
            if a > bound:
                n = int((explored[:, :, i] & (ch[:, :, i] >= bound)).sum())
                assert n >= MIN_WIDE, "%s agent %d (%d actions): %d explored steps with a choice >= %d" % (name, i, a, n, bound)
        if a > 128:
            steps = [et for batch in trained[i] for et in batch]
            wide = sum(int((act[e, t, i] >= 128).sum()) for e, t in steps)
            assert wide >= 1, "%s agent %d: no trained transition with an action >= 128" % (name, i)
            # ... and the tables show it: a visited cell in a column past 127
            off_i = O.table_offset(cfg_of(name, dtype), i)
            rows = int(config["agents"][i]["states"]) + 1
            cnt = run["counter"][:, off_i:off_i + rows * a].reshape(G, rows, a)
            assert cnt[:, :, 128:].sum() == wide


def cfg_of(name, dtype):
    config, G = W.CASES[name][:2]
    return O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)[0]


def test_the_cases_cover_the_widths_and_the_slots():
    widths = {a for name in W.CASES for a in W.n_actions(name)}
    assert {65, 127, 128, 129, 255, 256, 257, 1000} <= widths
    wide_slots = {i & 1 for name in W.CASES for i, a in enumerate(W.n_actions(name)) if a > 128}
    assert wide_slots == {0, 1}                             # x.x / x.y and x.z / x.w both carry a wide choice
    assert any(len(W.n_actions(n)) == 3 for n in W.CASES) and any(len(W.n_actions(n)) == 4 for n in W.CASES)
    assert any(c[0]["environment"]["noise_prob"] > 0 for c in W.CASES.values())
    assert any(a["states"] == 32000 and a["actions"] == 2 for c in W.CASES.values() for a in c[0]["agents"])
    for name, (config, G, E, seed, off) in W.CASES.items():
        T = config["environment"]["max_steps"]
        assert G <= 67 and G % 64 and T <= 20 and E <= 6, name
        assert all(a["epsilon"] == 0.5 for a in config["agents"])
        assert all(10 <= a["states"] <= 50 or a["states"] == 32000 for a in config["agents"]), name


WIDE = [(n, i) for n in W.CASES for i, a in enumerate(W.n_actions(n)) if a > 128]


@pytest.mark.parametrize("name,agent", WIDE)
@pytest.mark.parametrize("dtype", W.DTYPES)
def test_an_int8_choice_would_fail_the_device_comparison(name, agent, dtype):
    """The teeth of the device comparison, shown without a device: pass the oracle's recorded choices through int8, as
    thrl_op_draws stored them before ABI v4.  Choices of 128 and more come back negative, and the oracle's own td_update
    on those actions leaves a different table and different counters, so the bit-for-bit comparison fails."""
    config, G, E, seed, off = W.CASES[name]
    a = W.n_actions(name)[agent]
    cfg = cfg_of(name, dtype)
    run = W.oracle_run(name, dtype)
    explored, ch = _explored(name, dtype)
    narrow = ch.astype(np.int8).astype(np.int64)
    lost = explored[:, :, agent] & (narrow[:, :, agent] != ch[:, :, agent])
    assert lost.sum() >= MIN_WIDE and (narrow[:, :, agent][lost] < 0).sum() >= MIN_WIDE
    assert a > 256 or (narrow[:, :, agent][lost] < 0).all()
    # the first training batch of a game that explored such a choice in it, from the initial tables.  Rows >= 1 only: the
    # wrapped action indexes the row before (at row 0 of agent 0 in game 0, memory before the table), which the
    # oracle's cell address, st * A + ac, can only show inside the table
    batch = W.trained_steps(config, E)[agent][0]
    p = config["agents"][agent]
    rows, off_a = int(p["states"]) + 1, O.table_offset(cfg, agent)
    e_idx, t_idx = np.array([e for e, t in batch]), np.array([t for e, t in batch])
    k = e_idx * config["environment"]["max_steps"] + t_idx
    for g in range(G):
        price = np.concatenate([[run["s0"][g]], run["trace_price"][:, :, g].ravel()])      # before step k; after it at k + 1
        st = np.array([O.encode64(price[x], p.get("max_state", 10), p["states"]) for x in k])
        ns = np.array([O.encode64(price[x + 1], p.get("max_state", 10), p["states"]) for x in k])
        ac = run["trace_actions"][e_idx, t_idx, agent, g].astype(np.int64)
        bad = np.where(lost[e_idx, t_idx, g], narrow[e_idx, t_idx, agent, g], ac)
        keep = st >= 1
        if (bad[keep] < 0).any():
            break
    else:
        pytest.fail("no game explores a choice that wraps negative, off row 0, in the first training batch")
    rw = np.zeros(len(k))       # the reward does not matter to where the update lands
    tabs = []
    for actions in (ac, bad):
        t = run["q0"][g, off_a:off_a + rows * a].reshape(rows, a).copy()
        c = np.zeros((rows, a), np.int32)
        O.td_update(t, c, st[keep], actions[keep], rw[keep], ns[keep], p["alpha"], p["gamma"])
        tabs.append((t, c))
    assert not np.array_equal(tabs[0][0], tabs[1][0]) and not np.array_equal(tabs[0][1], tabs[1][1])
    hit = keep & (bad < 0)                  # the cells the wrapped choices should have reached: visited less often, or never
    assert (tabs[1][1][st[hit], ac[hit]] < tabs[0][1][st[hit], ac[hit]]).all()
    assert tabs[1][1].sum() == tabs[0][1].sum() == keep.sum()          # (the visits went to the row before)


# ------------------------------------------------------------------------------------------------ parity mode
def test_check_injection_refuses_what_int8_cannot_hold():
    from th_rl_amd import _lib
    from th_rl_amd.mixed import INJ_MAX_ACTIONS, check_injection
    E, T, N, G = 2, 3, 2, 4
    inj = dict(u=np.zeros((E, T, N, G)), choice=np.zeros((E, T, N, G), np.int64))
    kinds = ["QTable", "QTable"]
    assert INJ_MAX_ACTIONS == 128
    out = check_injection(inj, E, T, N, G, kinds, False, actions=[128, 21])
    assert out["choice"].dtype == np.int8
    with pytest.raises(_lib.ThrlError, match="agent 1 has 129 actions") as ei:
        check_injection(inj, E, T, N, G, kinds, False, actions=[128, 129])
    assert ei.value.code == _lib.ERR_BAD_CONFIG
    # a neural agent's slot is not a choice: its width does not matter here
    check_injection(dict(inj, action=np.zeros((E, T, N, G), np.int8)), E, T, N, G, ["QTable", "Reinforce"], False, actions=[21, 200])
    inj["choice"][0, 0, 0, 0] = 128
    with pytest.raises(_lib.ThrlError, match="does not fit int8"):
        check_injection(inj, E, T, N, G, kinds, False, actions=[128, 21])


# ------------------------------------------------------------------------------------------------ the analyses' mirrors
def test_mirrors_take_the_wide_configs_and_their_policies_pass_a_byte():
    """The numpy mirrors that tests/test_gpu_wide_analyses.py holds the device to run the wide shapes, and on the planted
    tables their walks depend on action indices of 255, 256 and more: with every greedy action reduced modulo 256, as a
    one-byte policy would hold it, the deviation mirror gives another answer."""
    import deviation_mirror as M
    import stationary_mirror as S
    import os
    import re
    import test_gpu_wide_analyses as GA
    # GA._deviation_plan restates thrl_deviation's plan: hold its constants and its two expressions to the sources
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "th_rl_amd", "csrc")
    hdr = open(os.path.join(csrc, "thrl_deviation.h")).read()
    consts = {k: eval(v) for k, v in re.findall(r"constexpr int (kDev\w+) = ([0-9* ]+);", hdr)}
    assert (consts["kDevTile"], consts["kDevLdsBudget"], consts["kDevMaxLut"]) == (256, 64 * 1024, 1024)
    api = open(os.path.join(csrc, "thrl_api_analysis.hip")).read()
    assert "a.pol_bytes = max_a <= 256 ? 1 : 2;" in api
    assert "(int64_t)((lut_n * 8 + 15) & ~15) + (int64_t)kDevTile * entries * a.pol_bytes;" in api
    assert "a.staged = lut_n <= kDevMaxLut && lds <= kDevLdsBudget;" in api
    assert "if (!a.staged) launch_n<T, uint8_t, false>(a, s);" in open(os.path.join(csrc, "thrl_deviation.hip")).read()
    for name, (config, staged, pol_bytes) in GA.DEVIATION.items():
        assert GA._deviation_plan(config) == (staged, pol_bytes), name
        q = W.planted_tables(config, 16, "float32", seed=3)
        s0 = np.random.RandomState(3).uniform(0, 10, 16)
        pol = S.policies(config, q)
        A = max(a["actions"] for a in config["agents"])
        assert (pol >= min(255, A - 1)).sum() >= 5, name
        ref = M.analyse(config, q, s0, deviator=0, steps=6, dev_len=2, horizon=512)
        assert (ref["lam"] >= 1).all(), name                   # every cycle found within the horizon the tests pass
        if A > 256:
            narrow = q.copy()                                   # tables whose greedy policy is the wide one modulo 256
            off = 0
            for a in config["agents"]:
                rows, n = a["states"] + 1, a["actions"]
                tab = narrow[:, off:off + rows * n].reshape(16, rows, n)
                best = tab.argmax(axis=2)
                g, r = np.nonzero(best >= 256)
                tab[g, r, best[g, r] % 256] = 99.0
                narrow[:, off:off + rows * n] = tab.reshape(16, -1)
                off += rows * n
            assert (S.policies(config, narrow) == pol % 256).all()
            bad = M.analyse(config, narrow, s0, deviator=0, steps=6, dev_len=2, horizon=512)
            assert not np.array_equal(bad["action_rows"], ref["action_rows"]), name


def test_the_state_set_analyses_plan_257_by_15_and_refuse_258_by_16():
    """thrl_equilibrium, thrl_attractors and thrl_stationary make their plan before they look at a pointer: with the tables
    left NULL a shape their limits take ends in THRL_ERR_NULL, one they refuse in THRL_ERR_UNSUPPORTED and its message."""
    import ctypes

    import test_attractors_host as AT
    import test_equilibrium_host as EQ
    import test_gpu_wide_analyses as GA
    import test_stationary_host as ST
    from th_rl_amd import _lib, build
    build.build()
    lib = _lib.load()
    over = W.game([W.agent(258, states=50), W.agent(16, states=40)], T=10)
    for entry, args in (("thrl_equilibrium", EQ._args), ("thrl_attractors", AT._args), ("thrl_stationary", ST._args)):
        fn = getattr(lib, entry)
        cfg = _lib.cfg_from_config(GA.WIDE15, 64, 0)[0]
        a = args()
        assert fn(ctypes.byref(cfg), None, ctypes.byref(a), None) == -2, (entry, lib.thrl_last_error())
        cfg = _lib.cfg_from_config(over, 64, 0)[0]
        assert fn(ctypes.byref(cfg), None, ctypes.byref(a), None) == -3, (entry, lib.thrl_last_error())
        assert b"4096" in lib.thrl_last_error() and b"tuples" in lib.thrl_last_error(), lib.thrl_last_error()


def test_the_16_bit_replay_memory_rests_on_validate():
    """k_generic_episodes keeps replay rows and actions as int16, and every analysis keeps policies as uint16: safe because
    validate() stops at 32,000 states and 32,000 actions.  Whoever moves that bound meets this test first."""
    import ctypes
    from th_rl_amd import _lib, build
    build.build()
    lib = _lib.load()

    def plan(**kw):
        cfg = _lib.cfg_from_config(W.game([W.agent(2, states=10), W.agent(**dict(dict(actions=2, states=10), **kw))], T=5), 4, 0)[0]
        return lib.thrl_select_kernel(ctypes.byref(cfg), 0), lib.thrl_last_error()

    assert 32000 <= np.iinfo(np.int16).max
    assert plan(actions=32000)[0] == _lib.KERNEL_GENERIC and plan(states=32000)[0] == _lib.KERNEL_GENERIC
    rc, msg = plan(actions=32001)
    assert rc == _lib.ERR_BAD_CONFIG and b"actions=32001 out of [2,32000]" in msg
    rc, msg = plan(states=32001)
    assert rc == _lib.ERR_BAD_CONFIG and b"states=32001 out of [1,32000]" in msg
