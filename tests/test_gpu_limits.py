"""Every episode kernel at the edges of its eligibility plan (limits_table.py; the arithmetic that puts each case on its
limit is checked on the host, test_limits_host.py).

Accepted side: the last configuration a plan takes, kernel forced, both table dtypes, two run() calls.  All-QTable games
against the CPU oracle from the same initial tables / states and the same Philox seed: tables, visit counters, env states
and epsilon identical, mean logs to rtol 1e-12 / atol 1e-13 (sums over steps and games are reordered).  Games with a neural
agent against the operator loop, bit for bit: per-game logs, tables, counters, states, epsilon, replay rings, network
parameters and Adam moments.

Refused side: the first configuration past the limit.  Forcing the kernel raises the limit's reason and launches nothing
(tables, counters and states unchanged); `auto` runs the kernel the table names and matches the reference the same way."""
import re

import numpy as np
import pytest

import limits_table as LT

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

SEED = 23


def _params(plan, side):
    pairs = LT.expand(LT.cases(plan, side))
    return dict(argnames="case,dtype", argvalues=pairs, ids=LT.ids(pairs))


class _Oracle:
    """The CPU oracle carried across run() calls: replay memory, epsilon and the episode index persist."""

    def __init__(self, config, G, dtype, q0, s0):
        self.cfg, self.eps = O.cfg_from_config(config, n_games=G, q_dtype=1 if dtype == "float64" else 0)
        self.q, self.s, self.c = q0.copy(), s0.copy(), np.zeros(q0.shape, np.int32)
        self.mem, self.episode, self.N = O.Memory(self.cfg), 0, self.cfg.n_agents

    def run(self, E):
        out = O.episodes(self.cfg, self.q, self.c, self.s, self.eps, self.mem, E, seed=SEED, first_episode=self.episode)
        self.episode += E
        return out

    def check(self, batch, out, oo, label):
        bad = np.flatnonzero((batch.tables_numpy() != self.q).any(axis=1))
        assert bad.size == 0, "%s: tables of %d games differ (first %s)" % (label, bad.size, bad[:5])
        assert np.array_equal(batch.counters_numpy(), self.c), label
        assert np.array_equal(batch.states_numpy(), self.s), label
        assert [float(x) for x in batch.eps[:self.N]] == [float(x) for x in self.eps[:self.N]], label
        np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13, err_msg=label)
        np.testing.assert_allclose(out["action_log"], oo["action_log"], rtol=1e-12, atol=1e-13, err_msg=label)


def _two_calls_vs_oracle(case, dtype, kernel, ran):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(case["config"], n_games=case["G"], dtype=dtype, kernel=kernel, seed=SEED).init_tables()
    orc = _Oracle(case["config"], case["G"], dtype, gb.tables_numpy(), gb.states_numpy())
    for call, E in enumerate((case["E"], case["E2"])):
        label = "%s %s call %d (%d episodes)" % (case["id"], dtype, call, E)
        out = gb.run(E)
        assert out["kernel"] == ran, label
        orc.check(gb, out, orc.run(E), label)
    T = case["config"]["environment"]["max_steps"]
    epk, keep = LT.cycle(case["config"])
    if ran != "generic" and epk > 0:                  # every kept transition of every cycle is one table update
        cycles = (case["E"] + case["E2"]) // epk
        assert int(gb.counters_numpy().sum()) == case["G"] * orc.N * cycles * min(keep, epk * T), case["id"]


def _forced_call_launches_nothing(case, dtype, kernel):
    import torch
    from th_rl_amd._lib import ThrlError
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(case["config"], n_games=case["G"], dtype=dtype, kernel=kernel, seed=SEED).init_tables()
    q0, s0 = gb.tables_numpy(), gb.states_numpy()
    with pytest.raises(ThrlError, match=re.escape(case["reason"])):
        gb.run(case["E"])
    torch.cuda.synchronize()
    assert np.array_equal(gb.tables_numpy(), q0) and np.array_equal(gb.states_numpy(), s0), case["id"]
    assert not gb.counters_numpy().any() and gb.episode == 0, case["id"]


@pytest.mark.parametrize(**_params("wave", "accept"))
def test_wave_kernel_at_its_limits(case, dtype):
    _two_calls_vs_oracle(case, dtype, "wave", "wave")


@pytest.mark.parametrize(**_params("wave", "refuse"))
def test_wave_kernel_refuses_past_its_limits(case, dtype):
    _forced_call_launches_nothing(case, dtype, "wave")
    if case["falls_to"]:
        _two_calls_vs_oracle(case, dtype, "auto", case["falls_to"])


@pytest.mark.parametrize(**_params("tuple", "accept"))
def test_tuple_kernel_at_its_limits(case, dtype):
    _two_calls_vs_oracle(case, dtype, "tuple", "tuple")


@pytest.mark.parametrize(**_params("tuple", "refuse"))
def test_tuple_kernel_refuses_past_its_limits(case, dtype):
    _forced_call_launches_nothing(case, dtype, "tuple")
    if case["falls_to"]:
        _two_calls_vs_oracle(case, dtype, "auto", case["falls_to"])


# ---------------------------------------------------------------------------------------------------------------
# games on MixedGameBatch


def _mixed(case, dtype):
    from th_rl_amd.mixed import MixedGameBatch
    return MixedGameBatch(case["config"], n_games=case["G"], dtype=dtype, seed=SEED).init_tables()


def _same_as_operator_loop(a, b, ra, rb, label):
    assert np.array_equal(ra["game_reward_log"], rb["game_reward_log"]), label
    assert np.array_equal(ra["game_action_log"], rb["game_action_log"]), label
    assert np.array_equal(a.tables_numpy(), b.tables_numpy()) and np.array_equal(a.counters_numpy(), b.counters_numpy()), label
    assert np.array_equal(a.states_numpy(), b.states_numpy()) and a.eps == b.eps and a.count == b.count, label
    for i in a.nn:
        assert a.nn[i].step == b.nn[i].step, label
        for k in ("price", "action", "reward", "nprice"):
            assert np.array_equal(a.buf[i][k].cpu().numpy(), b.buf[i][k].cpu().numpy()), "%s: ring %s of agent %d" % (label, k, i)
        for k in ("params", "adam_m", "adam_v"):
            assert np.array_equal(getattr(a.nn[i], k).cpu().numpy(), getattr(b.nn[i], k).cpu().numpy()), "%s: %s of agent %d" % (label, k, i)


def _fused_vs_operator_loop(case, dtype, episode_kernel):
    a, b = _mixed(case, dtype), _mixed(case, dtype)
    for call, E in enumerate((case["E"], case["E2"])):
        label = "%s %s call %d (%d episodes)" % (case["id"], dtype, call, E)
        ra, rb = a.run(E, fused=True), b.run(E, fused=False)
        assert ra["kernel"] == "mixed-fused" and ra["episode_kernel"] == episode_kernel and rb["kernel"] == "unfused", label
        _same_as_operator_loop(a, b, ra, rb, label)
    for i in a.nn:                                    # the networks did train: the comparison is not of two idle agents
        if a.cap[i] >= a.min_memory[i]:
            assert a.nn[i].step == case["E"] + case["E2"], case["id"]


def _fused_refuses_and_launches_nothing(case, dtype):
    import torch
    from th_rl_amd._lib import ThrlError
    a = _mixed(case, dtype)
    q0, s0 = a.tables_numpy(), a.states_numpy()
    with pytest.raises(ThrlError, match=re.escape(case["reason"])):
        a.run(case["E"], fused=True)
    torch.cuda.synchronize()
    assert np.array_equal(a.tables_numpy(), q0) and np.array_equal(a.states_numpy(), s0), case["id"]
    assert not a.counters_numpy().any() and a.episode == 0, case["id"]
    return a, q0, s0


@pytest.mark.parametrize(**_params("ptuple", "accept"))
def test_policy_tuple_kernel_at_its_limits(case, dtype):
    _fused_vs_operator_loop(case, dtype, "tuple")


@pytest.mark.parametrize(**_params("ptuple", "refuse"))
def test_policy_tuple_kernel_hands_over_past_its_limits(case, dtype):
    from th_rl_amd._lib import ThrlError
    if case["falls_to"] == "error":                   # no device path at all: the batch cannot be built
        with pytest.raises(ThrlError, match=re.escape(case["reason"])):
            _mixed(case, dtype)
    elif case["falls_to"] == "unfused":               # the general kernel refuses it too: the operator loop runs
        a, _, _ = _fused_refuses_and_launches_nothing(case, dtype)
        b = _mixed(case, dtype)
        ra, rb = a.run(case["E"]), b.run(case["E"], fused=False)
        assert ra["kernel"] == "unfused"
        _same_as_operator_loop(a, b, ra, rb, case["id"])
    else:
        _fused_vs_operator_loop(case, dtype, case["falls_to"])


def _mixed_two_calls_vs_oracle(case, dtype, batch, q0, s0, fused, ran):
    orc = _Oracle(case["config"], case["G"], dtype, q0, s0)
    for call, E in enumerate((case["E"], case["E2"])):
        label = "%s %s call %d (%d episodes)" % (case["id"], dtype, call, E)
        out = batch.run(E, fused=fused)
        assert out["kernel"] == ran, label
        if ran == "mixed-fused":
            assert out["episode_kernel"] == "wave", label          # two QTables: the general kernel, one wavefront per game
        orc.check(batch, out, orc.run(E), label)


@pytest.mark.parametrize(**_params("mixed", "accept"))
def test_general_mixed_kernel_at_its_limits(case, dtype):
    a = _mixed(case, dtype)
    _mixed_two_calls_vs_oracle(case, dtype, a, a.tables_numpy(), a.states_numpy(), True, "mixed-fused")


@pytest.mark.parametrize(**_params("mixed", "refuse"))
def test_general_mixed_kernel_refuses_past_its_limits(case, dtype):
    a, q0, s0 = _fused_refuses_and_launches_nothing(case, dtype)
    _mixed_two_calls_vs_oracle(case, dtype, a, q0, s0, None, "unfused")
