"""Action grids wider than the LDS kernels take (more than 64 actions) on the device: the operators alone, the generic
episode kernel, the operator loop of MixedGameBatch, parity mode and greedy play, each against the CPU oracle or
oracle.philox bit for bit.  The games are those of tests/wide_grids_cases.py; tests/test_wide_grids_host.py asserts that
the oracle's runs of them hold explored choices of 128 / 256 and more and train on them, and shows that a choice carried
in 8 bits (thrl_op_draws before ABI v4) fails these comparisons."""
import ctypes
import functools

import numpy as np
import pytest

import wide_grids_cases as W
from oracle import oracle as O  # (checker only)

pytestmark = pytest.mark.gpu

CASES = [(n, d) for n in W.CASES for d in W.DTYPES]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ thrl_op_draws
DRAW_ACTIONS = [257, 1000, 129, 32000]          # wide choices in even and odd slots, in the first and second draw of a step


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_op_draws_against_philox(N):
    """u, u2, noise_u, noise_a bit for bit, choice = (word * A) >> 32 in [0, A): G = 300 (one full block and a tail), a
    game_offset above 2^32, a seed with both key words set, a non-zero episode and step."""
    import torch
    from th_rl_amd import _lib
    A = DRAW_ACTIONS[:N]
    G, seed, off, episode, step = 300, 0x1234567_89ABCDEF, 5 * 2 ** 32 + 123, 7, 3
    config = W.game([W.agent(a) for a in A], T=5, noise_prob=0.3)
    cfg, _ = _lib.cfg_from_config(config, G, 0)
    L = _lib.load()
    u = torch.zeros((N, G), dtype=torch.float64, device="cuda:0")
    u2, nu, na = torch.zeros_like(u), torch.zeros_like(u[0]), torch.zeros_like(u[0])
    ch = torch.full((N + 1, G), -7, dtype=torch.int32, device="cuda:0")       # a row to spare: nothing writes past [N][G]
    _lib.check(L.thrl_op_draws(ctypes.byref(cfg), seed, off, episode, step, _p(u), _p(ch), _p(u2), _p(nu), _p(na), None),
               "thrl_op_draws")
    torch.cuda.synchronize()
    ru, rw, rc, nz = W.step_draws(A, G, seed, off, episode, step, noise=True)
    ch = ch.cpu().numpy()
    assert np.array_equal(u.cpu().numpy(), ru) and np.array_equal(u2.cpu().numpy(), rw * 2.0 ** -32)
    assert np.array_equal(ch[:N], rc) and (ch[N] == -7).all()
    assert all(ch[i].min() >= 0 and ch[i].max() < A[i] for i in range(N))
    assert all(ch[i].max() >= 128 for i in range(N))                          # the draws do hold what a byte loses
    lo = cfg.env_a * 0.7
    assert np.array_equal(nu.cpu().numpy(), nz[0] * 2.0 ** -32)
    assert np.array_equal(na.cpu().numpy(), lo + (cfg.env_a - lo) * (nz[1] * 2.0 ** -32))


# ------------------------------------------------------------------------------------------------ thrl_op_sample_action
@pytest.mark.parametrize("dtype", W.DTYPES)
def test_op_sample_action_returns_the_choice_or_the_first_argmax(dtype):
    import torch
    from th_rl_amd import _lib
    G, agent, eps = 70, 1, 0.5
    config = W.game([W.agent(257, states=10), W.agent(1000, states=11)], T=5)
    A, S = 1000, 11
    cfg, _ = _lib.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    L = _lib.load()
    rs = np.random.RandomState(5)
    q = W.planted_tables(config, G, dtype, seed=5)
    off = O.table_offset(O.cfg_from_config(config, G, 1)[0], agent)
    tab = q[:, off:off + (S + 1) * A].reshape(G, S + 1, A)
    tab[0::3, :, A - 1] = 20.0                              # the maximum in the last column
    tab[1::3, :, 700] = 30.0; tab[1::3, :, 300] = 30.0      # an exact tie: the first one wins
    q[:, off:off + (S + 1) * A] = tab.reshape(G, -1)
    price = rs.uniform(0, 10, G)
    u = rs.uniform(0, 1, G)
    choice = rs.randint(0, A, G).astype(np.int32)
    choice[::4] = A - 1
    out = torch.full((G,), -1, dtype=torch.int32, device="cuda:0")
    d = [_dev(q), _dev(price), _dev(u), _dev(choice)]
    _lib.check(L.thrl_op_sample_action(ctypes.byref(cfg), agent, _p(d[0]), _p(d[1]), eps, _p(d[2]), _p(d[3]), 1, _p(out),
                                       None), "thrl_op_sample_action")
    got = out.cpu().numpy()
    rows = np.array([O.encode32(p, 10, S) for p in price])
    greedy = np.array([int(np.argmax(tab[g, rows[g]])) for g in range(G)])
    want = np.where(u < eps, choice, greedy)
    assert np.array_equal(got, want)
    explored = u < eps
    assert (got[explored] == A - 1).sum() >= 3 and (got[~explored] == A - 1).sum() >= 3 and (got[~explored] == 300).sum() >= 3
    # a choice that is no action of the agent counts as the last one
    bad = choice.copy()
    bad[0::3], bad[1::3], bad[2::3] = A, -1, 2 ** 31 - 1
    d[3] = _dev(bad)
    _lib.check(L.thrl_op_sample_action(ctypes.byref(cfg), agent, _p(d[0]), _p(d[1]), eps, _p(d[2]), _p(d[3]), 1, _p(out),
                                       None), "thrl_op_sample_action")
    assert np.array_equal(out.cpu().numpy(), np.where(explored, A - 1, greedy))


# ------------------------------------------------------------------------------------------------ episodes
@functools.lru_cache(maxsize=None)
def _device_init_and_oracle(name, dtype):
    """The device's own initial tables of a case and the oracle's run from them: (q0, s0, q, counter, state, eps)."""
    from th_rl_amd.batched import GameBatch
    config, G, E, seed, off = W.CASES[name]
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel="auto", seed=seed, game_offset=off).init_tables()
    q0, s0 = gb.tables_numpy().copy(), gb.states_numpy().copy()
    assert not gb.counters_numpy().any()
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    q, s, c = q0.copy(), s0.copy(), np.zeros(q0.shape, np.int32)
    O.episodes(cfg, q, c, s, eps, O.Memory(cfg), E, seed=seed, game_offset=off)
    for a in (q0, s0, q, s, c, eps):
        a.setflags(write=False)
    return q0, s0, q, c, s, eps


@pytest.mark.parametrize("name,dtype", CASES)
def test_init_tables_match_the_oracle(name, dtype):
    """thrl_qtable_init against O.init at the project's 1e-11 (libm differences), on shapes test_init_matches_oracle never
    had: a gamma per agent, three and four agents, wide rows; float32 tables are the float64 value rounded, within one
    float32 ulp."""
    config, G, E, seed, off = W.CASES[name]
    q0, s0 = _device_init_and_oracle(name, dtype)[:2]
    q64, _, s64 = O.init(O.cfg_from_config(config, G, 1)[0], seed, off)
    assert np.array_equal(s0, s64)
    if dtype == "float64":
        np.testing.assert_allclose(q0, q64, rtol=0, atol=1e-11)
    else:
        assert q0.dtype == np.float32
        assert (np.abs(q0.astype(np.float64) - q64) <= np.spacing(np.abs(q64).astype(np.float32)).astype(np.float64)).all()
    gammas = [a["gamma"] for a in config["agents"]]
    cfg = O.cfg_from_config(config, G, 1)[0]
    # Not a tolerance on the kernel (the comparisons above are the check): a plausibility test that agent i got ITS gamma.
    # Its n cells are 12.5 / (1 - gamma) + N(0, 1), so their mean is within 6 / sqrt(n) of that value but once in 10^9
    # tables; the nearest other gamma of any case moves the value by 12.5 / 0.1 - 12.5 / 0.05 = -125.
    for i, gam in enumerate(gammas):
        lo = O.table_offset(cfg, i)
        hi = O.table_offset(cfg, i + 1) if i + 1 < len(gammas) else q0.shape[1]
        n = G * (hi - lo)
        assert abs(q0[:, lo:hi].astype(np.float64).mean() - 12.5 / (1 - gam)) < 6 / np.sqrt(n) + 1e-4   # (+ float32 rounding at 250)


@pytest.mark.parametrize("name,dtype", CASES)
def test_generic_kernel_equals_the_oracle(name, dtype):
    from th_rl_amd.batched import GameBatch
    config, G, E, seed, off = W.CASES[name]
    q0, s0, q, c, s, eps = _device_init_and_oracle(name, dtype)
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel="auto", seed=seed, game_offset=off).set_tables(q0.copy(), s0.copy())
    out = gb.run(E)
    assert out["kernel"] == "generic"
    N = len(config["agents"])
    assert np.array_equal(gb.tables_numpy(), q)
    assert np.array_equal(gb.counters_numpy(), c) and np.array_equal(gb.states_numpy(), s)
    assert [float(x) for x in gb.eps[:N]] == [float(x) for x in eps[:N]]
    assert c.sum() > 0


@pytest.mark.parametrize("name,dtype", CASES)
def test_operator_loop_equals_the_oracle(name, dtype):
    """MixedGameBatch on the same all-QTable games: the fused kernels stop at 64 actions (and at 64 KiB of tables per game),
    so run() falls back to thrl_op_draws -> thrl_op_sample_action -> thrl_op_scale -> thrl_op_env_step -> thrl_op_td_update."""
    from th_rl_amd.mixed import MixedGameBatch
    config, G, E, seed, off = W.CASES[name]
    q0, s0, q, c, s, eps = _device_init_and_oracle(name, dtype)
    mb = MixedGameBatch(config, n_games=G, dtype=dtype, seed=seed, game_offset=off).set_tables(q0.copy(), s0.copy())
    out = mb.run(E)
    assert out["kernel"] == "unfused"
    N = len(config["agents"])
    assert np.array_equal(mb.tables_numpy(), q)
    assert np.array_equal(mb.counters_numpy(), c) and np.array_equal(mb.states_numpy(), s)
    assert [float(x) for x in mb.eps[:N]] == [float(x) for x in eps[:N]]


def test_wide_qtable_against_reinforce_on_the_operator_loop():
    """QTable(200) against Reinforce(21): no oracle plays this pair, so the invariants -- every logged mean action inside
    its agent's action_range (to the rounding of its T divisions and additions), counters non-negative and summing to the transitions
    trained, two runs identical."""
    from th_rl_amd.mixed import MixedGameBatch
    T, G, E = 10, 37, 5
    qa = W.agent(200, states=20, lo=0.1, hi=0.4, min_memory=13, capacity=25)
    config = {"agents": [qa, dict(name="Reinforce", gamma=0.99, actions=21, states=1, action_range=[0.05, 0.3], min_memory=2 * T)],
              "environment": dict(name="NoisyPriceState", noise_prob=0.0, a=10, b=1, nplayers=2, max_steps=T)}
    runs = []
    for _ in range(2):
        mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=21).init_tables()
        out = mb.run(E)
        assert out["kernel"] == "unfused"
        runs.append((out["game_reward_log"], out["game_action_log"], mb.tables_numpy(), mb.counters_numpy(), mb.states_numpy(),
                     mb.nn[1].params.cpu().numpy(), np.array(mb.eps)))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    act, cnt = runs[0][1], runs[0][3]
    # a logged mean is the sum of T quotients action / T, each action in [lo, hi]: T divisions and T additions, each
    # rounded once, move it by at most 2 T ulp(hi) from a value in the range
    for i, (lo, hi) in enumerate(([0.1, 0.4], [0.05, 0.3])):
        slack = 2 * T * np.spacing(hi)
        assert (act[:, i] >= lo - slack).all() and (act[:, i] <= hi + slack).all()
    assert (cnt >= 0).all()
    trained = sum(len(b) for b in W.trained_steps({"agents": [qa], "environment": config["environment"]}, E)[0])
    assert trained > 0 and cnt.sum() == trained * G
    off1 = mb.offsets[1]
    assert cnt[:, :off1].sum() == trained * G and not cnt[:, off1:].any()
    assert cnt[:, :off1].reshape(G, 21, 200)[:, :, 128:].sum() > 0            # ... some of them past column 127


# ------------------------------------------------------------------------------------------------ parity mode
def _inj(config, G, E, seed):
    T, A = config["environment"]["max_steps"], [a["actions"] for a in config["agents"]]
    rs = np.random.RandomState(seed)
    u = rs.uniform(0, 1, (E, T, len(A), G))
    ch = np.stack([rs.randint(0, a, (E, T, G)) for a in A], axis=2)
    return u, ch


def test_injection_is_refused_past_128_actions():
    from th_rl_amd import _lib
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    config, G, E, seed, off = W.CASES["21x129"]
    u, ch = _inj(config, G, 2, 1)
    ch = np.minimum(ch, 127)
    gb = GameBatch(config, n_games=G, dtype="float64", seed=seed).init_tables()
    q0 = gb.tables_numpy().copy()
    with pytest.raises(_lib.ThrlError, match="QTable agent 1 has 129 actions") as ei:
        gb.run(2, inj=dict(u=u, choice=ch))
    assert ei.value.code == _lib.ERR_BAD_CONFIG and np.array_equal(gb.tables_numpy(), q0) and gb.episode == 0
    mb = MixedGameBatch(config, n_games=G, dtype="float64", seed=seed).init_tables()
    with pytest.raises(_lib.ThrlError, match="QTable agent 1 has 129 actions") as ei:
        mb.run(2, inj=dict(u=u, choice=ch))
    assert ei.value.code == _lib.ERR_BAD_CONFIG and mb.episode == 0
    # a choice the recorded format cannot hold is refused, not wrapped
    config, G, E, seed, off = W.CASES["127x128"]
    u, ch = _inj(config, G, 2, 2)
    ch[0, 0, 1, 0] = 128
    gb = GameBatch(config, n_games=G, dtype="float64", seed=seed).init_tables()
    with pytest.raises(_lib.ThrlError, match="does not fit int8"):
        gb.run(2, inj=dict(u=u, choice=ch))


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_injected_choice_127_reproduces_the_oracle(dtype):
    """128 actions, the widest the injected format holds: choice 127 in every fourth game of that agent."""
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    config, G, E, seed, off = W.CASES["127x128"]
    q0, s0 = _device_init_and_oracle("127x128", dtype)[:2]
    u, ch = _inj(config, G, E, 3)
    ch[:, :, 1, ::4] = 127
    ch8 = np.ascontiguousarray(ch.astype(np.int8))
    assert (ch8 == ch).all() and ((ch8[:, :, 1] == 127) & (u[:, :, 1] < 0.49)).sum() >= 5
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    q, s, c = q0.copy(), s0.copy(), np.zeros(q0.shape, np.int32)
    out = O.episodes(cfg, q, c, s, eps, O.Memory(cfg), E, inj_u=np.ascontiguousarray(u), inj_choice=ch8, trace=True)
    assert (out["trace_actions"][:, :, 1] == 127).sum() >= 5
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel="auto", seed=seed, game_offset=off).set_tables(q0.copy(), s0.copy())
    assert gb.run(E, inj=dict(u=u, choice=ch8))["kernel"] == "generic"
    mb = MixedGameBatch(config, n_games=G, dtype=dtype, seed=seed, game_offset=off).set_tables(q0.copy(), s0.copy())
    assert mb.run(E, inj=dict(u=u, choice=ch))["kernel"] == "unfused"
    for b in (gb, mb):
        assert np.array_equal(b.tables_numpy(), q) and np.array_equal(b.counters_numpy(), c)
        assert np.array_equal(b.states_numpy(), s) and [float(x) for x in b.eps[:2]] == [float(x) for x in eps[:2]]


# ------------------------------------------------------------------------------------------------ greedy play
@pytest.mark.parametrize("dtype", W.DTYPES)
def test_play_greedy_on_wide_tables(dtype):
    from th_rl_amd.batched import GameBatch
    config, G, E, seed, off = W.CASES["257x1000x3"]
    q = W.planted_tables(config, G, dtype, seed=9)
    st0 = np.random.RandomState(9).uniform(0, 10, (2, G))
    gb = GameBatch(config, n_games=G, dtype=dtype, seed=seed, game_offset=off).set_tables(q, st0[0])
    cfg, _ = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    for kw, okw in ((dict(state0=st0), dict(state0=np.ascontiguousarray(st0))), ({}, dict(seed=seed, game_offset=off))):
        mr, ma = gb.play_greedy(iters=2, **kw)
        omr, oma = O.play_greedy(cfg, q, 2, **okw)
        assert np.array_equal(mr, omr) and np.array_equal(ma, oma)
    # the planted maxima are played: an action mean that only columns past 255 can give
    lo, hi = config["agents"][1]["action_range"]
    assert (oma[:, 1] > lo + (hi - lo) * 256 / 999).any()
