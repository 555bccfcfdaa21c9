"""QTable.counter (agents.py:76) over long launches.  The episode kernels keep a launch's visits in 16-bit LDS cells
before adding them to the int32 counters: k_wave_episodes and k_tuple_episodes are cut into launches of at most 32
episodes by the host, k_ptuple_episodes folds its cells every floor(65535 / T) episodes.  Every test here puts more than
65,535 visits into one cell (asserted: without that it would pass for the wrong reason) and checks the counters bit
for bit against an int32 count: the C oracle, or the general fused kernel k_mixed_wave for games with neural agents.

The regime: greedy QTable agents (epsilon 0) whose tables are ~0 except one dominant action per game and agent, so each
game sits in a fixed point -- what a converged agent against a fixed opponent does."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

CFG_AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.0, epsilon=0.0,
                 eps_step=0.9995, action_range=[0.2, 0.4])
CFG_ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
WAVE = {"agents": [dict(CFG_AGENT), dict(CFG_AGENT, alpha=0.3)], "environment": dict(CFG_ENV)}
# the training cycle spans two episodes (max_steps 50 < min_memory 100): the wave kernel cuts launches at 32 episodes
CYCLE = {"agents": [dict(CFG_AGENT, min_memory=100, capacity=500), dict(CFG_AGENT, min_memory=100, capacity=500, alpha=0.3, gamma=0.9)],
         "environment": dict(CFG_ENV, max_steps=50)}
THREE = {"agents": [dict(CFG_AGENT, actions=11, states=50, action_range=[0.1, 0.3], min_memory=25),
                    dict(CFG_AGENT, actions=21, states=100, action_range=[0.15, 0.35], min_memory=25),
                    dict(CFG_AGENT, actions=5, states=20, action_range=[0.0, 0.3], min_memory=25, max_state=10)],
         "environment": dict(CFG_ENV, nplayers=3, max_steps=25)}
# a frozen neural opponent (capacity < min_memory: it never trains) on a narrow action range, so the price -- the QTable
# agent's state -- barely depends on its draws
FROZEN_R = {"name": "Reinforce", "gamma": 0.995, "actions": 21, "states": 1, "action_range": [0.3, 0.3005],
            "capacity": 200, "min_memory": 400}
FROZEN_AC = {"name": "ActorCritic", "gamma": 0.98, "actions": 21, "states": 1, "action_range": [0.3, 0.3005],
             "capacity": 200, "min_memory": 400}
U16 = 65535


def _dominant(q, offsets, shapes, qtable_agents, seed):
    """Tables ~0 (the initial tables scaled by 1e-3) with one action per game and QTable agent at 100 in every row: a greedy
    agent then plays that action whatever the state, and the visited cells keep it on top (their TD fixed point
    reward / (1 - gamma) stays far above 1e-3 * the initial values)."""
    q = np.array(q, copy=True)
    rs = np.random.RandomState(seed)
    for i in qtable_agents:
        r, a = shapes[i]
        t = q[:, offsets[i]:offsets[i] + r * a].reshape(-1, r, a)
        t *= 1e-3
        t[np.arange(q.shape[0]), :, rs.randint(0, a, q.shape[0])] = 100.0
        q[:, offsets[i]:offsets[i] + r * a] = t.reshape(q.shape[0], -1)
    return q


def _qtable_visits(c, offsets, shapes, i):
    r, a = shapes[i]
    return c[:, offsets[i]:offsets[i] + r * a]


# ---------------------------------------------------------------- QTable-only games against the C oracle (int32 counts)
def _qtable_long_launch(config, G, E, dtype, kernel, seed):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel=kernel, seed=seed).init_tables()
    q0 = _dominant(gb.tables_numpy(), gb.offsets, gb.shapes, range(gb.N), seed)
    s0 = gb.states_numpy()
    gb.set_tables(q0, s0)
    out = gb.run(E)
    assert out["kernel"] == kernel
    cfg, eps = O.cfg_from_config(config, n_games=G, q_dtype=1 if dtype == "float64" else 0)
    q, s = q0.astype(gb.tables_numpy().dtype), s0.copy()
    c = np.zeros(q.shape, np.int32)
    oo = O.episodes(cfg, q, c, s, eps, O.Memory(cfg), E, seed=seed)
    gc = gb.counters_numpy()
    T = config["environment"]["max_steps"]
    for i in range(gb.N):
        v = _qtable_visits(gc, gb.offsets, gb.shapes, i)
        assert (v.sum(axis=1, dtype=np.int64) == E * T).all(), i       # one visit per step and agent
    assert int(c.max()) > U16, "the regime the test exists for: > 65,535 visits in one cell"
    assert np.array_equal(gc, c)
    assert np.array_equal(gb.tables_numpy(), q)
    assert np.array_equal(gb.states_numpy(), s)
    assert [float(x) for x in gb.eps[:gb.N]] == [float(x) for x in eps[:gb.N]]
    np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13)
    return gb


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("E", [704, 750])                  # 22 whole 32-episode launches; 23 launches, the last one of 14
def test_wave_kernel_counters_past_16_bits_vs_oracle(E, dtype):
    """k_wave_episodes: one GameBatch.run of E x 100 steps, greedy, counts of one cell summed over 22-23 launches of
    <= 32 episodes past 2^16: tables, counters, state and epsilon bit for bit against the oracle."""
    _qtable_long_launch(WAVE, 160, E, dtype, "wave", seed=77)


def test_wave_kernel_counters_past_16_bits_two_episode_cycle_vs_oracle():
    """The wave kernel with a training cycle of two episodes (launches cut at whole cycles: 32 episodes) over 1,350
    episodes -- a multiple of the cycle, not of 32 -- past 2^16 visits in one cell: bit for bit against the oracle."""
    from th_rl_amd.batched import GameBatch
    probe = GameBatch(CYCLE, n_games=1, kernel="wave")
    assert probe.L.thrl_training_cycle(ctypes.byref(probe.cfg)) == 2
    _qtable_long_launch(CYCLE, 96, 1350, "float32", "wave", seed=14)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_tuple_kernel_counters_past_16_bits_three_players_vs_oracle(dtype):
    """k_tuple_episodes, three agents, T = 25: 2,700 episodes (85 launches of <= 32) put 67,500 steps on each game,
    past 2^16 visits in one cell: bit for bit against the oracle."""
    _qtable_long_launch(THREE, 96, 2700, dtype, "tuple", seed=5)


# ---------------------------------------------------------------- QTable vs a frozen neural agent: ptuple vs k_mixed_wave
def _mixed_pair(config, G, dtype, seed):
    """Two batches with the same network init and the same dominant-action tables; the second keeps the general kernel."""
    from th_rl_amd.mixed import MixedGameBatch
    out = []
    for tuple_kernel in (True, False):
        mb = MixedGameBatch(config, n_games=G, dtype=dtype, seed=seed).init_tables()
        qi = [i for i in range(mb.N) if mb.kinds[i] == "QTable"]
        mb.set_tables(_dominant(mb.tables_numpy(), mb.offsets, mb.shapes, qi, seed), mb.states_numpy())
        mb.tuple_kernel = tuple_kernel
        out.append(mb)
    a, b = out
    for i in a.nn:
        assert np.array_equal(a.nn[i].params.cpu().numpy(), b.nn[i].params.cpu().numpy())
    return a, b


def _assert_same_mixed(a, b, E, ra=None, rb=None):
    T = a.T
    qi = [i for i in range(a.N) if a.kinds[i] == "QTable"]
    for m in (a, b):
        c = m.counters_numpy()
        for i in qi:
            # one visit per step: a 16-bit cell that wraps leaves the sum 65,535 (low half: its carry lands in the
            # neighbouring cell) or 65,536 (high half: the carry leaves the dword) short per wrap
            assert (_qtable_visits(c, m.offsets, m.shapes, i).sum(axis=1, dtype=np.int64) == E * T).all(), \
                (i, sorted(set(_qtable_visits(c, m.offsets, m.shapes, i).sum(axis=1).tolist()) - {E * T}))
    assert int(b.counters_numpy().max()) > U16, "the regime the test exists for: > 65,535 visits in one cell"
    assert np.array_equal(a.counters_numpy(), b.counters_numpy())
    assert np.array_equal(a.tables_numpy(), b.tables_numpy())
    assert np.array_equal(a.states_numpy(), b.states_numpy())
    assert a.eps == b.eps and a.count == b.count and a.episode == b.episode == E
    for i in a.nn:
        assert a.nn[i].step == b.nn[i].step == 0                              # frozen: never trained
    if ra is not None:
        assert np.array_equal(ra["game_reward_log"], rb["game_reward_log"])
        assert np.array_equal(ra["game_action_log"], rb["game_action_log"])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("noise", [0.0, 0.05])
@pytest.mark.parametrize("opponent", ["reinforce", "actorcritic"])
def test_policy_tuple_kernel_counters_past_16_bits_in_one_launch(opponent, noise, dtype):
    """k_ptuple_episodes: a greedy QTable agent against a frozen Reinforce / ActorCritic, T = 100 and 760 episodes in ONE
    launch (76,000 steps per game): against k_mixed_wave, which counts in int32 -- counters (summing to E * T per game),
    tables, state, epsilon and per-game logs bit for bit.  With noise the off-grid steps visit other rows."""
    if opponent == "actorcritic" and dtype == "float64":
        pytest.skip("the ActorCritic pairing in float32 is enough")
    opp = FROZEN_R if opponent == "reinforce" else FROZEN_AC
    config = {"agents": [dict(CFG_AGENT), dict(opp)], "environment": dict(CFG_ENV, noise_prob=noise)}
    G, E = 24, 760
    a, b = _mixed_pair(config, G, dtype, seed=9)
    ra = a.run(E, fused=True)
    rb = b.run(E, fused=True)
    assert ra["episode_kernel"] == "tuple" and rb["episode_kernel"] == "wave"
    _assert_same_mixed(a, b, E, ra, rb)


def _mixed_episodes_direct(mb, E, flags):
    """One raw thrl_mixed_episodes call of E episodes (no cut by the caller), as MixedGameBatch fills the arguments."""
    import torch
    from th_rl_amd import _lib
    N, G = mb.N, mb.G
    rlog = torch.zeros((E, N, G), dtype=torch.float64, device=mb.device)
    alog = torch.zeros((E, N, G), dtype=torch.float64, device=mb.device)
    scratch = [torch.zeros_like(b["price"]) if mb.kinds[i] == "QTable" else None for i, b in enumerate(mb.buf)]
    mx = _lib.Mixed()
    for i in range(N):
        mx.kind[i] = {"QTable": 0, "Reinforce": 1, "ActorCritic": 2}[mb.kinds[i]]
        if mb.kinds[i] != "QTable":
            mx.nn_params[i] = mb.nn[i].params.data_ptr()
        b = mb.buf[i]
        mx.buf_price[i], mx.buf_action[i] = b["price"].data_ptr(), b["action"].data_ptr()
        mx.buf_reward[i], mx.buf_nprice[i] = b["reward"].data_ptr(), b["nprice"].data_ptr()
        if scratch[i] is not None:
            mx.buf_scratch[i] = scratch[i].data_ptr()
        mx.buf_len[i], mx.min_memory[i], mx.count[i] = mb.buf_len[i], mb.min_memory[i], mb.count[i]
    need = int(mb.L.thrl_mixed_policy_table_bytes(ctypes.byref(mb.cfg), ctypes.byref(mx)))
    ptab = torch.empty((max(need, 4) // 4,), dtype=torch.float32, device=mb.device)
    if need:
        mx.policy_tab, mx.policy_tab_bytes = ptab.data_ptr(), ptab.numel() * 4
    mx.flags = flags
    r = _lib.Run()
    r.seed, r.game_offset, r.first_episode, r.n_episodes = mb.seed, mb.game_offset, 0, E
    for i in range(N):
        r.eps[i] = mb.eps[i]
    _lib.check(mb.L.thrl_mixed_episodes(ctypes.byref(mb.cfg), ctypes.byref(mx), mb._p(mb.q), mb._p(mb.counter),
                                        mb._p(mb.state), ctypes.byref(r), mb._p(rlog), mb._p(alog),
                                        ctypes.c_void_p(torch.cuda.current_stream(mb.device).cuda_stream)),
               "thrl_mixed_episodes")
    torch.cuda.synchronize(mb.device)
    return r.kernel_used, [r.eps[i] for i in range(N)], rlog.cpu().numpy(), alog.cpu().numpy()


def test_mixed_episodes_c_abi_one_call_of_76800_steps():
    """thrl_mixed_episodes called directly with T = 256 and 300 episodes (76,800 steps per game in one call): the
    tuple-chain kernel against the same call with THRL_MIXED_NO_TUPLE_KERNEL -- counters, tables, state, epsilon, logs."""
    from th_rl_amd import _lib
    # (the ring must hold an episode for the tuple-chain kernel: capacity 300 >= T, still < min_memory)
    config = {"agents": [dict(CFG_AGENT, capacity=500, min_memory=100), dict(FROZEN_R, capacity=300, min_memory=600)],
              "environment": dict(CFG_ENV, max_steps=256)}
    E = 300
    a, b = _mixed_pair(config, 16, "float32", seed=21)
    ka, ea, ra, aa = _mixed_episodes_direct(a, E, 0)
    kb, eb, rb, ab = _mixed_episodes_direct(b, E, 1)                          # THRL_MIXED_NO_TUPLE_KERNEL
    assert ka == _lib.KERNEL_TUPLE and kb != _lib.KERNEL_TUPLE
    assert ea == eb
    a.episode = b.episode = E
    _assert_same_mixed(a, b, E)
    assert np.array_equal(ra, rb) and np.array_equal(aa, ab)


def test_train_one_frozen_reinforce_counters_past_16_bits(tmp_path, monkeypatch):
    """train_one on the reference's example pairing with a frozen Reinforce (capacity < min_memory), resumed from a
    near-greedy checkpoint: print_freq 700 makes each launch 70,000 steps.  The saved 0_counter.npy sums to
    epochs * max_steps and equals the same run on the general fused kernel."""
    import torch
    from th_rl_amd import trainer
    from th_rl_amd.mixed import MixedGameBatch
    epochs = 1400
    config = {"agents": [dict(CFG_AGENT), dict(FROZEN_R, action_range=[0.3, 0.3005])], "environment": dict(CFG_ENV)}
    mb = MixedGameBatch(config, n_games=1, dtype="float64", seed=1).init_tables()
    mb.set_tables(_dominant(mb.tables_numpy(), mb.offsets, mb.shapes, [0], 1), mb.states_numpy())
    ckpt = str(tmp_path / "start.pt")
    mb.save(ckpt)
    p = tmp_path / "config.json"
    p.write_text(json.dumps(dict(config, training={"print_freq": 700, "epochs": epochs, "seed": 1, "resume": ckpt})))

    kernels = []
    run0 = MixedGameBatch.run

    def run(self, *args, **kw):
        out = run0(self, *args, **kw)
        kernels.append(out["episode_kernel"])
        return out
    monkeypatch.setattr(MixedGameBatch, "run", run)
    np.random.seed(0); torch.manual_seed(0)
    trainer.train_one(str(tmp_path / "tuple"), str(p))
    assert kernels == ["tuple", "tuple"]

    init0 = MixedGameBatch.__init__

    def init(self, *args, **kw):
        init0(self, *args, **kw)
        self.tuple_kernel = False
    monkeypatch.setattr(MixedGameBatch, "__init__", init)
    np.random.seed(0); torch.manual_seed(0)
    trainer.train_one(str(tmp_path / "general"), str(p))
    assert kernels[2:] == ["wave", "wave"]

    ca = np.load(str(tmp_path / "tuple" / "0_counter.npy"))
    cb = np.load(str(tmp_path / "general" / "0_counter.npy"))
    assert cb.max() > U16, "the regime the test exists for: > 65,535 visits in one cell"
    assert ca.sum() == epochs * 100 and cb.sum() == epochs * 100
    assert np.array_equal(ca, cb)
    assert np.array_equal(np.load(str(tmp_path / "tuple" / "0.npy")), np.load(str(tmp_path / "general" / "0.npy")))
    with open(str(tmp_path / "tuple" / "log.csv")) as fa, open(str(tmp_path / "general" / "log.csv")) as fb:
        assert fa.read() == fb.read()


# ---------------------------------------------------------------- one input, one answer regardless of kernel
@pytest.mark.parametrize("kernel", ["tuple", "wave", "auto"])
@pytest.mark.parametrize("config", ["two", "three"])
def test_noise_prob_sweep_without_noise_is_refused_by_every_kernel(config, kernel):
    """A noise_prob sweep with cfg.noise_prob == 0 cannot switch the noise draws on: every kernel refuses it with
    THRL_ERR_BAD_CONFIG before any launch, instead of one of them running the config noise-free."""
    from th_rl_amd import _lib
    from th_rl_amd.batched import GameBatch
    cfg = dict(WAVE) if config == "two" else dict(THREE)
    if config == "three" and kernel == "wave":
        pytest.skip("the wave kernel takes two agents")
    G = 8
    gb = GameBatch(cfg, n_games=G, kernel=kernel, seed=3, sweep=dict(noise_prob=np.full(G, 0.1))).init_tables()
    q0, c0, s0 = gb.tables_numpy(), gb.counters_numpy(), gb.states_numpy()
    with pytest.raises(_lib.ThrlError, match="sweep_noise_prob") as ei:
        gb.run(2)
    assert ei.value.code == -1                                                # THRL_ERR_BAD_CONFIG
    assert np.array_equal(gb.tables_numpy(), q0) and np.array_equal(gb.counters_numpy(), c0)
    assert np.array_equal(gb.states_numpy(), s0) and gb.episode == 0
