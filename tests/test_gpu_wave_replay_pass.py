"""The wave kernel's replay by per-lane pass number against the C oracle, bit for bit.

Every group of four transitions carries one of 8 cut patterns (bit j-1: transition j may not share a pass with the
transitions in front of it).  Injected draws place each pattern in group 0, in group 7 (the last of a 32-transition
block), in the last group of the first segment and in the episode's last group; the other cases run the shared replay code
through ragged cycles, the three row-read widths, a training cycle that drops transitions at every position of a
group, noise, the greedy variant's in-register groups, a per-game alpha and a wave's second game.

Cut patterns in the oracle's own trajectory of test_cut_patterns_at_block_and_segment_edges (counted on the CPU from
the trace before the kernel was run; the same for both dtypes, the draws are injected; 64 games, 7 episodes, 25
groups each = 11,200 groups):
    pattern   0     1    2    3    4    5    6    7
    groups  9632  224  224  224  224  224  224  224
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
DTYPES = ["float32", "float64"]
PLACES = (0, 28, 60, 96)          # group 0, group 7 of its block, last group of segment 0, last group of the episode


def _config(T=100, A=21, eps=0.5, noise=0.0, **agent_kw):
    ag = dict(AGENT, actions=A, epsilon=eps, eps_end=min(eps, 0.001), min_memory=min(T, 100))
    ag.update(agent_kw)
    return {"agents": [dict(ag), dict(ag, alpha=0.3)], "environment": dict(ENV, max_steps=T, noise_prob=noise)}


def _batch(config, G, dtype, seed=0, **kw):
    from th_rl_amd.batched import GameBatch
    return GameBatch(config, n_games=G, dtype=dtype, kernel="wave", seed=seed, **kw)


def _row_of_price(cfg, price):
    return min(max(O.encode64(price, cfg.max_state[0], cfg.n_states[0]), 0), cfg.n_states[0])


def _price_of_pair(cfg, pair, A=21):
    sc = [O.scale(pair[0], A, cfg.act_lo[0], cfg.act_hi[0]), O.scale(pair[1], A, cfg.act_lo[1], cfg.act_hi[1])]
    return O.env_step(cfg, sc)[0]


def _hazard(wi, wj):
    """Transition j (later) may not share a pass with transition i (earlier): it reads the row i writes, or
    rewrites one of i's cells.  Words are (a0, a1, row, next_row)."""
    return wj[3] == wi[2] or (wj[2] == wi[2] and (wj[0] == wi[0] or wj[1] == wi[1]))


def _cut_pattern(words):
    """Cut bits of one group of (up to) four transitions: bit j-1 = a new pass starts in front of transition j."""
    bits, start = 0, 0
    for j in range(1, len(words)):
        if any(_hazard(words[i], words[j]) for i in range(start, j)):
            bits, start = bits | (1 << (j - 1)), j
    return bits


def _filler(T):
    """Action pairs without any hazard inside a group of four: the next row is a function of a0 + a1, and the sums
    7t mod 41 differ over any six consecutive steps; so do both agents' actions."""
    s = (7 * np.arange(T) + 3) % 41
    return np.stack([s // 2, s - s // 2], axis=1).astype(np.int64)


def _with_pattern(pattern, T=100):
    """The filler with `pattern` in the groups that start at PLACES: transition j repeats the pair played two steps
    earlier, so it leads into the row transition j-1 is played in (the row j-1 writes).  The step in front of step 0
    is the last step of the episode before (the game starts at that pair's price), so the last group is edited first."""
    a = _filler(T)
    for t0 in sorted(PLACES, reverse=True):
        for j in range(1, 4):
            if (pattern >> (j - 1)) & 1:
                a[t0 + j] = a[(t0 + j - 2) % T]
    return a


def _trace_patterns(cfg, oo, s0, games):
    """Cut pattern of every group the oracle played: [E, games, groups] from its trace (rows by the float64 encode)."""
    ta, tp = oo["trace_actions"], oo["trace_price"]
    E, T = ta.shape[0], ta.shape[1]
    out = np.zeros((E, len(games), (T + 3) // 4), np.int64)
    for gi, g in enumerate(games):
        row = _row_of_price(cfg, float(s0[g]))
        for e in range(E):
            words = []
            for t in range(T):
                nxt = _row_of_price(cfg, float(tp[e, t, g]))
                words.append((int(ta[e, t, 0, g]), int(ta[e, t, 1, g]), row, nxt))
                row = nxt
            for k in range(0, T, 4):
                out[e, gi, k // 4] = _cut_pattern(words[k:k + 4])
    return out


def _same(gb, q, c, s, label=""):
    bad = np.flatnonzero((gb.tables_numpy() != q).any(axis=1))
    assert bad.size == 0, "%s: tables of %d games differ (first %s)" % (label, bad.size, bad[:5])
    badc = np.flatnonzero((gb.counters_numpy() != c).any(axis=1))
    assert badc.size == 0, "%s: counters of %d games differ (first %s)" % (label, badc.size, badc[:5])
    assert np.array_equal(gb.states_numpy(), s), label


def _against_oracle(config, G, calls, dtype, seed, sweep=None):
    """One run() call per entry of `calls` on the wave kernel and on the oracle (own draws), compared after every call."""
    gb = _batch(config, G, dtype, seed=seed)
    if sweep:
        gb.set_sweep(sweep)
    gb.init_tables()
    q = gb.tables_numpy().copy(); s = gb.states_numpy().copy(); c = np.zeros(q.shape, np.int32)
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    osw = {k: v.cpu().numpy().copy() for k, v in gb.sweep.items()} if sweep else None
    mem, first = O.Memory(cfg), 0
    for k, E in enumerate(calls):
        label = "call %d (%d episodes)" % (k, E)
        out = gb.run(E)
        assert out["kernel"] == "wave", label
        oo = O.episodes(cfg, q, c, s, eps, mem, E, seed=seed, first_episode=first, **(dict(sweep=osw) if osw else {}))
        first += E
        _same(gb, q, c, s, label)
        np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13, err_msg=label)
        np.testing.assert_allclose(out["action_log"], oo["action_log"], rtol=1e-12, atol=1e-13, err_msg=label)
    return cfg


@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_patterns_at_block_and_segment_edges(dtype):
    """All 8 cut patterns in group 0, group 7, the last group of a segment and the last group of the episode: game g
    carries pattern g % 8, on its own random tables; every episode replays on tables the one before has written.
    Fails unless the oracle's trajectory holds each pattern at least 20 times."""
    config = _config()
    G, E, T = 64, 7, 100
    cfg0, _ = O.cfg_from_config(config, G, 1)
    gb = _batch(config, G, dtype, seed=5).init_tables()
    q0 = gb.tables_numpy().copy()
    actions = np.stack([_with_pattern(g % 8) for g in range(G)])
    s0 = np.array([_price_of_pair(cfg0, actions[g, T - 1]) for g in range(G)])
    u = np.zeros((E, T, 2, G))                                             # u = 0: everybody explores, with the injected action
    ch = np.ascontiguousarray(np.broadcast_to(np.transpose(actions, (1, 2, 0))[None], (E, T, 2, G)).astype(np.int8))
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    q = q0.copy(); c = np.zeros(q.shape, np.int32); s = s0.copy()
    oo = O.episodes(cfg, q, c, s, eps, O.Memory(cfg), E, inj_u=u, inj_choice=ch, trace=True)
    pat = _trace_patterns(cfg, oo, s0, range(G))
    for g in range(G):                                                      # the fixtures do what they say, in every episode
        for t0 in PLACES:
            assert (pat[:, g, t0 // 4] == g % 8).all(), (g, t0, pat[:, g, t0 // 4])
    counts = np.bincount(pat.ravel(), minlength=8)
    print("cut patterns 0..7 in the oracle's trajectory:", counts.tolist())
    assert (counts >= 20).all(), counts
    gb.set_tables(q0, s0)
    out = gb.run(E, inj=dict(u=u, choice=ch))
    assert out["kernel"] == "wave"
    _same(gb, q, c, s)
    np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 3, 5, 33, 63, 65, 100])
def test_partial_groups_and_blocks(dtype, T):
    _against_oracle(_config(T=T), G=64, calls=(3,), dtype=dtype, seed=21 + T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A", [2, 21, 32])
def test_row_read_widths(dtype, A):
    """2, 3 and 4 row reads per lane (A = 2, A <= 24, A > 24)."""
    _against_oracle(_config(A=A), G=64, calls=(3,), dtype=dtype, seed=50 + A)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("capacity", [61, 62, 63, 64])
def test_training_cycle_drops_transitions_at_every_position(dtype, capacity):
    """The deque holds the last `capacity` of the cycle's 100 transitions: the replay starts at step 39, 38, 37, 36,
    i.e. at position 3, 2, 1, 0 of a group."""
    cfg = _against_oracle(_config(capacity=capacity, min_memory=capacity), G=64, calls=(3, 2), dtype=dtype, seed=60 + capacity)
    assert int(cfg.capacity[0]) == capacity


@pytest.mark.parametrize("dtype", DTYPES)
def test_noise(dtype):
    _against_oracle(_config(noise=0.5), G=64, calls=(4,), dtype=dtype, seed=35)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("eps", [0.0, 0.02])
def test_greedy_variant(dtype, eps):
    """Hardly anybody explores: fixed points and period-2 groups run in registers, the others take the passes."""
    _against_oracle(_config(eps=eps), G=96, calls=(4, 3), dtype=dtype, seed=70)


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_game_alpha(dtype):
    G = 96
    rs = np.random.RandomState(5)
    _against_oracle(_config(), G=G, calls=(3,), dtype=dtype, seed=41, sweep=dict(alpha=rs.choice([0.05, 0.1, 0.5], (2, G))))


def test_more_games_than_resident_waves():
    """A wave's second game: keys and addresses of the first game's last segment are not carried over."""
    import torch
    resident = 20 * torch.cuda.get_device_properties(0).multi_processor_count
    G = resident + resident // 4
    assert G <= 8000, G
    _against_oracle(_config(), G=G, calls=(2,), dtype="float32", seed=3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_consecutive_calls(dtype):
    _against_oracle(_config(), G=300, calls=(4, 3), dtype=dtype, seed=99)
