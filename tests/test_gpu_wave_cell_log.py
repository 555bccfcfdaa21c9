"""The wave kernel's per-game work around the episode loop against the C oracle, bit for bit: the transition log of cell
words, the 32-bit visit histogram built from it over the freed table region, the counter apply, the table stream-out and
the operand phase that feeds all of them (cell offsets, next row).

Every case forces the wave kernel and compares tables, visit counters (of EVERY game), env states and epsilon with
np.array_equal after every call.

The mean logs cannot be identical to the oracle's, before or after any change of the kernel: the kernel rounds each game's
episode value to a fixed-point integer and sums integers (the games a wave gets are not deterministic, integer sums do not
care), the oracle sums doubles in game order; both sum ~100 step values of magnitude <= 25 in another order.  Measured on
the commit before this file, over all cases below: max |kernel - oracle| = 3.4e-14 on the mean logs (values ~ 11) and
1.4e-14 on the per-game logs, 1 to 30 units in the last place; no case is identical.  They are held to the bound every
other oracle comparison of the suite uses, rtol 1e-12 / atol 1e-13: T * 2^-53 * |value| = 100 * 1.1e-16 * 25 = 2.8e-13 is the
reordering bound of one game's sum, the fixed-point quantum (2^-43 or finer for at most 8,000 games: thrl_api.hip, log_scale) lies far below it.  Each figure is
printed before it is asserted."""
import numpy as np
import pytest

import limits_table as LT

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)


def _config(T=100, A=21, eps=0.5, noise=0.0, **agent_kw):
    ag = dict(AGENT, actions=A, epsilon=eps, eps_end=min(eps, 0.001) if eps != 0.02 else eps, min_memory=min(T, 100))
    ag.update(agent_kw)
    return {"agents": [dict(ag), dict(ag, alpha=0.3)], "environment": dict(ENV, max_steps=T, noise_prob=noise)}


def _logs(got, want, label):
    """Mean / per-game logs: the module docstring says why these are held to a tolerance and to which."""
    print("%s: logs max |diff| %.3g, identical %s" % (label, float(np.abs(got - want).max()), np.array_equal(got, want)))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13, err_msg=label)


def _against_oracle(config, G, calls, dtype="float32", kernel="wave", seed=7, s0=None, per_game_logs=False, counters=True):
    """One run() call per entry of `calls` on the forced wave kernel and on the oracle, compared after every call (a later
    call reuses the wave's transition log and starts from what the earlier one left).  Returns the oracle's final
    (cfg, tables, counters, states)."""
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel=kernel, seed=seed, counters=counters).init_tables()
    q = gb.tables_numpy().copy(); s = gb.states_numpy().copy()
    if s0 is not None:
        s = np.asarray(s0, np.float64).copy()
        gb.set_tables(q, s)
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    c = np.zeros(q.shape, np.int32)
    mem, first = O.Memory(cfg), 0
    for k, E in enumerate(calls):
        label = "call %d (%d episodes)" % (k, E)
        out = gb.run(E, per_game_logs=per_game_logs)
        assert out["kernel"] == "wave", label
        oo = O.episodes(cfg, q, c, s, eps, mem, E, seed=seed, first_episode=first)
        first += E
        bad = np.flatnonzero((gb.tables_numpy() != q).any(axis=1))
        assert bad.size == 0, "%s: tables of %d games differ (first %s)" % (label, bad.size, bad[:5])
        if counters:
            badc = np.flatnonzero((gb.counters_numpy() != c).any(axis=1))
            assert badc.size == 0, "%s: counters of %d games differ (first %s)" % (label, badc.size, badc[:5])
        assert np.array_equal(gb.states_numpy(), s), label
        assert [float(x) for x in gb.eps[:2]] == [float(x) for x in eps[:2]], label
        _logs(out["reward_log"], oo["reward_log"], label)
        _logs(out["action_log"], oo["action_log"], label)
        if per_game_logs:
            _logs(out["game_reward_log"], oo["game_reward_log"], label)
            _logs(out["game_action_log"], oo["game_action_log"], label)
    return cfg, q, c, s


# ---- base: headline config; partial and full batches of four episodes in the read-back; the log is reused by a second call
@pytest.mark.parametrize("E", [1, 3, 4, 5, 32])
def test_headline_episode_counts(E):
    cfg, q, c, s = _against_oracle(_config(), G=192, calls=(E, E), seed=40 + E)
    assert int(c.sum()) == 192 * 2 * 2 * E * 100                  # every transition of both calls is one update per agent


def test_more_games_than_resident_waves():
    """Waves that finish early claim another game: the histogram is zeroed over the previous game's tables and built
    again from the same log rows.  The plan keeps 20 waves per CU resident in this shape (5 per SIMD), and nothing a test
    can set lowers that inside a running process, so the game count exceeds the whole grid; 2 episodes."""
    import torch
    resident = 20 * torch.cuda.get_device_properties(0).multi_processor_count
    G = resident + resident // 4
    assert G <= 8000, G
    cfg, q, c, s = _against_oracle(_config(), G=G, calls=(2,), seed=3)
    assert int(c.sum()) == G * 2 * 2 * 100


def _rows(cfg, price):
    ms, n = cfg.max_state[0], cfg.n_states[0]
    clip = lambda r: min(max(r, 0), n)
    return clip(O.encode32(price, ms, n)), clip(O.encode64(price, ms, n))


def test_initial_price_off_the_window_and_between_rows():
    """Entry prices outside the window whose float32 (play) and float64 (train) rows differ: both spill rows are in use
    and play row != train row in the first step.  The first transition's counters land in the TRAIN row, a spill row."""
    config = _config()
    cfg, _ = O.cfg_from_config(config, 1, 0)
    lo, hi = 20, 60                                               # the headline window (test_gpu_wave_affine_play.py)
    prices = []
    for r in list(range(0, lo - 1)) + list(range(hi + 1, cfg.n_states[0])):
        edge = (r + 0.5) * cfg.max_state[0] / cfg.n_states[0]
        for p in (edge, np.nextafter(edge, 0.0), np.nextafter(edge, 100.0),
                  float(np.nextafter(np.float32(edge), np.float32(0.0))), float(np.nextafter(np.float32(edge), np.float32(100.0)))):
            r32, r64 = _rows(cfg, p)
            if r32 != r64 and not (lo <= r32 <= hi) and not (lo <= r64 <= hi):
                prices.append(p)
    assert len(prices) >= 16
    G = 64
    s0 = np.resize(np.array(prices, np.float64), G)
    E = 3
    cfgG, q, c, s = _against_oracle(config, G=G, calls=(E,), seed=13, s0=s0)
    A, stride_rows = 21, cfg.n_states[0] + 1
    from th_rl_amd.batched import GameBatch
    offs = GameBatch(config, n_games=1, kernel="wave").offsets
    for g in range(G):
        r32, r64 = _rows(cfg, float(s0[g]))
        for off in offs:
            t = c[g, off:off + stride_rows * A].reshape(stride_rows, A)
            assert t[r64].sum() == 1 and t[r32].sum() == 0, (g, r32, r64)   # trained once, in the train row only
            assert t[lo:hi + 1].sum() == E * 100 - 1


# ---- one short segment, two full segments, a tail that is no multiple of four
@pytest.mark.parametrize("T", [30, 128, 7])
def test_episode_lengths(T):
    cfg, q, c, s = _against_oracle(_config(T=T), G=96, calls=(5, 3), seed=20 + T)
    assert int(c.sum()) == 96 * 2 * 8 * T


# ---- training cycles
def test_two_episodes_per_cycle():
    config = _config(T=50, min_memory=100)
    assert LT.cycle(config) == (2, 100)
    cfg, q, c, s = _against_oracle(config, G=96, calls=(6, 2), seed=31)
    assert int(c.sum()) == 96 * 2 * 4 * 100


def test_capacity_64_drops_the_first_36_transitions():
    config = _config(T=100, min_memory=64, capacity=64)
    assert LT.cycle(config) == (1, 64)                            # replay_from = 36 > 0
    cfg, q, c, s = _against_oracle(config, G=96, calls=(5, 4), seed=32)
    assert int(c.sum()) == 96 * 2 * 9 * 64                        # dropped transitions are not counted


# ---- float64: a block's eleven waves, LDS addresses above 64 KB
def test_float64_full_blocks():
    config = _config()
    assert 10 * LT.wave_game_lds_bytes(config, "float64") > 64 * 1024 > 4 * LT.wave_game_lds_bytes(config, "float64")
    cfg, q, c, s = _against_oracle(config, G=88, calls=(5, 3), dtype="float64", seed=33)
    assert int(c.sum()) == 88 * 2 * 8 * 100


# ---- the 126-row x 32-action plan: offsets at the top of the 16-bit field
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_largest_plan(dtype):
    config = LT.BY_ID["wave-rows-126-A32-f64"]["config"]
    m = LT.measure(LT.BY_ID["wave-rows-126-A32-f64"])
    assert (m["win_rows"], m["max_actions"]) == (126, 32)
    # entry prices below the table's first row do not exist here (the window is the whole table): start games at the top and
    # bottom rows so that the last window rows' cells (the largest offsets) are visited
    G = 48
    s0 = np.resize(np.array([0.0, 0.04, 9.96, 10.0, 5.0, 0.39]), G)
    cfg, q, c, s = _against_oracle(config, G=G, calls=(3, 2), dtype=dtype, seed=34, s0=s0)
    A = 32
    from th_rl_amd.batched import GameBatch
    offs = GameBatch(config, n_games=1, kernel="wave").offsets
    t1 = c[:, offs[1]:offs[1] + 126 * A].reshape(G, 126, A)
    assert t1[:, 125].sum() > 0 and t1[:, :, A - 1].sum() > 0     # agent 1's last row and last column were counted


# ---- one case each of the other code variants
def test_noise():
    _against_oracle(_config(noise=0.05), G=96, calls=(4, 3), seed=35)


def test_greedy_variant():
    cfg, q, c, s = _against_oracle(_config(eps=0.02), G=96, calls=(5, 3), kernel="wave_greedy", seed=36)
    assert (c.max(axis=1) >= 40).mean() > 0.3                     # the regime: one cell rewritten over and over


def test_per_game_logs():
    _against_oracle(_config(), G=96, calls=(4, 3), seed=37, per_game_logs=True)


def test_without_counters():
    _against_oracle(_config(), G=96, calls=(4, 3), seed=38, counters=False)


def test_non_affine_grid():
    _against_oracle(_config(A=16), G=96, calls=(5, 3), seed=39)
