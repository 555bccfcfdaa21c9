"""The wave kernel's per-game phases around the episode loop against the C oracle: the table stream-in, the stream-out,
the log read-back into the visit histogram and the counter apply, which adds the histogram's non-zero cells to the
game's counters with no-return atomic adds (no load of the old counts).

Every case forces the wave kernel and compares tables, visit counters (of EVERY game), env states and epsilon with
np.array_equal after every call.  The logs are held to the suite's standing rtol 1e-12 / atol 1e-13:
tests/test_gpu_wave_cell_log.py says why they cannot be bit-equal (fixed-point sums per wave against the oracle's double
sums in game order).  Each figure is printed before it is asserted.

Window sizes: n = win_rows * actions elements per agent, chosen around the strides of the stream loops (64 elements per
pass, 512 per batch of loads) and around every residue of 4.  With 100 states the window of a symmetric game has an odd
number of rows, so the two multiples of 64 take another `states` as well as other `actions` / `action_range`."""
import numpy as np
import pytest

import limits_table as LT

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)


def _config(T=100, A=21, eps=0.5, noise=0.0, **agent_kw):
    ag = dict(AGENT, actions=A, epsilon=eps, eps_end=min(eps, 0.001), min_memory=min(T, 100))
    ag.update(agent_kw)
    return {"agents": [dict(ag), dict(ag, alpha=0.3)], "environment": dict(ENV, max_steps=T, noise_prob=noise)}


def _logs(got, want, label):
    print("%s: logs max |diff| %.3g, identical %s" % (label, float(np.abs(got - want).max()), np.array_equal(got, want)))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13, err_msg=label)


def _against_oracle(config, G, calls, dtype="float32", seed=7, prepare=None, per_game_logs=False, counters=True, sweep=None):
    """One run() call per entry of `calls` on the forced wave kernel and on the oracle, compared after every call.
    prepare(q, c, s, gb) edits the start tables, counters and states in place before the first call.  Returns the oracle's
    final (q, c, s) and the start (q0, c0, s0)."""
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel="wave", seed=seed, counters=counters)
    if sweep:
        gb.set_sweep(sweep)
    gb.init_tables()
    q = gb.tables_numpy().copy(); s = gb.states_numpy().copy()
    c = np.zeros(q.shape, np.int32)
    if prepare is not None:
        prepare(q, c, s, gb)
        gb.set_tables(q, s, counter=c if counters else None)
    q0, c0, s0 = q.copy(), c.copy(), s.copy()
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    osw = {k: v.cpu().numpy().copy() for k, v in gb.sweep.items()} if sweep else None    # (the oracle updates eps in place)
    mem, first = O.Memory(cfg), 0
    for k, E in enumerate(calls):
        label = "call %d (%d episodes)" % (k, E)
        out = gb.run(E, per_game_logs=per_game_logs)
        assert out["kernel"] == "wave", label
        kw = dict(sweep=osw) if osw is not None else {}
        oo = O.episodes(cfg, q, c, s, eps, mem, E, seed=seed, first_episode=first, **kw)
        first += E
        bad = np.flatnonzero((gb.tables_numpy() != q).any(axis=1))
        assert bad.size == 0, "%s: tables of %d games differ (first %s)" % (label, bad.size, bad[:5])
        if counters:
            badc = np.flatnonzero((gb.counters_numpy() != c).any(axis=1))
            assert badc.size == 0, "%s: counters of %d games differ (first %s)" % (label, badc.size, badc[:5])
        assert np.array_equal(gb.states_numpy(), s), label
        if osw is not None and "eps" in osw:
            assert np.array_equal(gb.sweep["eps"].cpu().numpy(), osw["eps"]), label
        else:
            assert [float(x) for x in gb.eps[:2]] == [float(x) for x in eps[:2]], label
        _logs(out["reward_log"], oo["reward_log"], label)
        _logs(out["action_log"], oo["action_log"], label)
        if per_game_logs:
            _logs(out["game_reward_log"], oo["game_reward_log"], label)
            _logs(out["game_action_log"], oo["game_action_log"], label)
    return (q, c, s), (q0, c0, s0)


def _offsets(config):
    from th_rl_amd.batched import GameBatch
    return GameBatch(config, n_games=1, kernel="wave").offsets


# ---- window sizes: (agent settings, expected n, what it is there for)
WINDOWS = {
    "n22":  (dict(A=2, action_range=[0.25, 0.3]), 22),              # less than one pass of 64
    "n42":  (dict(A=2, action_range=[0.2, 0.3]), 42),               # less than one pass; 84 dwords in float64
    "n63":  (dict(A=3, action_range=[0.2, 0.3]), 63),               # = 3 (mod 4), one below the threshold
    "n64":  (dict(A=2, action_range=[0.2, 0.33], states=120), 64),  # exactly one pass
    "n66":  (dict(A=2, action_range=[0.2, 0.36]), 66),              # = 2 (mod 4); two lanes in the last pass
    "n129": (dict(A=3, action_range=[0.2, 0.41]), 129),             # = 1 (mod 4) and = 1 (mod 64): one lane in the last pass
    "n256": (dict(A=16, action_range=[0.2, 0.35], states=50), 256),  # a multiple of 64: no partial pass
    "n287": (dict(A=7, action_range=[0.2, 0.4]), 287),              # = 3 (mod 4)
    "n861": (dict(A=21), 861),                                      # the headline window
}


@pytest.mark.parametrize("calls", [(1,), (5, 3)], ids=["1", "5+3"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("win", sorted(WINDOWS))
def test_window_sizes(win, dtype, calls):
    kw, n = WINDOWS[win]
    config = _config(**kw)
    lo, W, inside = LT.window(config, 0)
    assert W * config["agents"][0]["actions"] == n and inside
    (q, c, s), _ = _against_oracle(config, G=192, calls=calls, dtype=dtype, seed=50 + n)
    assert int(c.sum()) == 192 * 2 * sum(calls) * 100


# ---- neighbours: sentinels in every row outside the window, tables and counters, every game, both agents
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("win", ["n66", "n129", "n861"])
def test_rows_outside_the_window_keep_their_sentinels(win, dtype):
    kw, n = WINDOWS[win]
    config = _config(**kw)
    A, S = config["agents"][0]["actions"], config["agents"][0]["states"]
    lo, W, _ = LT.window(config, 0)
    offs = _offsets(config)
    assert offs[1] % 2 == 1 or A % 2 == 0                         # agent 1's table starts at an odd element where A is odd

    def prepare(q, c, s, gb):
        G = q.shape[0]
        for off in offs:
            tq = q[:, off:off + (S + 1) * A].reshape(G, S + 1, A)
            tc = c[:, off:off + (S + 1) * A].reshape(G, S + 1, A)
            rows = np.r_[0:lo, lo + W:S + 1]
            sent = (np.arange(G)[:, None, None] * 1000003 + rows[None, :, None] * 101 + np.arange(A)[None, None, :] + off)
            tq[:, rows] = -1.0 - (sent % 65521) / 65536.0          # distinct negative values: never a row maximum inside
            tc[:, rows] = 1 + sent % 1000003

    (q, c, s), (q0, c0, s0) = _against_oracle(config, G=192, calls=(3, 2), dtype=dtype, seed=61, prepare=prepare)
    # the device equals the oracle's (q, c) by the comparison above; rows that no transition touched (no visit counted)
    # still hold what they held before the run
    G = q.shape[0]
    rows = np.r_[0:lo, lo + W:S + 1]
    for off in offs:
        t, t0 = (x[:, off:off + (S + 1) * A].reshape(G, S + 1, A)[:, rows] for x in (q, q0))
        u, u0 = (x[:, off:off + (S + 1) * A].reshape(G, S + 1, A)[:, rows] for x in (c, c0))
        untouched = (u == u0).all(axis=2)
        assert untouched.mean() > 0.9
        assert np.array_equal(t[untouched], t0[untouched])
        assert (c[:, off + lo * A:off + (lo + W) * A] != c0[:, off + lo * A:off + (lo + W) * A]).any()


# ---- spill rows: entry prices outside the window, play row != train row
def _rows(cfg, price):
    ms, n = cfg.max_state[0], cfg.n_states[0]
    clip = lambda r: min(max(r, 0), n)
    return clip(O.encode32(price, ms, n)), clip(O.encode64(price, ms, n))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_both_spill_rows_live(dtype):
    config = _config()
    cfg, _ = O.cfg_from_config(config, 1, 0)
    lo, hi = 20, 60
    prices = []
    for r in list(range(0, lo - 1)) + list(range(hi + 1, cfg.n_states[0])):
        edge = (r + 0.5) * cfg.max_state[0] / cfg.n_states[0]
        for p in (edge, np.nextafter(edge, 0.0), np.nextafter(edge, 100.0),
                  float(np.nextafter(np.float32(edge), np.float32(0.0))), float(np.nextafter(np.float32(edge), np.float32(100.0)))):
            r32, r64 = _rows(cfg, p)
            if r32 != r64 and not (lo <= r32 <= hi) and not (lo <= r64 <= hi):
                prices.append(p)
    assert len(prices) >= 16
    G, E = 64, 3
    s_entry = np.resize(np.array(prices, np.float64), G)

    def prepare(q, c, s, gb):
        s[:] = s_entry
        c[:] = 7                                                   # the spill-row adds land on counters that are not zero

    (q, c, s), (q0, c0, s0) = _against_oracle(config, G=G, calls=(E,), dtype=dtype, seed=13, prepare=prepare)
    A, stride_rows = 21, cfg.n_states[0] + 1
    for g in range(G):
        r32, r64 = _rows(cfg, float(s_entry[g]))
        for off in _offsets(config):
            t = (c - c0)[g, off:off + stride_rows * A].reshape(stride_rows, A)
            assert t[r64].sum() == 1 and t[r32].sum() == 0, (g, r32, r64)   # trained once, in the train row only
            assert t[lo:hi + 1].sum() == E * 100 - 1


# ---- LDS reuse: a wave's second game sees neither the first game's histogram nor a late load
def test_more_games_than_resident_waves():
    import torch
    resident = 20 * torch.cuda.get_device_properties(0).multi_processor_count
    G = resident + resident // 4
    assert G <= 8000, G
    (q, c, s), _ = _against_oracle(_config(), G=G, calls=(2,), seed=3)
    assert int(c.sum()) == G * 2 * 2 * 100


# ---- counters: one cell collects every visit of the launch, on top of counters that are not zero
def _converged(config, a0=3, a1=5):
    """Tables on which greedy play repeats one action pair for ever: 100 in column a_i of every row, 0 elsewhere (the cell
    that is rewritten only moves towards reward / (1 - gamma) > 0), and every game starts at that pair's price."""
    A = config["agents"][0]["actions"]
    price = float(LT.prices(config)[a0 * A + a1])

    def prepare(q, c, s, gb):
        S = config["agents"][0]["states"]
        q[:] = 0.0
        for off, col in zip(gb.offsets, (a0, a1)):
            q[:, off:off + (S + 1) * A].reshape(q.shape[0], S + 1, A)[:, :, col] = 100.0
        s[:] = price
        c[:] = (np.arange(c.size, dtype=np.int64).reshape(c.shape) * 7919 % 100003 + 1).astype(np.int32)
    return prepare


@pytest.mark.parametrize("E", [1, 4, 5, 8, 9, 32])
def test_one_cell_collects_every_visit(E):
    config = _config(eps=0.0)
    (q, c, s), (q0, c0, s0) = _against_oracle(config, G=96, calls=(E, E), seed=70 + E, prepare=_converged(config))
    d = (c - c0).astype(np.int64)
    A, S = 21, 100
    for off in _offsets(config):
        t = d[:, off:off + (S + 1) * A]
        assert (t.max(axis=1) == 2 * E * 100).all() and (t.sum(axis=1) == 2 * E * 100).all()


def test_without_counters():
    _against_oracle(_config(), G=96, calls=(4, 3), seed=38, counters=False)


# ---- the other instantiations share the code: one case each
def test_noise():
    _against_oracle(_config(noise=0.05), G=96, calls=(4, 3), seed=35)


def test_training_cycle_of_two_episodes():
    config = _config(T=50, min_memory=100)
    assert LT.cycle(config) == (2, 100)
    (q, c, s), _ = _against_oracle(config, G=96, calls=(6, 2), seed=31)
    assert int(c.sum()) == 96 * 2 * 4 * 100


def test_per_game_logs():
    _against_oracle(_config(), G=96, calls=(4, 3), seed=37, per_game_logs=True)


def test_sweep_with_per_game_alpha():
    G = 96
    rs = np.random.RandomState(5)
    _against_oracle(_config(), G=G, calls=(4, 3), seed=41, sweep=dict(alpha=rs.choice([0.05, 0.1, 0.5], (2, G))))
