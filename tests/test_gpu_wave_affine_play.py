"""The wave kernel's closed-form play tables (affine payoff grids) against the oracle, bit for bit: tables, visit
counters, states, epsilon and the mean logs.  Every case runs the plain float32 variant and asserts through
thrl_wave_play_form which play form it exercises; the same natural-draw and episode-length cases run again on a
16-action grid, which is not affine and so pins the payoff-LUT path of the same kernel family."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
LENGTHS = [1, 3, 4, 5, 36, 63, 64, 65, 100, 127, 128, 129, 256]


def _config(T=100, A=21, eps=0.5, range1=None):
    # epsilon 1.0 and 0.0 stay where they are (eps_end = epsilon): every step explores / nobody does
    ag = dict(AGENT, actions=A, epsilon=eps, eps_end=eps if eps in (0.0, 1.0) else 0.001, min_memory=min(T, 100))
    ag1 = dict(ag, alpha=0.3)
    if range1 is not None:
        ag1["action_range"] = range1
    return {"agents": [dict(ag), ag1], "environment": dict(ENV, max_steps=T)}


def _batch(config, G, seed=0):
    from th_rl_amd.batched import GameBatch
    return GameBatch(config, n_games=G, dtype="float32", kernel="wave_plain", seed=seed)


def _form(gb):
    out = (ctypes.c_int * 3)()
    return gb.L.thrl_wave_play_form(ctypes.byref(gb.cfg), ctypes.byref(out)), tuple(out)


def _against_oracle(config, G, E, form, calls=1, seed=0, s0=None, inj=None, per_game_logs=False):
    """`calls` calls of E episodes each on the plain float32 wave kernel and on the oracle; everything is compared after
    every call (the second call starts from the state the first has left)."""
    gb = _batch(config, G, seed).init_tables()
    assert _form(gb)[0] == form
    q = gb.tables_numpy().copy(); s = gb.states_numpy().copy()
    if s0 is not None:
        s = np.asarray(s0, np.float64).copy()
        gb.set_tables(q, s)
    cfg, eps = O.cfg_from_config(config, G, 0)
    c = np.zeros(q.shape, np.int32)
    mem = O.Memory(cfg)
    outs = []
    for k in range(calls):
        kw = dict(inj_u=inj["u"], inj_choice=inj["choice"]) if inj is not None else dict(seed=seed)
        out = gb.run(E, inj=inj, per_game_logs=per_game_logs)
        assert out["kernel"] == "wave"
        oo = O.episodes(cfg, q, c, s, eps, mem, E, first_episode=k * E, **kw)
        assert np.array_equal(gb.tables_numpy(), q), "tables, call %d" % k
        assert np.array_equal(gb.counters_numpy(), c), "counters, call %d" % k
        assert np.array_equal(gb.states_numpy(), s), "states, call %d" % k
        assert np.array_equal(np.array(gb.eps[:2]), eps[:2])
        np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(out["action_log"], oo["action_log"], rtol=1e-12, atol=1e-13)
        if per_game_logs:
            np.testing.assert_allclose(out["game_reward_log"], oo["game_reward_log"], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(out["game_action_log"], oo["game_action_log"], rtol=1e-12, atol=1e-13)
        outs.append(oo)
    return cfg, outs


# ---- natural draws, episode lengths: closed form (21 actions) and payoff LUT (16 actions)
@pytest.mark.parametrize("A,form", [(21, 1), (16, 0)])
@pytest.mark.parametrize("eps", [0.5, 1.0, 0.0])
def test_natural_draws(A, form, eps):
    _against_oracle(_config(A=A, eps=eps), G=128, E=3, form=form, calls=2, seed=11)


@pytest.mark.parametrize("A,form", [(21, 1), (16, 0)])
@pytest.mark.parametrize("T", LENGTHS)
def test_episode_lengths(A, form, T):
    _against_oracle(_config(T=T, A=A), G=64, E=2, form=form, calls=2, seed=21 + T)


def test_slopes_1_2():
    config = _config(range1=[0.1, 0.5])
    gb = _batch(config, 64)
    got, (c, m0, m1) = _form(gb)
    assert got == 1 and (m0, m1) == (1, 2)
    _against_oracle(config, G=128, E=3, form=1, calls=2, seed=5)


def test_per_game_logs():
    _against_oracle(_config(), G=64, E=3, form=1, calls=2, seed=9, per_game_logs=True)


# ---- entry states
def _rows(cfg, price):
    ms, n = cfg.max_state[0], cfg.n_states[0]
    clip = lambda r: min(max(r, 0), n)
    return clip(O.encode32(price, ms, n)), clip(O.encode64(price, ms, n))


def _window(cfg):
    """First and last row the payoff grid reaches (either encode)."""
    A = cfg.n_actions[0]
    rows = [_rows(cfg, O.env_step(cfg, [O.scale(a0, A, cfg.act_lo[0], cfg.act_hi[0]), O.scale(a1, A, cfg.act_lo[1], cfg.act_hi[1])])[0])
            for a0 in range(A) for a1 in range(A)]
    return int(np.min(rows)), int(np.max(rows))


def _split_prices(cfg, lo, hi):
    """Prices at which the float32 and the float64 encode give different rows: (inside the window, outside it)."""
    inside, outside = [], []
    for r in range(cfg.n_states[0]):
        edge = (r + 0.5) * cfg.max_state[0] / cfg.n_states[0]              # rows are rint(price / max_state * states)
        for p in (edge, np.nextafter(edge, 0.0), np.nextafter(edge, 100.0),
                  float(np.nextafter(np.float32(edge), np.float32(0.0))), float(np.nextafter(np.float32(edge), np.float32(100.0)))):
            r32, r64 = _rows(cfg, p)
            if r32 != r64:
                (inside if lo <= r32 <= hi and lo <= r64 <= hi else outside).append(p)
    return inside, outside


@pytest.mark.parametrize("range1", [None, [0.1, 0.5]])
def test_entry_states(range1):
    """The first step of a call starts from a continuous price: rows below and above the window (spill rows), and
    prices whose play (float32) and train (float64) rows differ, inside and outside the window.  The oracle moves by the
    play row and updates the train row; tables and counters must agree cell for cell."""
    config = _config(range1=range1)
    cfg, _ = O.cfg_from_config(config, 1, 0)
    lo, hi = _window(cfg)
    assert (lo, hi) == ((20, 60) if range1 is None else (10, 70))
    inside, outside = _split_prices(cfg, lo, hi)
    assert inside and outside
    below = [0.0, 0.5, (lo - 1) * 0.1]                    # rows 0, 5, lo - 1 (row r is centred on the price r / 10)
    above = [(hi + 1) * 0.1, 8.0, 9.9]                    # rows hi + 1, 80, 99
    assert [_rows(cfg, p) for p in below] == [(0, 0), (5, 5), (lo - 1, lo - 1)]
    assert [_rows(cfg, p) for p in above] == [(hi + 1, hi + 1), (80, 80), (99, 99)]
    edge = [lo * 0.1, hi * 0.1]                           # first and last row of the window
    assert [_rows(cfg, p) for p in edge] == [(lo, lo), (hi, hi)]
    prices = below + above + edge + inside[:12] + inside[-12:] + outside[:12] + outside[-12:]
    G = 64
    s0 = np.resize(np.array(prices, np.float64), G)
    _against_oracle(config, G=G, E=2, form=1, calls=1, seed=3, s0=s0)
    # and with nobody exploring, so that the first transition's rows alone decide where the episode goes
    cfg0 = _config(range1=range1, eps=0.0)
    _against_oracle(cfg0, G=G, E=2, form=1, calls=1, seed=3, s0=s0)


# ---- injected draws: who explores, where in a group of four, which bytes
GROUPS = [0, 28, 32, 60, 64, 96]


def _injected_cases(T=100):
    """One game per (who explores at the target step, position in the group, group, choice bytes): u [T, 2], choice [T, 2].
    Every other step explores with both agents on a spread of action pairs, so the neighbouring bytes of the packed words
    are busy; the target step's choices are 0 or 20, the ends of the constant byte's range."""
    s = (7 * np.arange(T) + 3) % 41
    base = np.stack([s // 2, s - s // 2], axis=1).astype(np.int8)
    us, chs = [], []
    for t0 in GROUPS:
        for pos in range(4):
            for ex0 in (0, 1):
                for ex1 in (0, 1):
                    for ch in ((0, 0), (20, 20)) if (pos + ex0 + ex1) % 2 == 0 else ((0, 20), (20, 0)):
                        u = np.zeros((T, 2)); c = base.copy()
                        u[t0 + pos] = (0.0 if ex0 else 1.0, 0.0 if ex1 else 1.0)
                        c[t0 + pos] = ch
                        us.append(u); chs.append(c)
    return np.stack(us), np.stack(chs)


@pytest.mark.parametrize("background", ["explore", "greedy"])
def test_injected_draws(background):
    """Each of the four who-explores categories at each position of the groups at steps 0, 28, 32, 60, 64 and 96, with
    choices 0 and 20 for either agent; against a background of exploring steps and of greedy steps."""
    T = 100
    config = _config(T=T)
    u, ch = _injected_cases(T)                                    # [G, T, 2]
    if background == "greedy":
        tgt = np.zeros(u.shape[:2], bool)
        k = 0
        for t0 in GROUPS:
            for pos in range(4):
                tgt[k:k + 8, t0 + pos] = True
                k += 8
        u = np.where(tgt[:, :, None], u, 1.0)
    G, E = u.shape[0], 2
    assert G == 192
    inj = dict(u=np.ascontiguousarray(np.broadcast_to(np.transpose(u, (1, 2, 0))[None], (E, T, 2, G))),
               choice=np.ascontiguousarray(np.broadcast_to(np.transpose(ch, (1, 2, 0))[None], (E, T, 2, G)).astype(np.int8)))
    _against_oracle(config, G=G, E=E, form=1, calls=1, seed=17, inj=inj)
