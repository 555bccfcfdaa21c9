"""Closed-form play tables of the wave kernel, host side (no GPU): thrl_wave_play_form against a numpy restatement
of the payoff grid built from the oracle's scale / env_step / encode32 / encode64, and the packed byte arithmetic
of the kernel's table build (thrl_wave_kernel.h play_affine) restated in numpy uint32 and enumerated."""
import copy
import ctypes

import numpy as np
import pytest

from oracle import oracle as O  # checker only

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AGENT), dict(AGENT)], "environment": dict(ENV)}


def _mod(**kw):
    c = copy.deepcopy(CFG)
    for k, v in kw.items():
        if k in ("noise_prob", "max_steps"):
            c["environment"][k] = v
        elif k == "range1":
            c["agents"][1]["action_range"] = v
        else:
            for ag in c["agents"]:
                ag[k] = v
    return c


# name -> (config, float64 tables, expected answer, expected (c, m0, m1) or None, expected rows incl. the two spill rows)
CASES = {
    "cfg": (CFG, False, 1, (40, 1, 1), 43),
    "range_0.1_0.5": (_mod(range1=[0.1, 0.5]), False, 1, None, 63),        # slopes (1, 2); the last size one row register holds
    "actions16": (_mod(actions=16), False, 0, None, None),
    "states50": (_mod(states=50), False, 0, None, None),
    "states200": (_mod(states=200), False, 0, None, 83),                   # affine, but two row registers
    "noise": (_mod(noise_prob=0.05), False, 0, None, None),
    "float64": (CFG, True, 0, None, None),
    "two_episode_cycle": (_mod(max_steps=50), False, 0, None, None),       # min_memory 100 (default): trains every 2nd episode
}


@pytest.fixture(scope="module")
def lib():
    from th_rl_amd import build, _lib
    build.build()
    return _lib.load()


def grid_rows(config):
    """(r32, r64) [A, A]: the row after every action pair under the play (float32) and the train (float64) encode."""
    cfg, _ = O.cfg_from_config(config, 1, 0)
    A = cfg.n_actions[0]
    r32 = np.zeros((A, A), np.int64); r64 = np.zeros((A, A), np.int64)
    for a0 in range(A):
        for a1 in range(A):
            sc = [O.scale(a0, A, cfg.act_lo[0], cfg.act_hi[0]), O.scale(a1, A, cfg.act_lo[1], cfg.act_hi[1])]
            price = O.env_step(cfg, sc)[0]
            r32[a0, a1] = O.encode32(price, cfg.max_state[0], cfg.n_states[0])
            r64[a0, a1] = O.encode64(price, cfg.max_state[0], cfg.n_states[0])
    return r32, r64


def restated_form(config, float64=False):
    """What thrl_wave_play_form must answer, from the grid alone: (answer, (c, m0, m1) in local rows, window rows, grid is affine)."""
    r32, r64 = grid_rows(config)
    A = r32.shape[0]
    lo = int(min(r32.min(), r64.min())); W = int(max(r32.max(), r64.max())) - lo + 1
    c, m0, m1 = int(r32[0, 0]), int(r32[0, 0] - r32[1, 0]), int(r32[0, 0] - r32[0, 1])
    a0, a1 = np.meshgrid(np.arange(A), np.arange(A), indexing="ij")
    affine = bool(np.array_equal(r32, r64) and np.array_equal(r32, c - m0 * a0 - m1 * a1) and m0 >= 0 and m1 >= 0)
    env, ags = config["environment"], [dict(O.QTABLE_DEFAULTS, **a) for a in config["agents"]]
    T = env["max_steps"]
    one_episode_cycles = all(a["min_memory"] <= T <= a["capacity"] for a in ags)
    use = affine and not float64 and not env["noise_prob"] > 0 and W + 2 <= 64 and one_episode_cycles
    return int(use), (c - lo, m0, m1), W, affine


def query(lib, config, float64=False):
    from th_rl_amd import _lib
    cfg, _ = _lib.cfg_from_config(config, 64, 1 if float64 else 0)
    out = (ctypes.c_int * 3)(-1, -1, -1)
    got = lib.thrl_wave_play_form(ctypes.byref(cfg), ctypes.byref(out))
    assert lib.thrl_wave_play_form(ctypes.byref(cfg), None) == got          # out may be NULL
    return got, tuple(out)


@pytest.mark.parametrize("name", sorted(CASES))
def test_play_form_query(lib, name):
    config, f64, want, want_form, want_rows = CASES[name]
    got, form = query(lib, config, f64)
    use, rform, W, affine = restated_form(config, f64)
    assert got == want == use, (name, got, use)
    if want_rows is not None:
        assert W + 2 == want_rows
    if got:
        assert form == rform
        assert want_form is None or form == want_form
        assert 0 <= form[0] < W and form[0] - 20 * (form[1] + form[2]) >= 0
    else:
        assert form == (-1, -1, -1)                                          # untouched
    if name == "range_0.1_0.5":
        assert form[1:] == (1, 2)
    if name == "states200":
        assert affine and rform[1:] == (2, 2)
    if name in ("actions16", "states50"):
        assert not affine


def test_query_is_not_a_refusal(lib):
    """The play form changes nothing about which kernel runs, nor its workspace."""
    from th_rl_amd import _lib
    for name, (config, f64, _, _, _) in CASES.items():
        cfg, _ = _lib.cfg_from_config(config, 64, 1 if f64 else 0)
        assert lib.thrl_select_kernel(ctypes.byref(cfg), 0) == _lib.KERNEL_WAVE, name


def _u32(x):
    return np.asarray(x, np.uint64).astype(np.uint32)


@pytest.mark.parametrize("name", ["cfg", "range_0.1_0.5"])
def test_packed_arithmetic_enumerated(lib, name):
    """Tq = Kq - (G0q & M0q) - (G1q & M1q) in uint32, for every (greedy pair, choices, who explores) in every byte position
    with random valid steps in the other three bytes: every byte of the result is the LUT's row, and no byte of
    either subtraction borrows from its neighbour."""
    config = CASES[name][0]
    got, (c, m0, m1) = query(lib, config)
    assert got == 1
    r32, r64 = grid_rows(config)
    lo = int(r32.min())
    lut = (r32 - lo).astype(np.int64)
    A = lut.shape[0]
    assert np.array_equal(r32, r64) and lut.min() == 0 and lut.max() == c <= 61
    g0, g1, c0, c1, e0, e1 = [x.ravel() for x in np.meshgrid(*([np.arange(A)] * 4 + [np.arange(2)] * 2), indexing="ij")]
    n = g0.size
    rng = np.random.default_rng(7)

    def step_bytes(c0, c1, e0, e1):            # what a lane (= step) stores: m0b, m1b, kb
        return (np.where(e0 == 1, 0, 0xFF), np.where(e1 == 1, 0, 0xFF),
                c - np.where(e0 == 1, m0 * c0, 0) - np.where(e1 == 1, m1 * c1, 0))

    for pos in range(4):
        m0b = np.zeros((4, n), np.int64); m1b = np.zeros((4, n), np.int64); kb = np.zeros((4, n), np.int64)
        a0s = np.zeros((4, n), np.int64); a1s = np.zeros((4, n), np.int64)
        for j in range(4):
            if j == pos:
                s = (c0, c1, e0, e1)
            else:
                s = (rng.integers(0, A, n), rng.integers(0, A, n), rng.integers(0, 2, n), rng.integers(0, 2, n))
            m0b[j], m1b[j], kb[j] = step_bytes(*s)
            a0s[j] = np.where(s[2] == 1, s[0], g0); a1s[j] = np.where(s[3] == 1, s[1], g1)
        assert kb.min() >= 0 and kb.max() <= c
        pack = lambda b: _u32(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24))
        M0q, M1q, Kq = pack(m0b), pack(m1b), pack(kb)
        G0q, G1q = _u32(m0 * g0 * 0x01010101), _u32(m1 * g1 * 0x01010101)
        t1 = Kq - (G0q & M0q)                                  # uint32, wraps like the hardware
        Tq = t1 - (G1q & M1q)
        for j in range(4):
            b1 = kb[j] - ((m0 * g0) & m0b[j])                  # the same per byte, in wide integers
            b2 = b1 - ((m1 * g1) & m1b[j])
            assert b1.min() >= 0 and b2.min() >= 0                                    # nothing to borrow
            assert np.array_equal((t1 >> np.uint32(8 * j)) & np.uint32(0xFF), b1)     # and nothing borrowed
            assert np.array_equal((Tq >> np.uint32(8 * j)) & np.uint32(0xFF), b2)
            assert np.array_equal(b2, lut[a0s[j], a1s[j]])                            # the LUT's entry
