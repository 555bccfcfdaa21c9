"""The wave kernel's cell word and 32-bit visit histogram, restated in numpy (no GPU).

A transition of the wave kernel rewrites one table cell per agent: (srow, a0) of agent 0 and (srow, a1) of agent 1, srow a
local row of the wave's LDS window (W window rows + 2 spill rows, A actions).  The kernel packs the two cells into one word

    cw = off0 | off1 << 16,     off0 = 4 * (srow * A + a0),     off1 = 4 * ((W + 2) * A + srow * A + a1)

(byte offsets of the cells' u32 histogram counters from the start of the wave's table region), logs that word per
transition, and after the launch builds a u32-per-cell histogram over the freed table region from the log and adds it to
the game's visit counters.  0xFFFFFFFF marks a lane that is not counted: past the end of the cycle, or dropped from the
replay deque before it trained (lanes before replay_from).

Checked here over every window / action size plan_wave accepts (the extremes come from limits_table.py): both fields fit
16 bits, the marker is not a valid word, the histogram fits the region in both table dtypes, and build + apply equal a
direct count of the visits, spill rows and dropped lanes included."""
import numpy as np
import pytest

import limits_table as LT

MARK = 0xFFFFFFFF
W_MAX = LT.measure(LT.BY_ID["wave-rows-126"])["win_rows"]
A_MAX = LT.measure(LT.BY_ID["wave-A32"])["max_actions"]
T_MAX = LT.measure(LT.BY_ID["wave-256-transitions"])["transitions"]
E_MAX = 32                                                         # episodes per launch (kWaveMaxEpisodes)


def cell_word(srow, a0, a1, W, A):
    srow, a0, a1 = (np.asarray(x, np.uint32) for x in (srow, a0, a1))
    off0 = np.uint32(4) * (srow * np.uint32(A) + a0)
    off1 = np.uint32(4) * (np.uint32((W + 2) * A) + srow * np.uint32(A) + a1)
    return off0 | (off1 << np.uint32(16)), off0, off1


def logged_words(srow, a0, a1, valid, step, replay_from, W, A):
    """What the kernel stores: the marker for lanes that are not valid or lie before replay_from."""
    cw = cell_word(np.where(valid, srow, 0), np.where(valid, a0, 0), np.where(valid, a1, 0), W, A)[0]
    return np.where(valid & (step >= replay_from), cw, np.uint32(MARK)).astype(np.uint32)


def build_hist(words, W, A):
    """Read-back: marker test, then one add of 1 at each half's offset; u32 per cell, 2 * (W + 2) * A cells."""
    hist = np.zeros(2 * (W + 2) * A, np.uint32)
    w = words[words != np.uint32(MARK)]
    np.add.at(hist, (w & np.uint32(0xFFFF)) >> np.uint32(2), np.uint32(1))
    np.add.at(hist, (w >> np.uint32(16)) >> np.uint32(2), np.uint32(1))
    return hist


def apply_hist(hist, counters, lo, W, A, spill0, spill1):
    """counters [2, rows, A] of one game: the window rows are contiguous, spill rows W / W + 1 go to their global rows.
    Cells with a zero count are not written."""
    cells = (W + 2) * A
    written = np.zeros(counters.shape, bool)
    for ag in range(2):
        h = hist[ag * cells:(ag + 1) * cells].reshape(W + 2, A)
        flat = counters[ag].reshape(-1)
        wflat = written[ag].reshape(-1)
        for k in range(W * A):
            n = h.reshape(-1)[k]
            if n:
                flat[lo * A + k] += np.int32(n); wflat[lo * A + k] = True
        for j, grow in ((W, spill0), (W + 1, spill1)):
            if grow >= 0:
                for col in range(A):
                    if h[j, col]:
                        counters[ag, grow, col] += np.int32(h[j, col]); written[ag, grow, col] = True
    return written


def test_limits_are_the_plans():
    assert (W_MAX, A_MAX, T_MAX) == (126, 32, 256)
    c = LT.BY_ID["wave-rows-126-A32-f64"]
    m = LT.measure(c)
    assert (m["win_rows"], m["max_actions"]) == (W_MAX, A_MAX)     # both extremes are accepted together
    assert LT.BY_ID["wave-rows-127"]["side"] == "refuse" and LT.BY_ID["wave-A33"]["side"] == "refuse"


def test_fields_fit_16_bits_and_marker_is_unreachable():
    top = 0
    for W in range(1, W_MAX + 1):
        A = np.arange(2, A_MAX + 1)
        # the largest offsets: last spill row, last action
        cw, off0, off1 = cell_word(np.full(A.shape, W + 1), A - 1, A - 1, W, A)
        assert (off0 < off1).all() and (off1 <= 0xFFFF).all()
        assert (off1 == 4 * (2 * (W + 2) * A - 1)).all()           # the last u32 of the region
        assert ((cw & np.uint32(0xFFFF)) == off0).all() and ((cw >> np.uint32(16)) == off1).all()
        top = max(top, int(off1.max()))
    assert top == 4 * 8191 == 32764                                # (126 + 2) rows x 32 actions x 2 agents
    # every valid word has both halves a multiple of 4 and bit 15 / bit 31 clear; the marker has neither
    assert MARK & 3 == 3 and (MARK >> 16) & 3 == 3 and MARK >> 31 == 1
    assert top < 0x8000
    # exhaustive at the extreme plan: no (srow, a0, a1) gives the marker, and the word is invertible
    W, A = W_MAX, A_MAX
    s, a0, a1 = np.meshgrid(np.arange(W + 2), np.arange(A), np.arange(A), indexing="ij")
    cw = cell_word(s, a0, a1, W, A)[0]
    assert not (cw == np.uint32(MARK)).any()
    assert np.unique(cw).size == cw.size


@pytest.mark.parametrize("esz", [4, 8])
def test_histogram_fits_the_region(esz):
    for W in (1, 41, 62, 63, W_MAX):
        for A in (2, 16, 21, A_MAX):
            region = 2 * (W + 2) * A * esz                         # the two table windows (plan_wave: game_lds_bytes)
            hist_bytes = 4 * 2 * (W + 2) * A
            assert hist_bytes <= region
            assert hist_bytes == (region if esz == 4 else region // 2)
            assert region % 8 == 0                                 # 8-byte stores zero it
            off1_top = cell_word(W + 1, A - 1, A - 1, W, A)[2]
            assert int(off1_top) + 4 == hist_bytes
    assert E_MAX * T_MAX * 2 < 2 ** 32                             # a u32 cell cannot wrap in one launch


def _random_case(rng, W, A, T, E, replay_from, lo, rows):
    """E cycles of T transitions (NSEG * 64 lanes each, the tail lanes not valid)."""
    nseg = (T + 63) // 64
    step = np.tile(np.arange(nseg * 64), (E, 1))
    valid = step < T
    srow = rng.integers(0, W + 2, size=step.shape)
    # make sure both spill rows and the window's first and last row occur
    srow[0, :4] = (W, W + 1, 0, W - 1)
    a0 = rng.integers(0, A, size=step.shape)
    a1 = rng.integers(0, A, size=step.shape)
    # and a cell visited many times
    srow[:, 5:9] = W // 2; a0[:, 5:9] = A - 1; a1[:, 5:9] = 0
    return step, valid, srow, a0, a1


@pytest.mark.parametrize("W,A,T,E,replay_from", [
    (41, 21, 100, 25, 0),          # the headline shape
    (41, 21, 100, 5, 0),
    (41, 21, 100, 2, 36),          # capacity 64 of a 100-step cycle
    (W_MAX, A_MAX, 256, 32, 0),    # the extreme plan, the longest launch
    (W_MAX, A_MAX, 256, 3, 255),   # one transition kept
    (1, 2, 7, 4, 3),
    (62, 16, 30, 1, 0),
    (5, 3, 128, 2, 128),           # never trains: nothing is counted
])
def test_build_and_apply_equal_a_direct_count(W, A, T, E, replay_from):
    rng = np.random.default_rng(W * 1000 + A * 10 + T)
    lo, rows = 3, W + 3 + 4
    spill0, spill1 = 1, rows - 1                                   # global rows of the two spill rows (outside the window)
    step, valid, srow, a0, a1 = _random_case(rng, W, A, T, E, replay_from, lo, rows)
    words = logged_words(srow, a0, a1, valid, step, replay_from, W, A)
    assert (words[~valid] == np.uint32(MARK)).all()
    assert (words[step < replay_from] == np.uint32(MARK)).all()
    hist = build_hist(words, W, A)
    counters = rng.integers(0, 1000, size=(2, rows, A)).astype(np.int32)
    before = counters.copy()
    written = apply_hist(hist, counters, lo, W, A, spill0, spill1)
    # direct count of (srow, a0) / (srow, a1) over the counted transitions
    want = before.copy()
    touched = np.zeros(want.shape, bool)
    grow = np.where(srow < W, srow + lo, np.where(srow == W, spill0, spill1))
    keep = valid & (step >= replay_from)
    for ag, act in ((0, a0), (1, a1)):
        np.add.at(want[ag], (grow[keep], act[keep]), 1)
        touched[ag][grow[keep], act[keep]] = True
    assert np.array_equal(counters, want)
    assert np.array_equal(written, touched)                        # untouched counter cells are not written
    assert int(hist.sum()) == 2 * int(keep.sum()) == 2 * E * max(T - replay_from, 0)


def test_spill_rows_unused_are_not_applied():
    """A game that starts inside the window has no spill rows: their histogram rows stay empty and nothing is written."""
    W, A = 41, 21
    step = np.arange(64)[None]
    srow = np.full((1, 64), 7); a0 = np.full((1, 64), 3); a1 = np.full((1, 64), 4)
    words = logged_words(srow, a0, a1, step < 64, step, 0, W, A)
    hist = build_hist(words, W, A)
    cells = (W + 2) * A
    assert hist[W * A:cells].sum() == 0 and hist[cells + W * A:].sum() == 0
    counters = np.zeros((2, 101, A), np.int32)
    apply_hist(hist, counters, 20, W, A, -1, -1)
    assert counters[0, 27, 3] == 64 and counters[1, 27, 4] == 64 and counters.sum() == 128
