"""The lane -> element maps of the wave kernel's per-game phases around the episode loop (thrl_wave_kernel.h), restated in
numpy and enumerated: the table stream-in (batches of eight loads per agent at clamped indices, LDS writes under k < n),
the stream-out (one element per lane and pass) and the counter apply (one no-return atomic add per non-zero histogram
cell; the spill rows' cells by the lanes below 2 A).

A window of n = rows * actions elements is contiguous and in the same order in HBM and in LDS, so a copy is a list of
(source, destination) pairs relative to the window's first element.  For every n in 1..2700 and element sizes 4 and 8
(every access is one element wide): every index lies in [0, n), every element is covered, and a pair copies an element to
its own index.  The counter apply must touch every cell exactly once, since an add, unlike a copy, may not be repeated.
Nothing outside the window is read or written: over-read is excluded here, by enumeration, not by a GPU run.

The LDS-direct stream-in and the 16-byte stream-out that profiles/stream_io.md measured and left out are not in the
kernel, so they are not restated here."""
import numpy as np
import pytest

LANES = np.arange(64)
N_MAX = 2700


def stream_in(n):
    """Batches of 8 loads per agent at the clamped element min(k, n - 1); the LDS write of load j only where k < n.
    Returns the elements READ (clamped loads included), the (source, destination) pairs written, and the load count."""
    read, src, dst, loads = [], [], [], 0
    for k0 in range(0, n, 512):
        for j in range(8):
            k = k0 + j * 64 + LANES
            kc = np.minimum(k, n - 1)
            read.append(kc)
            src.append(kc[k < n]); dst.append(k[k < n])
            loads += 1
    return np.concatenate(read), np.concatenate(src), np.concatenate(dst), loads


def stream_out(n):
    """for (k = lane; k < n; k += 64): element k of LDS to element k of HBM."""
    ks = [(k0 + LANES)[k0 + LANES < n] for k0 in range(0, n, 64)]
    return np.concatenate(ks), np.concatenate(ks), len(ks)


def counter_apply(W, A):
    """Histogram cell -> counter element (relative to the agent's table, window at row lo = 0 here): the window's cells by
    for (k = lane; k < W*A; k += 64), the two spill rows (histogram rows W and W + 1) by lane < 2 A."""
    n = W * A
    cells = [(k0 + LANES)[k0 + LANES < n] for k0 in range(0, n, 64)]
    spill = LANES[LANES < 2 * A]
    return np.concatenate(cells), n + spill, spill // A, spill % A


def _check(src, dst, n, label):
    assert src.min() >= 0 and src.max() < n, label
    assert dst.min() >= 0 and dst.max() < n, label
    assert np.array_equal(src, dst), label                        # an element only ever lands on its own index
    cover = np.zeros(n, bool)
    cover[dst] = True
    assert cover.all(), label


@pytest.mark.parametrize("size", [4, 8])
def test_stream_in_every_window_length(size):
    """The maps are counted in elements, so they are the same for both element sizes; the byte ranges follow."""
    for n in range(1, N_MAX + 1):
        label = "n %d size %d" % (n, size)
        read, src, dst, loads = stream_in(n)
        assert read.min() >= 0 and (read.max() + 1) * size <= n * size, label      # the clamped loads stay inside too
        _check(src, dst, n, label)
        assert dst.size == n, label                               # no element is written twice
        assert loads == 8 * -(-n // 512), label


@pytest.mark.parametrize("size", [4, 8])
def test_stream_out_every_window_length(size):
    for n in range(1, N_MAX + 1):
        label = "n %d size %d" % (n, size)
        src, dst, stores = stream_out(n)
        _check(src, dst, n, label)
        assert src.size == n and (dst.max() + 1) * size == n * size, label
        assert stores == -(-n // 64), label


def test_counter_apply_adds_every_cell_once():
    for W, A in ((41, 21), (11, 2), (21, 3), (32, 2), (16, 16), (126, 32), (1, 2), (3, 32)):
        cells, spill_cells, which, col = counter_apply(W, A)
        n = W * A
        assert np.array_equal(np.sort(cells), np.arange(n))                          # window: each cell once
        assert np.array_equal(spill_cells, np.arange(n, n + 2 * A))                  # histogram rows W and W + 1, each cell once
        assert np.array_equal(which, np.repeat([0, 1], A)) and np.array_equal(col, np.tile(np.arange(A), 2))
        assert 2 * A <= 64                                                            # the plan's 32 actions fit one pass


def test_headline_instruction_counts():
    """2 x 861 elements: 2 x 16 loads in two dependent batches, 2 x 14 stores, 2 x 14 (+ 2) conditional atomic adds."""
    assert stream_in(861)[3] == 16 and stream_out(861)[2] == 14
    assert -(-861 // 64) == 14
