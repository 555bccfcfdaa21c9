"""The wave kernel's replay by per-lane pass number, restated in numpy against the serial pass loop it replaces.

A group of four transitions carries three cut bits (bit j-1: a new pass starts in front of transition j).  The
serial loop walked [lo, hi) ranges from cut to cut, starting at `first` (transitions in front of it have left the
deque) and ending at `nv` (the group's transitions inside the cycle).  The key schedule gives every transition
the key 4 * group + (cuts that count in front of it), where a cut counts only between two transitions that both
train, and no key to a transition that does not train; pass k of group g stores the lanes whose key is 4 g + k,
for k = 0 .. popcount(counted cuts).  Both must store the same transitions in the same order."""
import itertools

import numpy as np

KEY_SHIFT = 25          # thrl_wave_kernel.h kKeyShift
KEY_NONE = 0x7F         # thrl_wave_kernel.h kKeyNone
LDS_BYTES = 160 * 1024  # a CU's LDS: no store address reaches it


def serial_passes(cuts3, nv, first):
    """replay_group's former do ... while: list of passes, each the list of positions it stores."""
    if first >= 4:
        return []
    cuts = ((cuts3 & 7) << 1) | (1 << nv)
    lo = max(first, 0)
    if lo >= nv:
        return []
    out = []
    while True:
        rest = cuts >> (lo + 1)
        hi = lo + 1 + (int(rest & -rest).bit_length() - 1)
        out.append(list(range(lo, hi)))
        lo = hi
        if lo >= nv:
            return out


def key_schedule(cuts3, nv, first, group):
    """Phase (d2) for one group: (counted cut bits, key of each of the four positions), lane-parallel in numpy."""
    d = np.arange(4)
    trains = (d >= first) & (d < nv)
    pairs = trains & np.concatenate(([False], trains[:-1]))             # transitions d - 1 and d both train
    counted = cuts3 & int(sum(1 << (j - 1) for j in range(1, 4) if pairs[j]))
    pass_no = np.array([bin(counted & ((1 << int(j)) - 1)).count("1") for j in d])
    key = np.where(trains, 4 * group + pass_no, KEY_NONE)
    return counted, key


def keyed_passes(counted, key, group):
    """replay_group now: pass 0 always, then one pass per counted cut; a pass stores the matching keys."""
    return [[int(j) for j in np.nonzero(key == 4 * group + k)[0]] for k in range(1 + bin(counted).count("1"))]


CASES = list(itertools.product(range(8), range(1, 5), range(0, 5), range(8), range(2)))


def test_key_schedule_equals_serial_loop():
    assert len(CASES) == 8 * 4 * 5 * 8 * 2
    for cuts3, nv, first, group, half in CASES:
        serial = serial_passes(cuts3, nv, first)
        counted, key = key_schedule(cuts3, nv, first, group)
        if first >= 4:                       # the group is skipped before its first pass, as before
            assert serial == [] and np.all(key == KEY_NONE)
            continue
        got = keyed_passes(counted, key, group)
        kept = [j for j in range(4) if first <= j < nv]
        # same store sets in the same order (a group without a kept transition runs one empty pass: harmless)
        assert [p for p in got if p] == serial, (cuts3, nv, first, group, got, serial)
        if kept:
            assert got == serial
            inside = [j for j in range(1, 4) if (cuts3 >> (j - 1)) & 1 and j - 1 in kept and j in kept]
            assert len(got) == 1 + len(inside) == len(serial)
        else:
            assert got == [[]]
        stored = [j for p in got for j in p]
        assert sorted(stored) == kept                                        # every kept transition exactly once
        assert not set(stored) - set(kept)                                   # no dropped transition
        # exec layout: the transition sits in lane 32 * half + 8 * position + group; other groups' keys never match
        lanes = {32 * half + 8 * j + group for j in stored}
        assert len(lanes) == len(stored)
        others = [4 * g2 + k for g2 in range(8) if g2 != group for k in range(4)]
        assert not set(int(x) for x in key) & set(others)


def test_no_pass_matches_the_empty_key():
    assert all(4 * g + k != KEY_NONE for g in range(8) for k in range(4))
    assert KEY_NONE < (1 << (32 - KEY_SHIFT))


def test_packed_key_never_collides_with_an_address():
    addr = np.arange(0, LDS_BYTES, 4, dtype=np.uint64)
    assert int(addr.max()) < (1 << 18) <= (1 << KEY_SHIFT)
    for key in list(range(32)) + [KEY_NONE]:
        word = addr | np.uint64(key << KEY_SHIFT)
        assert int(word.max()) < (1 << 32)
        assert np.array_equal(word >> np.uint64(KEY_SHIFT), np.full(addr.shape, key, np.uint64))
        assert np.array_equal(word & np.uint64((1 << KEY_SHIFT) - 1), addr)
