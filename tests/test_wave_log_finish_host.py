"""The wave kernel's log finish, restated in numpy (no GPU): where an episode's four totals are parked, which lane and
which accumulator finishes them, and that this is what the per-episode finish (the LOG and CYCLE instantiations'
`log_into`) adds.

Per-episode path (thrl_wave_kernel.h, `log_into`): after `wave_sum4` every lane L holds the total of quantity k = L & 3
(reward0, reward1, action0, action1) of episode e; the rewards are divided by T, the value is scaled by log_scale[k >> 1]
and rounded to an integer, and lane 4 * (e & 15) + k adds it to `acc` (e < 16) or `acc_hi` (e >= 16).

Per-game path (`!LOG && !CYCLE`): lanes 4 * (e & 3) + k park the undivided totals in slot 4 * e + k of the wave's 128-word
`partial` region (those lanes, not lanes 0-3: the reduction's total is the same in every row of 16 lanes but can differ by
an ulp between the positions of a row, and the finishing lane of today's path sits at position 4 * (e & 3) + k); after the game's episode loop lane L reads slot L (pass 0) and slot 64 + L (pass 1), runs the same arithmetic and
adds to `acc` in pass 0 and to `acc_hi` in pass 1, for episodes below n_episodes only.  A slot the game did not write holds
whatever the region held before (an earlier launch's integer sums, or nothing that is a number): the add is masked, so
such a slot contributes nothing whatever its bits are.
"""
import numpy as np
import pytest

MAX_EPISODES = 32          # kWaveMaxEpisodes
SLOTS = 4 * MAX_EPISODES   # one wave's partial region, 8-byte words


def slot_of(e, k):
    return 4 * e + k


def pass_lane_of(slot):
    return slot // 64, slot % 64


def today_lane_acc(e, k):
    """Lane and accumulator (0 = acc, 1 = acc_hi) of the per-episode finish."""
    return 4 * (e & 15) + k, 0 if e < 16 else 1


def double2ll(x):
    """v_cvt of the product: round to nearest even; what is no number converts to 0 (and must be masked anyway)."""
    with np.errstate(invalid="ignore"):
        r = np.rint(x)
    ok = np.isfinite(r) & (np.abs(r) < 2.0 ** 62)
    return np.where(ok, r, 0.0).astype(np.int64)


def finish_one(v, lane, T, log_scale):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where((lane & 3) < 2, v / np.float64(T), v)
        return double2ll(v * np.where(lane & 2, log_scale[1], log_scale[0]))


def wave_sum4(totals_e):
    """What every lane holds after the reduction: quantity lane & 3.  The four rows of 16 lanes agree bit for bit, the four
    quads of a row need not (the rotate-adds associate differently by position): modelled as an ulp per position."""
    lane = np.arange(64)
    v = np.asarray(totals_e, np.float64)[lane & 3]
    for _ in range(4):
        v = np.where(((lane & 15) >> 2) > _, np.nextafter(v, np.inf), v)
    return v


def park_lane(e, k):
    """The lane whose value is parked: the position in its row of the lane that finishes episode e today."""
    return 4 * (e & 3) + k


def per_episode(totals, T, log_scale, acc=None):
    """totals [n_episodes][4] of one game -> acc [2][64], the per-episode path."""
    acc = np.zeros((2, 64), np.int64) if acc is None else acc
    lane = np.arange(64)
    for e in range(totals.shape[0]):
        vq = finish_one(wave_sum4(totals[e]), lane, T, log_scale)
        hit = (lane >> 2) == (e & 15)
        acc[0 if e < 16 else 1][hit] += vq[hit]
    return acc


def park(region, totals):
    for e in range(totals.shape[0]):
        v = wave_sum4(totals[e])
        for k in range(4):                                        # four lanes, one 8-byte store each
            region[slot_of(e, k)] = v[park_lane(e, k)]


def per_game(region, n_episodes, T, log_scale, acc=None):
    """The game epilogue on the wave's region (float64 view of the 128 words)."""
    acc = np.zeros((2, 64), np.int64) if acc is None else acc
    lane = np.arange(64)
    for p in range(2):
        vq = finish_one(region[64 * p + lane], lane, T, log_scale)
        played = 16 * p + (lane >> 2) < n_episodes
        acc[p][played] += vq[played]                              # the add is masked, not the product
    return acc


def test_slot_map_is_a_bijection_onto_the_lanes_of_two_passes():
    seen = {}
    for e in range(MAX_EPISODES):
        for k in range(4):
            s = slot_of(e, k)
            assert 0 <= s < SLOTS
            p, lane = pass_lane_of(s)
            assert (lane, p) == today_lane_acc(e, k), (e, k)
            assert lane & 3 == k and 16 * p + (lane >> 2) == e
            assert park_lane(e, k) == lane & 15                   # the same position in a row: the same bits of the total
            seen[s] = (e, k)
    assert sorted(seen) == list(range(SLOTS))                     # every slot is one (episode, quantity)


@pytest.mark.parametrize("n_episodes", range(1, MAX_EPISODES + 1))
def test_every_played_episode_is_finished_once_where_today_finishes_it(n_episodes):
    rs = np.random.RandomState(n_episodes)
    T, log_scale = 100, (2.0 ** 40, 2.0 ** 52)
    totals = np.concatenate([rs.uniform(0.0, 2500.0, (n_episodes, 2)), rs.uniform(20.0, 40.0, (n_episodes, 2))], axis=1)
    want = per_episode(totals, T, log_scale)
    for stale in (np.nan, np.inf, 1e300, 12345.678, 0.0):
        region = np.full(SLOTS, stale, np.float64)
        # what an earlier, longer launch left: its integer sums, read as doubles
        region[1::2] = np.arange(1, SLOTS // 2 + 1, dtype=np.int64).view(np.float64) if stale == 0.0 else region[1::2]
        park(region, totals)
        got = per_game(region, n_episodes, T, log_scale)
        assert np.array_equal(got, want), stale
    # which lanes moved: exactly those of the played episodes, each once (marker totals of 1 count the adds)
    ones = np.ones((n_episodes, 4))
    region = np.full(SLOTS, 7.0)
    park(region, ones)
    cnt = per_game(region, n_episodes, 1, (1.0, 1.0))
    for e in range(MAX_EPISODES):
        for k in range(4):
            lane, a = today_lane_acc(e, k)
            assert cnt[a][lane] == (1 if e < n_episodes else 0), (e, k)


def test_both_halves_take_the_divide_and_their_own_scale():
    T, log_scale = 7, (2.0 ** 20, 2.0 ** 33)
    totals = np.array([[10.0, 11.0, 12.0, 13.0]])
    region = np.zeros(SLOTS)
    park(region, totals)
    acc = per_game(region, 1, T, log_scale)
    want = [int(np.rint(np.float64(10.0) / 7.0 * 2.0 ** 20)), int(np.rint(np.float64(11.0) / 7.0 * 2.0 ** 20)),
            int(12.0 * 2.0 ** 33), int(13.0 * 2.0 ** 33)]
    assert acc[0][:4].tolist() == want and not acc[0][4:].any() and not acc[1].any()
    # an episode of the upper half: the same lanes, the other accumulator
    region = np.zeros(SLOTS)
    region[slot_of(16, 0):slot_of(16, 0) + 4] = totals[0]
    acc = per_game(region, 17, T, log_scale)
    assert acc[1][:4].tolist() == want and not acc[1][4:].any()


def test_a_wave_parks_several_games_and_launches_in_the_same_slots():
    """Three games of five episodes, the region then holds the launch's integer sums (the kernel's last two stores), then
    two games of three episodes: the second launch sees neither the first's parked values nor its sums."""
    rs = np.random.RandomState(3)
    T, log_scale = 100, (2.0 ** 38, 2.0 ** 50)
    region = np.full(SLOTS, np.nan)
    for n_episodes, games in ((5, 3), (3, 2)):
        got, want = np.zeros((2, 64), np.int64), np.zeros((2, 64), np.int64)
        for _ in range(games):
            totals = np.concatenate([rs.uniform(0.0, 2500.0, (n_episodes, 2)), rs.uniform(20.0, 40.0, (n_episodes, 2))], axis=1)
            park(region, totals)
            per_game(region, n_episodes, T, log_scale, got)
            per_episode(totals, T, log_scale, want)
        assert np.array_equal(got, want), n_episodes
        assert not got[:, 4 * n_episodes:].any() if n_episodes < 16 else True
        region[:] = got.reshape(-1).view(np.float64)              # a.partial[wave][0..127] = acc, acc_hi
