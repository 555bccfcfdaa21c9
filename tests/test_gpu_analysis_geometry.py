"""More games than the grid, for every analysis entry point whose grid is planned from the device's CU count and LDS
(thrl_attractors and thrl_stationary have such a case in their own modules): the blocks loop over games, so a slip in
a grid or in a block's LDS layout shows as a game whose result depends on where it stands in the batch.

K = 5 distinct base games are tiled to G = 32 * multi_processor_count + 3 games (32 is the largest blocks-per-CU cap
of these entry points): game g is a copy of base game g % K, and every per-game output of game g must equal, byte for
byte, that of base game g % K from a separate call with G = K.  G = 1 runs too.  Two QTable agents with 4 and 3
actions (T = 12 tuples), 20 states."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 5
AG = dict(name="QTable", gamma=0.95, actions=4, states=20, alpha=0.1, eps_end=0.001, epsilon=0.5, eps_step=0.9995,
          action_range=[0.2, 0.4])
CONFIG = {"agents": [dict(AG), dict(AG, actions=3, alpha=0.3, gamma=0.9)],
          "environment": dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=25)}


def _track(gb):
    tr = gb.track_convergence(window=4)             # the baseline launch extracts every game's policy
    tr.check(count=False)
    return tr.to_numpy()


def _crossplay(gb):
    seats = np.tile(np.arange(gb.G), (gb.N, 1))     # match m seats every agent from game m; no policy given: the extraction pass
    out = gb.crossplay(seats)
    out.pop("seats")                                # the input, echoed
    return out


# entry point -> the call through the batch methods
CALLS = {
    "thrl_policy_track": _track,
    "thrl_crossplay": _crossplay,
    "thrl_equilibrium": lambda gb: gb.equilibrium(policies=True),
    "thrl_tuple_equilibrium": lambda gb: gb.greedy_equilibrium(policies=True),
    "thrl_tuple_attractors": lambda gb: gb.greedy_attractors(policies=True),
    "thrl_tuple_stationary": lambda gb: gb.greedy_stationary(noise_prob=0.05, resolution=64, pi=True),
    "thrl_sampled_chain": lambda gb: gb.sampled_play(epsilon=0.1, pi=True),
    "thrl_sampled_noise_chain": lambda gb: gb.sampled_play(epsilon=0.1, noise_prob=0.05, resolution=64),
}


@pytest.fixture(scope="module")
def base():
    """(tables [K, stride], states [K]) of K games after a little training: distinct tables, states on the price grid."""
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(CONFIG, n_games=K, seed=7).init_tables()
    gb.run(20, logs=False)
    q, s = gb.tables_numpy().copy(), gb.states_numpy().copy()
    assert len({q[k].tobytes() for k in range(K)}) == K
    return q, s


def _batch(base, G):
    from th_rl_amd.batched import GameBatch
    q, s = base
    g = np.arange(G) % K
    return GameBatch(CONFIG, n_games=G, counters=False).set_tables(q[g], s[g])


def _per_game(big, small, G, n):
    """{field: (array of the G games, array of the n games)} with the game axis first, for every array output whose
    shape differs between the two calls; the others must not differ at all."""
    out = {}
    assert sorted(big) == sorted(small)
    for f in big:
        a, b = big[f], small[f]
        if not isinstance(a, np.ndarray):
            continue
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.ndim == b.ndim, f
        axes = [i for i in range(a.ndim) if a.shape[i] != b.shape[i]]
        if not axes:                                # of the config, not of a game
            assert a.tobytes() == b.tobytes(), f
            continue
        assert len(axes) == 1 and a.shape[axes[0]] == G and b.shape[axes[0]] == n, (f, a.shape, b.shape)
        out[f] = (np.ascontiguousarray(np.moveaxis(a, axes[0], 0)), np.ascontiguousarray(np.moveaxis(b, axes[0], 0)))
    return out


def _bytes(x):
    return x.reshape(x.shape[0], -1).view(np.uint8)


@pytest.mark.parametrize("entry", list(CALLS))
def test_more_games_than_the_grid(entry, base):
    import torch
    call = CALLS[entry]
    G = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    ref = call(_batch(base, K))
    fields = _per_game(call(_batch(base, G)), ref, G, K)
    assert len(fields) >= 3, sorted(fields)
    spots = np.r_[0:K, G // 2 - K // 2:G // 2 - K // 2 + K, G - K:G]
    for f, (a, b) in sorted(fields.items()):
        a, b = _bytes(a), _bytes(b)
        for g in spots:
            assert np.array_equal(a[g], b[g % K]), (entry, f, int(g))
        bad = np.flatnonzero((a != b[np.arange(G) % K]).any(axis=1))
        assert bad.size == 0, (entry, f, bad[:8])
    # one game: the grid is one block
    one = _per_game(call(_batch(base, 1)), ref, 1, K)
    assert sorted(one) == sorted(fields)
    for f, (a, b) in one.items():
        assert np.array_equal(_bytes(a)[0], _bytes(b)[0]), (entry, f)
