"""The wave kernel's per-game log finish (`!LOG && !CYCLE` instantiations: an episode parks its four totals in the wave's
`partial` region, the game's epilogue divides, scales, rounds and adds them) against the per-episode finish.

The reference is the LOG instantiation of the same kernel, which still finishes every episode where it is played: the
same config, seed and call sequence run with and without per-game logs must return bit-equal `reward_log` and
`action_log` (fixed-point integer sums of the same rounded values: no tolerance).  Tables, visit counters and states of
both runs are compared bit for bit against the C oracle, and the logs against the oracle's to the tolerance the other wave
tests use.  The CYCLE case pins that the per-episode path is still what it was.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)


def _config(T=100, A=21, eps=0.5, noise=0.0, **agent_kw):
    ag = dict(AGENT, actions=A, epsilon=eps, eps_end=min(eps, 0.001) if eps != 0.02 else eps, min_memory=min(T, 100))
    ag.update(agent_kw)
    return {"agents": [dict(ag), dict(ag, alpha=0.3)], "environment": dict(ENV, max_steps=T, noise_prob=noise)}


def _check(config, G, calls, dtype="float32", kernel="wave", seed=7, sweep=None):
    """One run() call per entry of `calls`, on a batch without per-game logs (the per-game finish), on one with them (the
    per-episode finish) and on the oracle; compared after every call."""
    from th_rl_amd.batched import GameBatch
    batches = []
    for _ in range(2):
        gb = GameBatch(config, n_games=G, dtype=dtype, kernel=kernel, seed=seed)
        if sweep:
            gb.set_sweep(sweep)
        batches.append(gb.init_tables())
    plain, logged = batches
    q = plain.tables_numpy().copy(); s = plain.states_numpy().copy(); c = np.zeros(q.shape, np.int32)
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    osw = {k: v.cpu().numpy().copy() for k, v in plain.sweep.items()} if sweep else None
    mem, first = O.Memory(cfg), 0
    for k, E in enumerate(calls):
        label = "call %d (%d episodes)" % (k, E)
        out = plain.run(E)
        ref = logged.run(E, per_game_logs=True)
        assert out["kernel"] == "wave" and ref["kernel"] == "wave", label
        for name in ("reward_log", "action_log"):
            got, want = np.asarray(out[name]), np.asarray(ref[name])
            assert got.shape == want.shape and got.shape[0] == E, (label, name, got.shape)
            d = got != want
            print("%s %s: %d of %d values differ, max |diff| %.3g" % (label, name, int(d.sum()), d.size,
                                                                      float(np.abs(got - want).max())))
            assert not d.any(), "%s: %s differs from the per-episode finish in episodes %s" % (
                label, name, np.flatnonzero(d.reshape(E, -1).any(axis=1))[:8])
        oo = O.episodes(cfg, q, c, s, eps, mem, E, seed=seed, first_episode=first, **(dict(sweep=osw) if osw else {}))
        first += E
        for gb, who in ((plain, "plain"), (logged, "logged")):
            bad = np.flatnonzero((gb.tables_numpy() != q).any(axis=1))
            assert bad.size == 0, "%s, %s: tables of %d games differ (first %s)" % (label, who, bad.size, bad[:5])
            badc = np.flatnonzero((gb.counters_numpy() != c).any(axis=1))
            assert badc.size == 0, "%s, %s: counters of %d games differ (first %s)" % (label, who, badc.size, badc[:5])
            assert np.array_equal(gb.states_numpy(), s), (label, who)
        np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13, err_msg=label)
        np.testing.assert_allclose(out["action_log"], oo["action_log"], rtol=1e-12, atol=1e-13, err_msg=label)


@pytest.mark.parametrize("E", [1, 15, 16, 17, 31, 32])
def test_episode_counts(E):
    """One and both read-back passes, the last slot of the first and the first of the second, a full region."""
    _check(_config(), G=64, calls=(E,), seed=60 + E)


def test_second_call_plays_fewer_episodes():
    """Slots 3 and 4 hold what the first call left (its integer sums): the second call must not add them."""
    _check(_config(), G=64, calls=(5, 3), seed=71)


def test_second_call_after_a_full_region():
    _check(_config(), G=64, calls=(32, 2), seed=72)


@pytest.mark.parametrize("T", [4, 64, 65, 100])
def test_episode_lengths(T):
    """The divide by T; one ragged, one full and two segments."""
    _check(_config(T=T), G=64, calls=(3,), seed=80 + T)


@pytest.mark.parametrize("A", [2, 21])
def test_action_counts(A):
    _check(_config(A=A), G=64, calls=(3,), seed=90 + A)


def test_more_games_than_resident_waves():
    """A wave parks and finishes several games in the same slots."""
    _check(_config(), G=6400, calls=(2,), seed=3)


@pytest.mark.parametrize("G", [1, 3])
def test_fewer_games_than_waves(G):
    """Most waves play no game: their accumulators stay zero and they read no slot."""
    _check(_config(), G=G, calls=(3, 2), seed=100 + G)


def test_per_game_alpha():
    G = 96
    rs = np.random.RandomState(5)
    _check(_config(), G=G, calls=(3,), seed=41, sweep=dict(alpha=rs.choice([0.05, 0.1, 0.5], (2, G))))


def test_noise():
    _check(_config(noise=0.05), G=64, calls=(4, 3), seed=35)


def test_float64():
    _check(_config(), G=88, calls=(5, 3), dtype="float64", seed=33)


def test_greedy_variant():
    _check(_config(eps=0.02), G=96, calls=(5, 3), kernel="wave_greedy", seed=36)


def test_training_cycle_keeps_the_per_episode_finish():
    """min_memory 100 with 50-step episodes: a CYCLE instantiation, whose log sums are finished per part as before."""
    _check(_config(T=50, min_memory=100), G=64, calls=(6, 2), seed=77)
