"""The wave kernel's Philox with the three-input xor (thrl_device.h: draw_lanes, philox4x32_10_lanes) against the C
oracle, bit for bit on tables, visit counters and states.

Nothing is injected: every explore decision and every random action comes from the kernel's own draws, so one wrong bit
in any round moves a trajectory.  The cases put bits above 2^32 into the seed and the first game's number, start at a
large episode, run both segments of a 100-step episode and ragged ones, and go through the variants that share the
call: training cycles of several episodes (the episode word differs per lane), noise, a per-game sweep, per-game logs,
and more games than resident waves.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AGENT = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
             epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
DTYPES = ["float32", "float64"]


def _config(T=100, A=21, eps=0.5, noise=0.0, **agent_kw):
    ag = dict(AGENT, actions=A, epsilon=eps, eps_end=min(eps, 0.001), min_memory=min(T, 100))
    ag.update(agent_kw)
    return {"agents": [dict(ag), dict(ag, alpha=0.3)], "environment": dict(ENV, max_steps=T, noise_prob=noise)}


def _same(gb, q, c, s, label=""):
    bad = np.flatnonzero((gb.tables_numpy() != q).any(axis=1))
    assert bad.size == 0, "%s: tables of %d games differ (first %s)" % (label, bad.size, bad[:5])
    badc = np.flatnonzero((gb.counters_numpy() != c).any(axis=1))
    assert badc.size == 0, "%s: counters of %d games differ (first %s)" % (label, badc.size, badc[:5])
    assert np.array_equal(gb.states_numpy(), s), label


def _against_oracle(config, G, calls, dtype, seed, sweep=None, game_offset=0, first_episode=0, per_game_logs=False):
    """One run() call per entry of `calls` on the wave kernel and on the oracle (own draws), compared after every call."""
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel="wave", seed=seed, game_offset=game_offset)
    if sweep:
        gb.set_sweep(sweep)
    gb.init_tables()
    gb.episode = first_episode
    q = gb.tables_numpy().copy(); s = gb.states_numpy().copy(); c = np.zeros(q.shape, np.int32)
    cfg, eps = O.cfg_from_config(config, G, 1 if dtype == "float64" else 0)
    osw = {k: v.cpu().numpy().copy() for k, v in gb.sweep.items()} if sweep else None
    mem, first = O.Memory(cfg), first_episode
    for k, E in enumerate(calls):
        label = "call %d (%d episodes)" % (k, E)
        out = gb.run(E, per_game_logs=per_game_logs)
        assert out["kernel"] == "wave", label
        oo = O.episodes(cfg, q, c, s, eps, mem, E, seed=seed, game_offset=game_offset, first_episode=first,
                        **(dict(sweep=osw) if osw else {}))
        first += E
        _same(gb, q, c, s, label)
        np.testing.assert_allclose(out["reward_log"], oo["reward_log"], rtol=1e-12, atol=1e-13, err_msg=label)
        np.testing.assert_allclose(out["action_log"], oo["action_log"], rtol=1e-12, atol=1e-13, err_msg=label)
        if per_game_logs:
            np.testing.assert_allclose(out["game_reward_log"], oo["game_reward_log"], rtol=1e-12, atol=1e-13, err_msg=label)
            np.testing.assert_allclose(out["game_action_log"], oo["game_action_log"], rtol=1e-12, atol=1e-13, err_msg=label)
    return cfg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed,game_offset,first_episode", [
    ((0xDEADBEEF << 32) | 0x12345678, 0, 0),
    (7, (5 << 32) + 123, 0),
    (0xFFFFFFFFFFFFFFFF, (0xABCDEF << 32) | 0xFFFFFFC0, 0),          # the game counter's low word wraps inside the batch
    (3, 0, 0xFFFFFF00),
    ((1 << 63) | 1, (1 << 40) + 1, 123456789),
])
def test_seed_game_and_episode_words(dtype, seed, game_offset, first_episode):
    """Both segments of a 100-step episode, 64 games x 3 episodes: seed and first game with bits above 2^32, a large
    first episode."""
    _against_oracle(_config(), G=64, calls=(3,), dtype=dtype, seed=seed, game_offset=game_offset, first_episode=first_episode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [4, 5, 31, 33, 63, 64, 65, 100, 128, 130])
def test_episode_lengths(dtype, T):
    """Ragged last segments (the lanes behind the episode's end draw too and must not count), one, two and three
    segments."""
    _against_oracle(_config(T=T), G=64, calls=(3,), dtype=dtype, seed=21 + T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A", [2, 3, 21, 32])
def test_action_counts(dtype, A):
    """The random action is mulhi(draw, A)."""
    _against_oracle(_config(A=A), G=64, calls=(3,), dtype=dtype, seed=50 + A)


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_cycle_of_several_episodes(dtype):
    """min_memory 100 with 50-step episodes: a training cycle plays two episodes, so the episode word of the counter
    differs between the lanes of a segment."""
    _against_oracle(_config(T=50, min_memory=100), G=64, calls=(6, 2), dtype=dtype, seed=77)


@pytest.mark.parametrize("dtype", DTYPES)
def test_noise(dtype):
    _against_oracle(_config(noise=0.05), G=64, calls=(4,), dtype=dtype, seed=35)


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_game_alpha(dtype):
    G = 96
    rs = np.random.RandomState(5)
    _against_oracle(_config(), G=G, calls=(3,), dtype=dtype, seed=41, sweep=dict(alpha=rs.choice([0.05, 0.1, 0.5], (2, G))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_game_logs(dtype):
    _against_oracle(_config(), G=96, calls=(4, 3), dtype=dtype, seed=37, per_game_logs=True)


def test_more_games_than_resident_waves():
    """A wave's second game draws with its own game word."""
    _against_oracle(_config(), G=6400, calls=(2,), dtype="float32", seed=3)
