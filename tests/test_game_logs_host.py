"""Host-side logic of the per-game log artefacts (training.game_logs): the shard cut of an id list, utils.game_log on
single-directory and shard layouts, and the per-launch byte budget of the device buffers.  No GPU."""
import os

import numpy as np
import pandas
import pytest

from th_rl_amd.launch import shard_training
from th_rl_amd.trainer import GAME_LOG_BUDGET, game_log_chunk, game_log_ids

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
CONFIG = {"agents": [dict(AG), dict(AG)],
          "environment": dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)}


def _cfg(**training):
    return dict(CONFIG, training=dict(dict(epochs=10, seed=1), **training))


def test_shard_training_cuts_a_game_logs_list():
    ids = [0, 5, 9, 10, 24, 25, 39]
    got = []
    for r in range(4):                                  # 40 games on 4 ranks: blocks of 10
        tr, off, n = shard_training(_cfg(n_games=40, game_logs=ids), r, 4)
        assert all(tr["game_offset"] <= i < tr["game_offset"] + n for i in tr["game_logs"])
        got += tr["game_logs"]
    assert got == ids
    tr, _, _ = shard_training(_cfg(n_games=40, game_offset=100, game_logs=[100, 112, 139]), 1, 4)
    assert tr["game_logs"] == [112]                     # global ids: the run's own game_offset counts


def test_shard_training_keeps_true_and_absent_unchanged():
    tr, _, _ = shard_training(_cfg(n_games=40, game_logs=True), 2, 4)
    assert tr["game_logs"] is True
    tr, _, _ = shard_training(_cfg(n_games=40), 2, 4)
    assert "game_logs" not in tr


def _write(d, ids, rew, act):
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "game_ids.npy"), np.asarray(ids, np.int64))
    np.save(os.path.join(d, "game_rewards.npy"), rew)
    np.save(os.path.join(d, "game_actions.npy"), act)


def test_game_log_single_directory_and_shards(tmp_path):
    from th_rl_amd.utils import game_log
    rs = np.random.RandomState(0)
    E, N = 7, 2
    rew, act = rs.rand(E, N, 3), rs.rand(E, N, 3)
    _write(str(tmp_path / "one"), [4, 8, 15], rew, act)
    df = game_log(str(tmp_path / "one"), 8)
    assert list(df.columns) == [("rewards", 0), ("rewards", 1), ("actions", 0), ("actions", 1)]
    np.testing.assert_array_equal(df["rewards"].to_numpy(), rew[:, :, 1])
    np.testing.assert_array_equal(df["actions"].to_numpy(), act[:, :, 1])
    # the same columns as the log.csv train_one writes, once read back
    df.to_csv(str(tmp_path / "log.csv"), index=None)
    back = pandas.read_csv(str(tmp_path / "log.csv"), header=[0, 1], float_precision="round_trip")
    np.testing.assert_array_equal(back.to_numpy(), df.to_numpy())
    with pytest.raises(KeyError):
        game_log(str(tmp_path / "one"), 5)

    sh = tmp_path / "sharded"
    r0, a0, r1, a1 = rs.rand(E, N, 2), rs.rand(E, N, 2), rs.rand(E, N, 1), rs.rand(E, N, 1)
    _write(str(sh / "shard0"), [0, 3], r0, a0)
    _write(str(sh / "shard1"), [21], r1, a1)
    np.testing.assert_array_equal(game_log(str(sh), 3)["rewards"].to_numpy(), r0[:, :, 1])
    np.testing.assert_array_equal(game_log(str(sh), 21)["actions"].to_numpy(), a1[:, :, 0])


def test_per_chunk_byte_budget():
    for N, G in ((2, 1 << 20), (3, 65536), (2, 4096), (8, 1 << 22), (1, 1)):
        k = game_log_chunk(N, G)
        assert k >= 1
        assert k * N * G * 8 <= GAME_LOG_BUDGET or k == 1
    assert game_log_chunk(2, 1 << 20) == 16             # the headline shape: 16 episodes = 256 MiB per buffer
    for cycle in (2, 3, 10):                            # whole training cycles of the wave kernel
        k = game_log_chunk(2, 1 << 20, cycle)
        assert k % cycle == 0 and (k * 2 * (1 << 20) * 8 <= GAME_LOG_BUDGET or k == cycle)
    assert game_log_chunk(8, 1 << 24, 3) == 3           # never less than one cycle


def test_game_log_ids():
    g, l = game_log_ids(True, 4, 10)
    assert g.tolist() == [10, 11, 12, 13] and l.tolist() == [0, 1, 2, 3] and g.dtype == np.int64
    g, l = game_log_ids([12, 10], 4, 10)
    assert g.tolist() == [12, 10] and l.tolist() == [2, 0]
    with pytest.raises(ValueError):
        game_log_ids([9], 4, 10)
