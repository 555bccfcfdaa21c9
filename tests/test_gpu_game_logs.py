"""Per-game episode logs (thrl_buffers.game_reward_log / game_action_log, [E][N][G]) from the LDS-resident wave and
tuple kernels, and the trainer's per-game artefacts (training.game_logs).  Against the CPU oracle, the generic kernel and
the same runs without per-game logs."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}
GREEDY = {"agents": [dict(AG, epsilon=0.01, eps_end=0.01), dict(AG, epsilon=0.02, eps_end=0.02)], "environment": dict(ENV)}
NOISY = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV, noise_prob=0.05)}
CYCLE = {"agents": [dict(AG, min_memory=100), dict(AG, min_memory=100, alpha=0.3)], "environment": dict(ENV, max_steps=50)}
THREE = {"agents": [dict(AG, actions=11, states=50, action_range=[0.1, 0.3], min_memory=25),
                    dict(AG, actions=21, states=100, action_range=[0.15, 0.35], min_memory=25),
                    dict(AG, actions=5, states=20, action_range=[0.0, 0.3], min_memory=25, max_state=10)],
         "environment": dict(ENV, nplayers=3, max_steps=25)}
GRIDS = {"agents": [dict(AG, actions=7, states=30, action_range=[0.1, 0.5], min_memory=10),
                    dict(AG, actions=21, states=100, action_range=[0.2, 0.4], min_memory=10, alpha=0.3, gamma=0.9)],
         "environment": dict(ENV, max_steps=40)}
THREE_NOISE = {"agents": THREE["agents"], "environment": dict(THREE["environment"], noise_prob=0.05)}

E = 40          # > 32: two launch chunks, the second with first_episode = 32


def _sweep(N, G, noise):
    rs = np.random.RandomState(7)
    sw = dict(gamma=rs.choice([0.35, 0.9, 0.95], (N, G)), alpha=rs.choice([0.05, 0.1, 0.5], (N, G)),
              eps=rs.uniform(0.0, 0.9, (N, G)), eps_end=rs.choice([0.0, 0.01], (N, G)),
              eps_step=rs.choice([0.9, 0.999], (N, G)))
    if noise:
        sw["noise_prob"] = rs.choice([0.0, 0.05, 0.5], G)
    return sw


# label, config, G, kernel, kernel reported, sweep (None / "plain" / "noise")
CASES = [
    ("wave_plain", TWO, 4096, "wave_plain", "wave", None),
    ("wave_greedy", GREEDY, 4096, "wave_greedy", "wave", None),
    ("wave_noise", NOISY, 4096, "wave", "wave", None),
    ("wave_sweep", NOISY, 4096, "wave", "wave", "noise"),
    ("wave_cycle", CYCLE, 4096, "wave", "wave", None),
    ("tuple_three_players", THREE, 4096, "tuple", "tuple", None),
    ("tuple_two_grids", GRIDS, 4096, "tuple", "tuple", None),
    ("tuple_noise", THREE_NOISE, 4096, "tuple", "tuple", None),
    ("tuple_sweep", THREE_NOISE, 4096, "tuple", "tuple", "noise"),
]


def _batch(config, G, dtype, kernel, sweep, seed=23):
    from th_rl_amd.batched import GameBatch
    gb = GameBatch(config, n_games=G, dtype=dtype, kernel=kernel, seed=seed)
    if sweep is not None:
        gb.set_sweep(sweep)
    return gb


def _state(gb):
    eps = gb.sweep["eps"].cpu().numpy() if "eps" in gb.sweep else np.array(gb.eps[:gb.N], np.float64)
    return gb.tables_numpy(), gb.counters_numpy(), gb.states_numpy(), eps


def _assert_same_state(a, b, label):
    for x, y, what in zip(a, b, ("tables", "counters", "state", "epsilon")):
        if what == "epsilon":
            x, y = np.asarray(x)[:len(a[3])], np.asarray(y, np.float64)[:len(a[3])]
        assert np.array_equal(x, y), "%s: %s differ" % (label, what)


def test_wave_and_tuple_kernels_take_per_game_logs():
    """Before: per-game logs sent every all-QTable run to the generic kernel (an explicit kernel="wave" / "tuple"
    raised THRL_ERR_UNSUPPORTED).  Now the LDS-resident kernels write them, under AUTO and when asked for."""
    for config, kernel in ((TWO, "wave"), (THREE, "tuple")):
        for k in (kernel, "auto"):
            gb = _batch(config, 256, "float32", k, None).init_tables()
            out = gb.run(3, per_game_logs=True)
            assert out["kernel"] == kernel, (k, out["kernel"])
            assert out["game_reward_log"].shape == (3, gb.N, 256)
            assert np.all(out["game_reward_log"] > 0) and np.all(out["game_action_log"] > 0)
            if kernel == "wave":
                assert gb.replay_mem is None                  # no replay memory just because logs were asked for


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("label,config,G,kernel,used,sweep", CASES, ids=[c[0] for c in CASES])
def test_per_game_logs_vs_oracle_unlogged_run_and_generic(label, config, G, kernel, used, sweep, dtype):
    N = len(config["agents"])
    sw = None if sweep is None else _sweep(N, G, sweep == "noise")
    gb = _batch(config, G, dtype, kernel, sw).init_tables()
    q0, s0 = gb.tables_numpy(), gb.states_numpy()
    out = gb.run(E, per_game_logs=True)
    assert out["kernel"] == used, label
    logged = _state(gb)

    # the oracle: same tables, counters, state and epsilon bit for bit; per-game rows to 1e-12
    cfg, eps0 = O.cfg_from_config(config, n_games=G, q_dtype=1 if dtype == "float64" else 0)
    q, s, c = q0.copy(), s0.copy(), np.zeros(q0.shape, np.int32)
    osw = None if sw is None else {k: np.array(v, np.float64) for k, v in sw.items()}
    oo = O.episodes(cfg, q, c, s, eps0, O.Memory(cfg), E, seed=23, sweep=osw)
    _assert_same_state(logged, (q, c, s, osw["eps"] if osw and "eps" in osw else eps0), label)
    np.testing.assert_allclose(out["game_reward_log"], oo["game_reward_log"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(out["game_action_log"], oo["game_action_log"], rtol=1e-12, atol=1e-13)

    # logs do not perturb the run: the same run without them is bit-identical, mean logs included
    plain = _batch(config, G, dtype, kernel, sw)
    plain.set_tables(q0, s0)
    po = plain.run(E)
    assert po["kernel"] == used
    _assert_same_state(_state(plain), logged, label)
    if used == "wave":      # fixed-point sums: order independent, so the same bits
        assert np.array_equal(po["reward_log"], out["reward_log"]) and np.array_equal(po["action_log"], out["action_log"])
    else:                   # the tuple kernel sums with float64 atomics: the order varies, the logs agree to 1e-12
        np.testing.assert_allclose(po["reward_log"], out["reward_log"], rtol=1e-12)
        np.testing.assert_allclose(po["action_log"], out["action_log"], rtol=1e-12)
    np.testing.assert_allclose(out["game_reward_log"].mean(axis=2), out["reward_log"], rtol=1e-12)
    np.testing.assert_allclose(out["game_action_log"].mean(axis=2), out["action_log"], rtol=1e-12)

    # the generic kernel's sequential per-step sums agree to 1e-12
    gen = _batch(config, G, dtype, "generic", sw)
    gen.set_tables(q0, s0)
    go = gen.run(E, per_game_logs=True)
    assert go["kernel"] == "generic"
    _assert_same_state(_state(gen), logged, label)
    np.testing.assert_allclose(out["game_reward_log"], go["game_reward_log"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(out["game_action_log"], go["game_action_log"], rtol=1e-12, atol=1e-13)


def test_one_of_the_two_pointers():
    """The ABI allows either per-game array alone."""
    import ctypes
    import torch
    from th_rl_amd import _lib
    for config in (TWO, THREE):
        gb = _batch(config, 128, "float32", "auto", None).init_tables()
        ref = _batch(config, 128, "float32", "auto", None)
        ref.set_tables(gb.tables_numpy(), gb.states_numpy())
        want = ref.run(5, per_game_logs=True)
        for which in ("game_reward_log", "game_action_log"):
            gb2 = _batch(config, 128, "float32", "auto", None)
            gb2.set_tables(gb.tables_numpy(), gb.states_numpy())
            dst = torch.zeros((5, gb2.N, 128), dtype=torch.float64, device=gb2.device)
            b = _lib.Buffers()
            b.q, b.counter, b.state = gb2._ptr(gb2.q), gb2._ptr(gb2.counter), gb2._ptr(gb2.state)
            setattr(b, which, gb2._ptr(dst))
            b.workspace, b.workspace_bytes = gb2._ptr(gb2.workspace), gb2.workspace.numel()
            r = _lib.Run()
            r.seed, r.n_episodes, r.kernel = gb2.seed, 5, _lib.KERNEL_AUTO
            for i in range(gb2.N):
                r.eps[i] = gb2.eps[i]
            _lib.check(gb2.L.thrl_qtable_episodes(ctypes.byref(gb2.cfg), ctypes.byref(b), ctypes.byref(r), gb2._stream()),
                       "thrl_qtable_episodes")
            torch.cuda.synchronize()
            assert _lib.KERNEL_NAMES[r.kernel_used] in ("wave", "tuple")
            assert np.array_equal(dst.cpu().numpy(), want[which]), which


# ---------------------------------------------------------------------------------------------------- trainer
def _train(tmp_path, name, training, config=TWO):
    from th_rl_amd import trainer
    d = tmp_path / name
    cfg = dict(config, training=dict(training))
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps(cfg))
    trainer.train_one(str(d), str(p))
    return str(d)


def _log_csv(d):
    import pandas
    return pandas.read_csv(os.path.join(d, "log.csv"), header=[0, 1], float_precision="round_trip").to_numpy()


def test_trainer_game_logs_gamma_sweep(tmp_path):
    from th_rl_amd import utils
    from th_rl_amd.batched import GameBatch
    G, epochs = 64, 40
    gamma = [0.35] * (G // 2) + [0.95] * (G // 2)
    training = dict(epochs=epochs, print_freq=20, n_games=G, seed=5, sweep={"gamma": gamma}, game_logs=True)
    d = _train(tmp_path, "all", training)
    for f in ("game_rewards.npy", "game_actions.npy", "game_ids.npy"):
        assert os.path.isfile(os.path.join(d, f))
    assert np.array_equal(np.load(os.path.join(d, "game_ids.npy")), np.arange(G))
    assert np.load(os.path.join(d, "game_ids.npy")).dtype == np.int64

    gb = GameBatch(TWO, n_games=G, dtype="float32", seed=5, sweep={"gamma": gamma}).init_tables()
    ref = gb.run(epochs, per_game_logs=True)
    assert ref["kernel"] == "wave"
    for g in (0, 1, G // 2, G - 1):
        df = utils.game_log(d, g)
        assert list(df.columns) == [("rewards", 0), ("rewards", 1), ("actions", 0), ("actions", 1)]
        np.testing.assert_allclose(df["rewards"].to_numpy(), ref["game_reward_log"][:, :, g], rtol=1e-12)
        np.testing.assert_allclose(df["actions"].to_numpy(), ref["game_action_log"][:, :, g], rtol=1e-12)
    rew = np.load(os.path.join(d, "game_rewards.npy"))
    act = np.load(os.path.join(d, "game_actions.npy"))
    assert rew.shape == (epochs, 2, G) and rew.dtype == np.float64
    np.testing.assert_allclose(np.concatenate([rew.mean(axis=2), act.mean(axis=2)], axis=1), _log_csv(d), rtol=1e-12)

    # a list of ids keeps only those games; the run itself is the same
    d2 = _train(tmp_path, "some", dict(training, game_logs=[3, G - 2]))
    assert np.array_equal(np.load(os.path.join(d2, "game_ids.npy")), [3, G - 2])
    assert np.load(os.path.join(d2, "game_rewards.npy")).shape == (epochs, 2, 2)
    for g in (3, G - 2):
        np.testing.assert_allclose(utils.game_log(d2, g).to_numpy(), utils.game_log(d, g).to_numpy(), rtol=1e-12)
    with pytest.raises(KeyError):
        utils.game_log(d2, 0)
    assert np.array_equal(_log_csv(d2), _log_csv(d))


def test_trainer_game_logs_small_tabular_path(tmp_path):
    """Small float64 all-QTable batches train on the mixed-agent kernel (MixedGameBatch): the same files."""
    from th_rl_amd import utils
    d = _train(tmp_path, "small", dict(epochs=12, print_freq=5, n_games=4, seed=3, dtype="float64", game_logs=True))
    rew = np.load(os.path.join(d, "game_rewards.npy"))
    act = np.load(os.path.join(d, "game_actions.npy"))
    assert rew.shape == (12, 2, 4)
    np.testing.assert_allclose(np.concatenate([rew.mean(axis=2), act.mean(axis=2)], axis=1), _log_csv(d), rtol=1e-12)
    np.testing.assert_array_equal(utils.game_log(d, 2)["rewards"].to_numpy(), rew[:, :, 2])
