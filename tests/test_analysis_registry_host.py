"""The table of analyses (th_rl_amd.analysis.REGISTRY) against what it points at: the modules' parsers, writers and
merge hooks, launch's refusals, utils' readers, and the order the cross-dependencies need.  Host only."""
import importlib
import inspect

import pytest

from th_rl_amd import analysis, launch, utils

KEYS = [a.key for a in analysis.REGISTRY]
AGENT = dict(name="QTable", gamma=0.95, actions=5, states=10, alpha=0.1, eps_end=0.001, epsilon=0.5, eps_step=0.9995,
             action_range=[0.2, 0.4])
CONFIG = {"agents": [dict(AGENT), dict(AGENT)],
          "environment": dict(name="NoisyPriceState", noise_prob=0.05, a=10, b=1, nplayers=2, max_steps=10)}


def test_keys_are_unique_and_found_by_record():
    assert len(set(KEYS)) == len(KEYS) == 12
    for a in analysis.REGISTRY:
        assert analysis.record(a.key) is a
    with pytest.raises(KeyError):
        analysis.record("no_such_analysis")


@pytest.mark.parametrize("a", analysis.REGISTRY, ids=KEYS)
def test_module_has_the_parser_the_writer_and_the_merge_hook(a):
    mod = importlib.import_module("th_rl_amd." + a.module)
    parse, write = getattr(mod, a.parse), getattr(mod, a.write)
    assert parse(True, CONFIG) == parse({}, CONFIG)                    # the shared preamble: true is the empty dict
    with pytest.raises(ValueError, match=r"training\.%s: unknown keys \['no_such_option'\]" % a.key):
        parse({"no_such_option": 1}, CONFIG)
    with pytest.raises(ValueError, match=r"training\.%s must be true or a dict" % a.key):
        parse(3, CONFIG)
    params = inspect.signature(write).parameters
    assert list(params)[:6] == ["exp_path", "batch", "config", "opt", "ids", "n_groups"]
    # every keyword train_one passes for the record's flags is one the writer takes
    want = [name for name, _ in a.after]
    want += ["q", "state0"] if a.converged else []
    want += ["spec", "histograms", "budget"] if a.rows else []
    want += ["tuple_policy"] if a.tuple_policy else []
    want += ["tracker", "every", "episodes_run", "stopped_early"] if a.key == "convergence" else []
    assert sorted(want) == sorted(list(params)[6:])
    if a.converged:
        assert parse({"tables": "converged"}, CONFIG)["tables"] == "converged"
        with pytest.raises(ValueError, match=r"training\.%s\.tables must be 'final' or 'converged'" % a.key):
            parse({"tables": "first"}, CONFIG)
    else:
        with pytest.raises(ValueError, match="unknown keys"):
            parse({"tables": "converged"}, CONFIG)
    assert callable(getattr(mod, "merged", None)) == a.merge
    assert not a.copy or a.merge


def test_launch_refuses_exactly_the_records_without_a_merge():
    for a in analysis.REGISTRY:
        cfg = dict(CONFIG, training={"n_games": 4, "seed": 1, a.key: True})
        if a.merge:
            launch.check_launch_config(cfg)
        else:
            with pytest.raises(ValueError, match=r"training\.%s is not available under th_rl_amd\.launch" % a.key):
                launch.check_launch_config(cfg)
        launch.check_launch_config(dict(CONFIG, training={a.key: False}))
        launch.check_launch_config(dict(CONFIG, training={a.key: None}))
    with pytest.raises(ValueError, match="no sharded merge"):
        launch.merge_analysis("sampled_play", CONFIG, "unused", 2)


def test_a_shard_carries_the_global_groups_for_every_merged_key():
    sweep = {"gamma": [0.5, 0.5, 0.9, 0.9]}
    for a in analysis.REGISTRY:
        if a.merge:
            cfg = dict(CONFIG, training={"n_games": 4, "seed": 1, "sweep": sweep, a.key: True})
            training, offset, n_local = launch.shard_training(cfg, 1, 2)
            assert (training["groups"], training["n_groups"], offset, n_local) == ([1, 1], 2, 2, 2), a.key


def test_utils_has_a_summary_and_a_games_reader_for_each_record(tmp_path):
    readers = [a.reader for a in analysis.REGISTRY]
    assert len(set(readers)) == len(readers)
    for a in analysis.REGISTRY:
        assert callable(getattr(utils, a.reader + "_summary")), a.key
        games = getattr(utils, a.reader + "_games")
        with pytest.raises(KeyError, match=r"under .* \(training\.%s\)" % a.key):       # nothing there: the key is named
            games(str(tmp_path))


def test_order_is_execution_order():
    at = {k: i for i, k in enumerate(KEYS)}
    assert at["deviation"] < at["equilibrium"]                       # equilibrium reads dev_cycle_reward.npy
    assert at["attractors"] < at["stationary"]                       # stationary uses attractors' reset_reward
    assert at["greedy_deviation"] < at["greedy_equilibrium"]         # greedy equilibrium takes its cycle_reward
    assert at["greedy_cycles"] < at["sampled_play"]                  # sampled play checks whether greedy cycles ran
    assert KEYS == ["convergence", "deviation", "equilibrium", "crossplay", "attractors", "stationary", "greedy_cycles",
                    "greedy_deviation", "greedy_equilibrium", "greedy_attractors", "greedy_stationary", "sampled_play"]
    for a in analysis.REGISTRY:                                      # what a writer is handed was written before it
        for _, key in a.after:
            assert at[key] < at[a.key], (a.key, key)
    assert dict(analysis.record("stationary").after) == {"with_attractors": "attractors"}
    assert dict(analysis.record("greedy_equilibrium").after) == {"deviation": "greedy_deviation"}
    assert dict(analysis.record("sampled_play").after) == {"with_cycles": "greedy_cycles"}


def test_both_batch_classes_share_the_analysis_methods():
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    names = [a.key for a in analysis.REGISTRY if a.key != "convergence"] + ["track_convergence"]
    for name in names:
        fn = getattr(analysis.AnalysisMethods, name)
        assert getattr(GameBatch, name) is fn and getattr(MixedGameBatch, name) is fn and fn.__doc__, name
