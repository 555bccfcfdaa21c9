"""train_one's analysis loop on the device (th_rl_amd.analysis.REGISTRY): the analyses only read the batch, so the
per-game .npy files a key writes are byte-identical whether it runs alone or beside every other key, and every
record's readers in utils load the result.  A tiny all-QTable run (8 games, 5 actions, 20 epochs, fixed seed): the
reference run with all twelve keys is trained once, then one run per key."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

G = 8
AG = dict(name="QTable", gamma=0.95, actions=5, states=20, alpha=0.1, eps_end=0.001, epsilon=0.5, eps_step=0.9995,
          action_range=[0.2, 0.4])
CONFIG = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)],
          "environment": dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=25)}
TRAINING = {"epochs": 20, "print_freq": 500, "seed": 5, "n_games": G, "n_groups": 2, "groups": [0] * 4 + [1] * 4}
# key -> (its options here, the prefix of its per-game files, the stem of its readers in utils)
KEYS = {
    "convergence": ({"window": 4, "every": 4, "snapshot": True}, "conv_", "convergence"),
    "deviation": ({"steps": 8}, "dev", "deviation"),
    "equilibrium": (True, "eq_", "equilibrium"),
    "crossplay": ({"rounds": 2}, "xplay_", "crossplay"),
    "attractors": (True, "attr_", "attractor"),
    "stationary": ({"noise_prob": 0.05}, "stat_", "stationary"),
    "greedy_cycles": ({"rounds": 1}, "gcyc_", "greedy_cycle"),
    "greedy_deviation": ({"steps": 8}, "gdev", "greedy_deviation"),
    "greedy_equilibrium": (True, "geq_", "greedy_equilibrium"),
    "greedy_attractors": (True, "gattr_", "greedy_attractor"),
    "greedy_stationary": ({"noise_prob": 0.05, "resolution": 64}, "gstat_", "greedy_stationary"),
    "sampled_play": (True, "splay_", "sampled_play"),
}


def _train(d, keys):
    from th_rl_amd import trainer
    cfg = dict(CONFIG, training=dict(TRAINING, **{k: KEYS[k][0] for k in keys}))
    path = os.path.join(str(d), "c.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    exp = os.path.join(str(d), "run")
    trainer.train_one(exp, path)
    return exp


def _files(exp, prefix):
    return {n: open(os.path.join(exp, n), "rb").read() for n in sorted(os.listdir(exp))
            if n.startswith(prefix) and n.endswith(".npy")}


@pytest.fixture(scope="module")
def together(tmp_path_factory):
    return _train(tmp_path_factory.mktemp("together"), list(KEYS))


def test_the_table_here_is_the_registry():
    from th_rl_amd import analysis
    assert [(a.key, a.reader) for a in analysis.REGISTRY] == [(k, v[2]) for k, v in KEYS.items()]


@pytest.mark.parametrize("key", list(KEYS))
def test_a_key_alone_writes_the_files_it_writes_beside_the_others(key, together, tmp_path):
    prefix = KEYS[key][1]
    alone, beside = _files(_train(tmp_path, [key]), prefix), _files(together, prefix)
    assert alone and sorted(alone) == sorted(beside)
    for name in alone:
        assert alone[name] == beside[name], name
    other = [n for k, v in KEYS.items() if k != key for n in _files(os.path.join(str(tmp_path), "run"), v[1])]
    assert not other, other                                     # and nothing of a key that was not asked for


def test_every_record_has_readers_that_load_the_run(together):
    from th_rl_amd import utils
    for key, (_, _, reader) in KEYS.items():
        summary = getattr(utils, reader + "_summary")(together)
        for df in summary if isinstance(summary, tuple) else (summary,):
            assert len(df.columns), key
        assert len(summary[0] if isinstance(summary, tuple) else summary) >= 2, key       # a row per group at least
        games = getattr(utils, reader + "_games")(together)
        assert games.index.tolist() == list(range(G)), key
