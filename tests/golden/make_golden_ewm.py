#!/usr/bin/env python3
"""Fixture G13: the smoothed learning curves the REFERENCE's analysis works with.

  rewards / actions   the two frames th_rl.utils.load_experiment returns for the committed run
                      tests/golden/ref_run_example_config (201 rows x 2 agents): log.csv read with pandas and
                      smoothed per column with .ewm(halflife=1000).mean()
  log_rewards / log_actions   the raw columns of that log.csv, as load_experiment read them
  x, ewm_h1 / ewm_h3 / ewm_h8   a stored 64 x 4 random input and pandas' x.ewm(halflife=h).mean() of it

load_experiment is called from the reference's own utils module when that imports here (it needs plotly and click
at import time); otherwise this script applies the same one pandas line (utils.py:20-21) to the same log.csv itself.
The field `source` says which of the two happened.  Data only.
Usage: python tests/golden/make_golden_ewm.py"""
import os
import sys

import numpy
import pandas

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
RUN = os.path.join(HERE, "ref_run_example_config")


def frames():
    log = pandas.read_csv(os.path.join(RUN, "log.csv"))
    try:
        sys.dont_write_bytecode = True
        sys.path.insert(0, REF)
        from th_rl.utils import load_experiment
        _, _, _, actions, rewards = load_experiment(RUN)
        source = "th_rl.utils.load_experiment"
    except Exception as e:      # the plotting imports are missing: the same line, applied here
        print("reference utils not usable here (%s: %s): applying its ewm line directly" % (type(e).__name__, e))
        rewards = log[["rewards", "rewards.1"]].ewm(halflife=1000).mean()
        actions = log[["actions", "actions.1"]].ewm(halflife=1000).mean()
        source = "pandas ewm(halflife=1000).mean() applied by make_golden_ewm.py"
    return (log[["rewards", "rewards.1"]].to_numpy(), log[["actions", "actions.1"]].to_numpy(),
            rewards.to_numpy(), actions.to_numpy(), source)


def main():
    log_r, log_a, rew, act, source = frames()
    x = numpy.random.RandomState(13).uniform(-1.0, 25.0, (64, 4))
    out = dict(log_rewards=log_r, log_actions=log_a, rewards=rew, actions=act, halflife=numpy.array(1000.0),
               source=numpy.array(source), x=x, pandas_version=numpy.array(pandas.__version__))
    for h in (1, 3, 8):
        out["ewm_h%d" % h] = pandas.DataFrame(x).ewm(halflife=h).mean().to_numpy()
    p = os.path.join(HERE, "g13_ewm_curves.npz")
    numpy.savez_compressed(p, **out)
    print("wrote", p, source, rew.shape, act.shape)


if __name__ == "__main__":
    main()
