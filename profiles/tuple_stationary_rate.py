"""Rate of the stationary analysis in tuple form (thrl_price_policy + thrl_tuple_stationary), float32 tables, networks
with kinks inside the price range:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = 441, 65,536 games after 20 training episodes, resolution 1024
          (about 1,100 cells), noise_prob 0.05, from the reset distribution, tol 1e-12, at most 200 steps

It records the extraction at the cell midpoints (thrl_price_policy) beside thrl_tuple_policy on the same batch -- the
second is the yardstick of the first: the same kernels, T prices against J -- with the cost per price of each and
their ratio, and the chain's games per second with the steps it took.

    python profiles/tuple_stationary_rate.py [--games N] [--max-iters K] [--out profiles/tuple_stationary_rate.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/tuple_stationary_rate.py --repeat 1

Times are device events around the calls (outputs allocated by the runners' own code paths and their copies to the host
are included), median of `--repeat` after a warm-up, with the spread (min, max); games/s is games over the median."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from tuple_attractors_rate import CONFIGS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(HERE, "tuple_stationary_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, tuple_play as tp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    config, G = CONFIGS["MIXED"], a.games
    mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
    tabs = ts.tables(config, a.resolution)
    rs = np.random.RandomState(0)
    n = min(G, 4096)
    for rb in mb.nn.values():               # up to 4,096 distinct networks whose greedy action moves with the price
        w = np.zeros((n, rb.P), np.float32)
        w1 = rs.uniform(-1, 1, (n, 256))
        w[:, :256], w[:, 256:512] = w1, -w1 * rs.uniform(tabs["price"].min(), tabs["price"].max(), (n, 256))
        n2 = rb.A * 256 + rb.A
        w[:, 512:512 + n2] = rs.uniform(-1, 1, (n, n2))
        rb.params.copy_(torch.from_numpy(w).to(mb.device).repeat((G + n - 1) // n, 1)[:G])
    mb.run(20, per_game_logs=False)
    T, J = int(tabs["n_tuples"]), int(tabs["n_cells"])
    r = {"games": G, "tuples": T, "cells": J, "band_w": int(tabs["band_w"]), "resolution": a.resolution,
         "noise_prob": 0.05, "tol": 1e-12, "max_iters": a.max_iters}
    r["tuple_policy"] = timed(lambda: tp.extract(mb, tabs), a.repeat, torch, G)
    r["price_policy"] = timed(lambda: ts.extract_cells(mb, tabs), a.repeat, torch, G)
    per_t = r["tuple_policy"]["median_ms"] / T
    per_j = r["price_policy"]["median_ms"] / J
    r["ms_per_price"] = {"tuple_policy": per_t, "price_policy": per_j, "ratio": per_j / per_t}
    pol, cells = tp.extract(mb, tabs), ts.extract_cells(mb, tabs)
    out = {}
    r["chain"] = timed(lambda: out.update(s=mb.greedy_stationary(noise_prob=0.05, max_iters=a.max_iters, tuple_policy=pol,
                                                                 cell_policy=cells, tabs=tabs)), a.repeat, torch, G)
    s = out["s"]
    r.update(iters_mean=float(s["iters"].mean()), iters_max=int(s["iters"].max()),
             converged=float((s["iters"] < a.max_iters).mean()), n_switch_mean=float(s["n_switch"].mean()),
             n_switch_max=int(s["n_switch"].max()), unresolved_mean=float(s["unresolved"].mean()),
             unresolved_max=float(s["unresolved"].max()), mass_error_max=float(np.abs(s["mass"] - 1.0).max()))
    res["MIXED"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
