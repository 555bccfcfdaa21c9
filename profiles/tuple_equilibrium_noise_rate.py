"""Time of the equilibrium check under demand noise in tuple form (thrl_tuple_equilibrium_noise) on trained games of the
reference's example pairing (QTable gamma 0.95 against Reinforce gamma 0.995, 21 actions each, 100 states,
NoisyPriceState noise_prob 0.05), resolution 1024, float32, both agents, beside its yardsticks on the same batch and
the same extracted strategies in the same process:

  extract            tuple_play.extract + tuple_stationary.extract_cells (thrl_tuple_policy, thrl_price_policy)
  stationary         tuple_stationary.run with pi stored (thrl_tuple_stationary): the weights of the check
  equilibrium        tuple_analysis.equilibrium, the noise-free check (thrl_tuple_equilibrium), both agents
  noise              tuple_analysis.equilibrium_noise with that pi, eval_tol 1e-12, max_sweeps 8192
  noise_1e-9         the same at eval_tol 1e-9
  iters, sweeps      the distribution of the rounds and of the evaluation sweeps per (agent, game), per agent too

    python profiles/tuple_equilibrium_noise_rate.py [--games N] [--episodes E] [--out profiles/tuple_equilibrium_noise_rate.json]

Times are wall-clock around the module-level calls between device synchronisations (the upload of the tables and the
download of the per-game outputs included), median of `--repeat` after a warm-up, with the spread (min, max)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENV = dict(name="NoisyPriceState", noise_prob=0.05, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001, epsilon=0.5,
                       eps_step=0.9995, action_range=[0.2, 0.4]),
                  dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
       "environment": dict(ENV)}


def timed(fn, repeat, torch):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def stats(x):
    x = np.asarray(x)
    q = np.quantile(x, [0.25, 0.5, 0.75])
    return {"min": int(x.min()), "q25": float(q[0]), "q50": float(q[1]), "q75": float(q[2]), "max": int(x.max()),
            "mean": float(x.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, tuple_analysis as ta, tuple_play as tp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    G = a.games
    mb = MixedGameBatch(CFG, n_games=G, dtype="float32", seed=1).init_tables()
    mb.run(a.episodes, per_game_logs=False)
    tabs = ts.tables(CFG, a.resolution)
    T, J, W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
    pols = {}

    def extract():
        pols["t"], pols["c"] = tp.extract(mb, tabs), ts.extract_cells(mb, tabs)

    res = {"games": G, "episodes": a.episodes, "resolution": a.resolution, "n_tuples": T, "n_cells": J, "band_w": W,
           "lds_bytes": (44 * T + 28 * J + 2048 + 15) // 16 * 16, "noise_prob": 0.05, "agents": [0, 1], "gamma": [0.95, 0.995],
           "max_sweeps": 8192, "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["extract"] = timed(extract, a.repeat, torch)
    st = {}

    def stationary():
        st.update(ts.run(mb, pi=True, tuple_policy=pols["t"], cell_policy=pols["c"], tabs=tabs))

    res["stationary"] = timed(stationary, a.repeat, torch)
    res["stationary_iters"] = stats(st["iters"])
    res["equilibrium"] = timed(lambda: ta.equilibrium(mb, tuple_policy=pols["t"], tabs=tabs), a.repeat, torch)
    out = {}

    def noise(eval_tol):
        out.update(ta.equilibrium_noise(mb, eval_tol=eval_tol, tuple_policy=pols["t"], cell_policy=pols["c"],
                                        weights=st["pi"], tabs=tabs))

    res["noise"] = timed(lambda: noise(1e-12), a.repeat, torch)
    it, sw = out["iters"], out["sweeps"]
    res["capped"] = int((it < 0).sum())
    res["iters"], res["sweeps"] = stats(it[it >= 0]), stats(sw)
    res["sweeps_agent"] = [stats(sw[i]) for i in range(2)]
    res["br_all"] = float(out["br_all"].mean())
    res["br_w"] = float(out["br_w"].mean())
    res["n_diff_tuples_mean"], res["n_diff_cells_mean"] = float(out["n_diff_tuples"].mean()), float(out["n_diff_cells"].mean())
    res["solves_per_s"] = 2 * G / (res["noise"]["median_ms"] * 1e-3)
    res["tuple_updates_per_s"] = float(sw.sum()) * T / (res["noise"]["median_ms"] * 1e-3)
    res["noise_1e-9"] = timed(lambda: noise(1e-9), a.repeat, torch)
    res["sweeps_1e-9"] = stats(out["sweeps"])
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
