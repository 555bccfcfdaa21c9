"""Rate of sampled play under demand noise (thrl_sampled_noise_chain), float32 tables, networks with kinks inside the price
range: QTable vs Reinforce, 21 x 21 actions, T = D = 441, 65,536 games after 20 training episodes, epsilon where training
stopped, noise_prob 0.05, resolution 1024 (1,121 nodes), from the uniform distribution, tol 1e-12, at most --max-iters
steps.  For scale it records thrl_sampled_chain (the noise-free half of the step) and thrl_tuple_stationary (greedy play
under the same noise) on the same batch, and for each steps per second (games x mean steps over the time), the mean
steps, the share of games within tol and the largest mass error; for the noisy chain also the largest max_jump and the
per-step cost against thrl_sampled_chain's, to be read beside (D + Jn) / D.

    python profiles/sampled_noise_rate.py [--games N] [--max-iters K] [--out profiles/sampled_noise_rate.json]

Times are device events around the calls (outputs allocated by the runners' own code paths and their copies to the host
are included), median of `--repeat` after a warm-up, with the spread (min, max)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sampled_play_rate import kinked, steps  # noqa: E402
from tuple_attractors_rate import CONFIGS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--noise-prob", type=float, default=0.05)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(HERE, "sampled_noise_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, sampled_play as sp, tuple_play as tp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    G, config = a.games, CONFIGS["MIXED"]
    mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
    tabs = sp.noise_tables(config, a.resolution)
    kinked(mb, tabs, torch, G)
    mb.run(20, per_game_logs=False)
    T, D, Jn = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"])
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}, "games": G, "tuples": T, "prices": D,
           "nodes": Jn, "band_w": int(tabs["band_w"]), "noise_prob": a.noise_prob, "resolution": a.resolution, "tol": 1e-12,
           "max_iters": a.max_iters, "lds_bytes": sp.working_set(config, tabs, n_nodes=Jn)["bytes"],
           "lds_bytes_noise_free": sp.working_set(config, tabs)["bytes"], "epsilon": [float(x) for x in list(mb.eps)[:mb.N]]}
    probs, dpol = sp.price_probs(mb, tabs["dprice"]), ts.price_policy(mb, tabs["dprice"])
    nprobs, npol = sp.price_probs(mb, tabs["xn"]), ts.price_policy(mb, tabs["xn"])
    out = {}

    def record(name, call, key):
        t = timed(lambda: out.update({key: call()}), a.repeat, torch, G)
        s = out[key]
        r = dict(steps(t, s, G), converged=float((s["iters"] < a.max_iters).mean()),
                 mass_error_max=float(np.abs(s["mass"] - 1.0).max()))
        r["time"] = t
        r["ms_per_step_per_kgame"] = t["median_ms"] / (r["iters_mean"] * G / 1000.0)
        res[name] = r
        return r

    n = record("sampled_noise_chain", lambda: mb.sampled_play(
        max_iters=a.max_iters, probs=probs, dpolicy=dpol, tabs=tabs, noise_prob=a.noise_prob, nprobs=nprobs, npolicy=npol), "n")
    n["max_jump_max"] = float(out["n"]["max_jump"].max())
    n["agree_mean"] = float(out["n"]["agree"].mean())
    p = record("sampled_chain", lambda: mb.sampled_play(max_iters=a.max_iters, probs=probs, dpolicy=dpol, tabs=tabs), "p")
    stabs = ts.tables(config, a.resolution)
    pol, cells = tp.extract(mb, stabs), ts.extract_cells(mb, stabs)
    record("tuple_stationary", lambda: mb.greedy_stationary(noise_prob=a.noise_prob, max_iters=a.max_iters, tuple_policy=pol,
                                                            cell_policy=cells, tabs=stabs), "g")
    res["step_cost_over_sampled_chain"] = n["ms_per_step_per_kgame"] / p["ms_per_step_per_kgame"]
    res["multiplications_ratio"] = float(D + Jn) / D
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
