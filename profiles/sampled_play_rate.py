"""Rate of sampled play (thrl_price_probs + thrl_sampled_chain), float32 tables, networks with kinks inside the price
range:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = D = 441, 65,536 games after 20 training episodes, epsilon where
          training stopped, from the uniform distribution, tol 1e-12, at most --max-iters steps
  RR      2 x Reinforce on one exact grid, 21 x 21 actions, T = 441, D = 41, the same games count and options

It records thrl_price_probs beside thrl_price_policy at the same D prices (the second is the yardstick of the first:
the same network evaluation, an argmax kept against A floats stored) and the chain beside thrl_tuple_stationary's chain
on the same MIXED batch (the neighbouring exact Markov-chain iteration: resolution 1024, noise_prob 0.05, the same cap),
with games/s and steps/s (games x mean steps over the time) for each.

    python profiles/sampled_play_rate.py [--games N] [--max-iters K] [--out profiles/sampled_play_rate.json]

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


def kinked(mb, tabs, torch, G):
    """Up to 4,096 distinct networks whose softmax moves with the price, fc_pi four times larger in three games of four."""
    rs = np.random.RandomState(0)
    n = min(G, 4096)
    for rb in mb.nn.values():
        w = np.zeros((n, rb.P), np.float32)
        w1 = rs.uniform(-1, 1, (n, 256))
        w[:, :256], w[:, 256:512] = w1, -w1 * rs.uniform(tabs["price"].min(), tabs["price"].max(), (n, 256))
        n2 = rb.A * 256 + rb.A
        pi = rs.uniform(-1, 1, (n, n2)) / 4.0
        pi[np.arange(n) % 4 != 0] *= 4.0
        w[:, 512:512 + n2] = pi
        rb.params.copy_(torch.from_numpy(w).to(mb.device).repeat((G + n - 1) // n, 1)[:G])


def steps(t, s, G):
    it = s["iters"][s["iters"] >= 0]
    t["steps_per_s"] = float(it.sum()) / (t["median_ms"] * 1e-3)
    return dict(iters_mean=float(it.mean()), iters_max=int(it.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(HERE, "sampled_play_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, sampled_play as sp, tuple_play as tp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    G = a.games
    rf = dict(CONFIGS["MIXED"]["agents"][1], action_range=[0.125, 0.125 + 21.0 / 128.0])
    cases = {"MIXED": CONFIGS["MIXED"], "RR": {"agents": [dict(rf), dict(rf)], "environment": CONFIGS["MIXED"]["environment"]}}
    for name, config in cases.items():
        mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
        tabs = sp.tables(config)
        kinked(mb, tabs, torch, G)
        mb.run(20, per_game_logs=False)
        T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
        r = {"games": G, "tuples": T, "prices": D, "lds_bytes": sp.working_set(config, tabs)["bytes"], "tol": 1e-12,
             "max_iters": a.max_iters, "epsilon": [float(x) for x in list(mb.eps)[:mb.N]]}
        r["price_policy"] = timed(lambda: ts.price_policy(mb, tabs["dprice"]), a.repeat, torch, G)
        r["price_probs"] = timed(lambda: sp.price_probs(mb, tabs["dprice"]), a.repeat, torch, G)
        r["probs_over_policy"] = r["price_probs"]["median_ms"] / r["price_policy"]["median_ms"]
        probs, dpol = sp.price_probs(mb, tabs["dprice"]), ts.price_policy(mb, tabs["dprice"])
        out = {}
        r["chain"] = timed(lambda: out.update(s=mb.sampled_play(max_iters=a.max_iters, probs=probs, dpolicy=dpol, tabs=tabs)),
                           a.repeat, torch, G)
        s = out["s"]
        r.update(steps(r["chain"], s, G), converged=float((s["iters"] < a.max_iters).mean()),
                 agree_mean=float(s["agree"].mean()), mass_error_max=float(np.abs(s["mass"] - 1.0).max()))
        if name == "MIXED":                      # the neighbouring chain on the same batch
            stabs = ts.tables(config, 1024)
            pol, cells = tp.extract(mb, stabs), ts.extract_cells(mb, stabs)
            r["tuple_stationary_chain"] = timed(lambda: out.update(n=mb.greedy_stationary(
                noise_prob=0.05, max_iters=a.max_iters, tuple_policy=pol, cell_policy=cells, tabs=stabs)), a.repeat, torch, G)
            r["tuple_stationary"] = dict(steps(r["tuple_stationary_chain"], out["n"], G), cells=int(stabs["n_cells"]))
        res[name] = r
        del mb
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
