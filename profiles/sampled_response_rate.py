"""Rate of the best responses to sampled play (thrl_sampled_response), float32 tables, networks with kinks inside the
price range:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = D = 441, --games games after 20 training episodes, epsilon where
          training stopped, both agents solved at --gamma (default: each agent's own, 0.95 and 0.995), eval_tol 1e-12, at
          most 8,192 sweeps per evaluation; the rows, the strategies and the long-run distribution pi are computed once,
          outside the timed call

It records games/s, (agent, game) pairs/s and sweeps/s (the sweeps of all pairs over the time), the share of pairs capped,
and the sweep and round counts, beside sampled_play's chain on the same batch (the neighbouring exact iteration on the
same rows).

    python profiles/sampled_response_rate.py [--games N] [--gamma X] [--repeat R] [--out profiles/sampled_response_rate.json]

Times are device events around the calls (outputs allocated by the runner's own code path and their copies to the host
are included), median of `--repeat` after a warm-up, with the spread (min, max); games/s is games over the median."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sampled_play_rate import kinked  # noqa: E402
from tuple_attractors_rate import CONFIGS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "sampled_response_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, sampled_play as sp, sampled_response as sr, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    G = a.games
    config = CONFIGS["MIXED"]
    mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
    tabs = sp.tables(config)
    kinked(mb, tabs, torch, G)
    mb.run(20, per_game_logs=False)
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    ws = sr.working_set(config, tabs)
    r = {"games": G, "tuples": T, "prices": D, "lds_bytes": ws["bytes"], "team": ws["team"], "eval_tol": 1e-12,
         "max_sweeps": 8192, "epsilon": [float(x) for x in list(mb.eps)[:mb.N]]}
    probs, dpol = sp.price_probs(mb, tabs["dprice"]), ts.price_policy(mb, tabs["dprice"])
    out = {}
    r["chain"] = timed(lambda: out.update(s=mb.sampled_play(pi=True, probs=probs, dpolicy=dpol, tabs=tabs)), a.repeat, torch, G)
    pi = out["s"]["pi"]
    print(json.dumps({"chain": r["chain"]}), flush=True)
    r["response"] = timed(lambda: out.update(x=mb.sampled_response(gamma=a.gamma, pi=pi, probs=probs, dpolicy=dpol, tabs=tabs)),
                          a.repeat, torch, G)
    x = out["x"]
    ok = x["iters"] >= 0
    sec = r["response"]["median_ms"] * 1e-3
    r.update(gamma=[float(g) for g in x["gamma"][:, 0]], pairs_per_s=float(x["iters"].size) / sec,
             sweeps_per_s=float(x["sweeps"].sum()) / sec, capped=float((~ok).mean()),
             sweeps_mean=[float(v) for v in x["sweeps"].mean(axis=1)], sweeps_max=int(x["sweeps"].max()),
             iters_mean=[float(x["iters"][i][ok[i]].mean()) if ok[i].any() else None for i in range(mb.N)],
             iters_max=int(x["iters"].max()), br_prob_w_mean=[float(np.nanmean(v)) for v in x["br_prob_w"]],
             response_over_chain=r["response"]["median_ms"] / r["chain"]["median_ms"])
    res["MIXED"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
