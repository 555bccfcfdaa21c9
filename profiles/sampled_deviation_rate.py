"""Rate of the deviation test of sampled play (thrl_sampled_deviation), float32 tables, networks with kinks inside the
price range:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = D = 441, --games games after 20 training episodes, epsilon where
          training stopped, both deviators, K = --steps periods of which L = 1 deviates to the one-period best response;
          the rows, the strategies and the long-run distribution pi are computed once, outside the timed call

It records games/s for the deviation call alone (both deviators: two calls) and for the sampled_play(pi=True) call it rests
on, and their ratio beside the prediction from the operation counts: a period costs one non-lazy chain step, T D N
multiplications, so the K + 1 distributions a deviator's call evaluates should cost about (K + 1) / iters of the
stationary call on the same games.  The prediction was made before anything had measured this kernel.

    python profiles/sampled_deviation_rate.py [--games N] [--steps K] [--repeat R] [--out profiles/sampled_deviation_rate.json]

Times are device events around the calls (outputs allocated by the runner's own code path and their copies to the host
are included), median of `--repeat` after a warm-up, with the spread (min, max); games/s is games over the median."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sampled_play_rate import kinked  # noqa: E402
from tuple_attractors_rate import CONFIGS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "sampled_deviation_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, sampled_deviation as sd, sampled_play as sp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    G, K = a.games, a.steps
    config = CONFIGS["MIXED"]
    mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
    tabs = sp.tables(config)
    kinked(mb, tabs, torch, G)
    mb.run(20, per_game_logs=False)
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    r = {"games": G, "tuples": T, "prices": D, "steps": K, "dev_len": 1, "action": "best_response",
         "lds_bytes": sd.working_set(config, tabs)["bytes"], "epsilon": [float(x) for x in list(mb.eps)[:mb.N]]}
    probs, dpol = sp.price_probs(mb, tabs["dprice"]), ts.price_policy(mb, tabs["dprice"])
    out = {}
    r["chain"] = timed(lambda: out.update(s=mb.sampled_play(pi=True, probs=probs, dpolicy=dpol, tabs=tabs)), a.repeat, torch, G)
    pi, iters = out["s"]["pi"], out["s"]["iters"]
    print(json.dumps({"chain": r["chain"]}), flush=True)

    def both():
        for d in range(mb.N):
            out[d] = mb.sampled_deviation(deviator=d, steps=K, weights=pi, probs=probs, dpolicy=dpol, tabs=tabs)
    r["deviation"] = timed(both, a.repeat, torch, G)
    ratio = r["deviation"]["median_ms"] / r["chain"]["median_ms"]
    predicted = mb.N * (K + 1) / float(iters.mean())
    r.update(chain_iters_mean=float(iters.mean()), chain_iters_max=int(iters.max()), deviation_over_chain=ratio,
             predicted_over_chain=predicted, measured_over_predicted=ratio / predicted,
             prediction="N deviators x (K + 1) distributions / the mean steps of the stationary call; made from the operation "
                        "counts before anything had measured this kernel",
             dev_share_mean=[float(out[d]["dev_share"].mean()) for d in range(mb.N)],
             unprofitable=[float((out[d]["gain"] < 0).mean()) for d in range(mb.N)],
             returned=[float((out[d]["ret_step"] >= 0).mean()) for d in range(mb.N)],
             mass_error_max=max(float(abs(out[d]["mass"] - 1.0).max()) for d in range(mb.N)))
    res["MIXED"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
