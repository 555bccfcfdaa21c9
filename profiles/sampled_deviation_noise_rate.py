"""Rate of the deviation test of sampled play under demand noise (thrl_sampled_deviation_noise), float32 tables, networks
with kinks inside the price range:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = D = 441, Jn = 1,121 nodes (resolution 1024), noise_prob 0.05, --games
          games after 20 training episodes, epsilon where training stopped, both deviators, K = --steps periods of which
          L = 1 deviates to the one-period best response; the rows at the prices and at the nodes, the strategies and the
          long-run distribution pi are computed once, outside the timed call

It records games/s for the deviation call alone (both deviators: two calls), for the sampled_play(noise, pi=True) call it
rests on with its mean step count, and for the noise-free sampled_deviation on the same games, and the ratios beside the
prediction from the operation counts: a period costs one non-lazy step of the noise chain, T (D + Jn) N multiplications,
so the K + 1 distributions a deviator's call evaluates should cost about (K + 1) / iters of the stationary call on the
same games, and the best-response pass over the S = D + Jn states adds S T (N - 1) once per game, S T (N - 1) / (T S N) =
(N - 1) / N of a step.  The prediction was made before anything had measured this kernel.

    python profiles/sampled_deviation_noise_rate.py [--games N] [--steps K] [--repeat R] [--step-timeout S]
                                                    [--out profiles/sampled_deviation_noise_rate.json]

Times are device events around the calls (outputs allocated by the runner's own code path and their copies to the host
are included), median of `--repeat` after a warm-up, with the spread (min, max); games/s is games over the median.  Every
GPU step runs under its own time limit: a step that passes --step-timeout seconds ends the process with a traceback."""
import argparse
import faulthandler
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
    ap.add_argument("--noise-prob", type=float, default=0.05)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--step-timeout", type=float, default=240)
    ap.add_argument("--out", default=os.path.join(HERE, "sampled_deviation_noise_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, sampled_deviation as sd, sampled_play as sp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch

    def step(what, fn):
        faulthandler.dump_traceback_later(a.step_timeout, exit=True)
        out = fn()
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()
        print(json.dumps({what: out if isinstance(out, dict) and "median_ms" in out else "done"}), flush=True)
        return out

    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    G, K, p = a.games, a.steps, a.noise_prob
    config = CONFIGS["MIXED"]
    tabs = sp.noise_tables(config, a.resolution)
    T, D, Jn = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"])
    ws = sd.working_set_noise(config, tabs=tabs, n_nodes=Jn)
    cu_lds = 160 * 1024
    r = {"games": G, "tuples": T, "prices": D, "nodes": Jn, "noise_prob": p, "resolution": a.resolution, "steps": K, "dev_len": 1,
         "action": "best_response", "lds_bytes": ws["bytes"], "blocks_per_cu": cu_lds // ws["bytes"],
         "noise_free_lds_bytes": sd.working_set(config, tabs)["bytes"]}

    def prepare():
        mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
        kinked(mb, tabs, torch, G)
        mb.run(20, per_game_logs=False)
        rows = dict(probs=sp.price_probs(mb, tabs["dprice"]), dpolicy=ts.price_policy(mb, tabs["dprice"]), tabs=tabs)
        nodes = dict(nprobs=sp.price_probs(mb, tabs["xn"]), npolicy=ts.price_policy(mb, tabs["xn"]))
        return mb, rows, nodes
    mb, rows, nodes = step("prepare", prepare)
    r["epsilon"] = [float(x) for x in list(mb.eps)[:mb.N]]
    out = {}
    r["chain"] = step("chain", lambda: timed(lambda: out.update(s=mb.sampled_play(pi=True, noise_prob=p, **rows, **nodes)),
                                             a.repeat, torch, G))
    pi, iters = out["s"]["pi"], out["s"]["iters"]

    def both():
        for d in range(mb.N):
            out[d] = mb.sampled_deviation_noise(deviator=d, steps=K, weights=pi, noise_prob=p, **rows, **nodes)
    r["deviation"] = step("deviation", lambda: timed(both, a.repeat, torch, G))

    def free():
        for d in range(mb.N):
            out["free%d" % d] = mb.sampled_deviation(deviator=d, steps=K, weights=pi, **rows)
    r["noise_free_deviation"] = step("noise_free_deviation", lambda: timed(free, a.repeat, torch, G))
    ratio = r["deviation"]["median_ms"] / r["chain"]["median_ms"]
    N = mb.N
    predicted = N * (K + 1 + (N - 1.0) / N) / float(iters.mean())
    r.update(chain_iters_mean=float(iters.mean()), chain_iters_max=int(iters.max()), deviation_over_chain=ratio,
             predicted_over_chain=predicted, measured_over_predicted=ratio / predicted,
             deviation_over_noise_free=r["deviation"]["median_ms"] / r["noise_free_deviation"]["median_ms"],
             predicted_over_noise_free=float(D + Jn) / D,
             prediction="N deviators x ((K + 1) distributions + (N - 1) / N of a step for the best-response pass) / the mean steps "
                        "of the stationary call under the same noise; against the noise-free test (D + Jn) / D, the states a "
                        "step walks; made from the operation counts before anything had measured this kernel",
             dev_share_mean=[float(out[d]["dev_share"].mean()) for d in range(N)],
             unprofitable=[float((out[d]["gain"] < 0).mean()) for d in range(N)],
             returned=[float((out[d]["ret_step"] >= 0).mean()) for d in range(N)],
             max_jump_max=float(out[0]["max_jump"].max()),
             mass_error_max=max(float(abs(out[d]["mass"] - 1.0).max()) for d in range(N)))
    res["MIXED"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
