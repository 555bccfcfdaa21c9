"""Rate of the best responses to sampled play under demand noise (thrl_sampled_response_noise), float32 tables, networks
with kinks inside the price range:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = D = 441, --games games after 20 training episodes, epsilon where
          training stopped, noise_prob 0.05 at the default resolution (Jn = 1,121 nodes, S = 1,562 states), both agents
          solved at --gamma (default: each agent's own, 0.95 and 0.995), eval_tol 1e-12, at most 8,192 sweeps per
          evaluation; the rows, the strategies and the long-run distribution pi are computed once, outside the timed call

It records games/s, (agent, game) pairs/s and sweeps/s, the share of pairs capped and the sweep and round counts, and with
--free the noise-free call (thrl_sampled_response) on the same batch in the same process, the two alternating, beside the
ratio the operation counts predict: a sweep of a deterministic strategy is S T / A_i + T W multiply-adds against
D T / A_i, a sweep of the mixed policy or an improvement step S T + T W against D T (include/thrl_response_noise.h); each
call's counts of the two kinds of sweep are taken from its own outputs (sweeps, iters), so the prediction is per batch.

    python profiles/sampled_response_noise_rate.py [--games N] [--gamma X] [--repeat R] [--free] [--warm-games N]
                                                   [--chunks K] [--out FILE]

--warm-games warms the kernels up on a few games in place of the whole batch, --chunks times the noisy call as K calls of
games / K games and adds the times up: at 65,536 games one call runs a quarter of an hour.  The committed JSON is put
together from a run at 65,536 games (--warm-games 512 --chunks 8 --repeat 1), one at 4,096 with --free and two of
profiles/sampled_response_rate.py on the parent's build and on this one.

Times are device events around the calls (outputs allocated by the runner's own code path and their copies to the host
are included), median of `--repeat` after a warm-up, with the spread (min, max); games/s is games over the median."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sampled_play_rate import kinked  # noqa: E402
from tuple_attractors_rate import CONFIGS  # noqa: E402

NOISE_PROB = 0.05


def madds(x, states, T, W, acts):
    """The multiply-adds of a call by the header's counts: per (agent, game) the improvement steps are iters + 1, the
    mixed sweeps cannot be told from the sweeps of the rounds in the outputs, so they are estimated as sweeps / (iters +
    2) (one evaluation of iters + 2: the mixed policy's and one per round); unsolved pairs are left out."""
    ok = x["iters"] >= 0
    total = 0.0
    for i, A in enumerate(acts):
        sw, it = x["sweeps"][i][ok[i]].astype(np.float64), x["iters"][i][ok[i]].astype(np.float64)
        mixed = sw / (it + 2.0)
        full, one = states * T + T * W, states * T / A + T * W
        total += float((mixed * full + (sw - mixed) * one + (it + 1.0) * full).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=None)
    ap.add_argument("--warm-games", type=int, default=0, help="warm up on this many games instead of the whole batch")
    ap.add_argument("--chunks", type=int, default=1, help="time the noisy call over the batch in this many equal slices of "
                    "games, one call each, and add the times up (a call of a quarter of an hour says nothing while it runs)")
    ap.add_argument("--free", action="store_true", help="also time thrl_sampled_response on the same batch, alternating")
    ap.add_argument("--out", default=os.path.join(HERE, "sampled_response_noise_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, sampled_play as sp, sampled_response as sr, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    G = a.games
    config = CONFIGS["MIXED"]
    mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
    tabs = sp.noise_tables(config)
    kinked(mb, tabs, torch, G)
    mb.run(20, per_game_logs=False)
    T, D, Jn, W = int(tabs["n_tuples"]), int(tabs["n_prices"]), int(tabs["n_nodes"]), int(tabs["band_w"])
    acts = [int(x) for x in tabs["n_actions"]]
    ws = sr.working_set_noise(config, tabs=tabs, n_nodes=Jn)
    r = {"games": G, "tuples": T, "prices": D, "nodes": Jn, "band_w": W, "lds_bytes": ws["bytes"], "noise_prob": NOISE_PROB,
         "eval_tol": 1e-12, "max_sweeps": 8192, "epsilon": [float(x) for x in list(mb.eps)[:mb.N]]}
    probs, dpol = sp.price_probs(mb, tabs["dprice"]), ts.price_policy(mb, tabs["dprice"])
    nprobs, npol = sp.price_probs(mb, tabs["xn"]), ts.price_policy(mb, tabs["xn"])
    pi_n = mb.sampled_play(pi=True, probs=probs, dpolicy=dpol, tabs=tabs, noise_prob=NOISE_PROB, nprobs=nprobs, npolicy=npol)["pi"]
    out = {}
    cut = lambda d, n: {i: x[:n].contiguous() for i, x in d.items()}
    keys = ("iters", "sweeps", "gamma", "br_prob_w")

    def noise(n=G, lo=0):
        sl = slice(lo, lo + n)
        cut = lambda d: {i: x[sl].contiguous() for i, x in d.items()}
        return mb.sampled_response_noise(gamma=a.gamma, pi=pi_n[sl], probs=cut(probs), dpolicy=dpol[sl].contiguous(),
                                         nprobs=cut(nprobs), npolicy=npol[sl].contiguous(), ntabs=tabs, noise_prob=NOISE_PROB,
                                         n_games=n)
    calls = {"noise": lambda n=G: out.update(noise=noise(n))}
    if a.free:
        pi_f = mb.sampled_play(pi=True, probs=probs, dpolicy=dpol, tabs=tabs)["pi"]
        calls["free"] = lambda n=G: out.update(free=mb.sampled_response(
            gamma=a.gamma, pi=pi_f[:n], probs=cut(probs, n), dpolicy=dpol[:n].contiguous(), tabs=tabs, n_games=n))
    ms = {k: [] for k in calls}
    r["warm_up_games"], r["chunks"] = a.warm_games or G, a.chunks
    for rep in range(a.repeat + 1):                      # the first round warms up (the same kernels and shape, on
        for k, fn in calls.items():                      # --warm-games games where given); the calls alternate
            if k == "noise" and a.chunks > 1 and not (rep == 0 and a.warm_games):
                n, parts, total = G // a.chunks, [], 0.0
                for c in range(a.chunks):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    parts.append(noise(n, c * n))
                    e1.record()
                    torch.cuda.synchronize()
                    total += e0.elapsed_time(e1)
                    print(json.dumps({"noise": e0.elapsed_time(e1), "round": rep, "chunk": c, "games": n}), flush=True)
                    r.setdefault("chunk_ms", []).append(e0.elapsed_time(e1))
                out["noise"] = {f: np.concatenate([x[f] for x in parts], axis=1) for f in keys}
                if rep:
                    ms[k].append(total)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(a.warm_games) if (rep == 0 and a.warm_games) else fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms[k].append(e0.elapsed_time(e1))
            print(json.dumps({k: e0.elapsed_time(e1), "round": rep}), flush=True)
    for k, v in ms.items():
        med = statistics.median(v)
        x = out[k]
        ok = x["iters"] >= 0
        sec = med * 1e-3
        r[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "games_per_s": G / sec,
                "pairs_per_s": float(x["iters"].size) / sec, "sweeps_per_s": float(x["sweeps"].sum()) / sec,
                "capped": float((~ok).mean()), "gamma": [float(g) for g in x["gamma"][:, 0]],
                "sweeps_mean": [float(v2) for v2 in x["sweeps"].mean(axis=1)], "sweeps_max": int(x["sweeps"].max()),
                "iters_mean": [float(x["iters"][i][ok[i]].mean()) if ok[i].any() else None for i in range(mb.N)],
                "iters_max": int(x["iters"].max()), "br_prob_w_mean": [float(np.nanmean(v2)) for v2 in x["br_prob_w"]],
                "madds": madds(x, D + Jn if k == "noise" else D, T, W if k == "noise" else 0, acts)}
    if a.free:
        r["measured_ratio"] = r["noise"]["median_ms"] / r["free"]["median_ms"]
        r["expected_ratio_from_operation_counts"] = r["noise"]["madds"] / r["free"]["madds"]
        A = acts[1]
        r["expected_ratio_per_sweep"] = {"deterministic": ((D + Jn) * T / A + T * W) / (D * T / A),
                                         "mixed": ((D + Jn) * T + T * W) / float(D * T)}
    res["MIXED"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
