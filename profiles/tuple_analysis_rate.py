"""Rates of the deviation test and the equilibrium check in tuple form (thrl_tuple_deviation, thrl_tuple_equilibrium) at
65,536 games, float32 tables, networks with kinks inside the price range, after 20 training episodes, both agents
solved, from the states training stopped at:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = 441
  NN2     Reinforce (32 actions) vs ActorCritic (21), T = 672

beside the extraction (thrl_tuple_policy) of each config and, as the yardstick, thrl_equilibrium and thrl_deviation on
an all-QTable 21 x 21 batch of the same size after 20 episodes (S = 41 states).

    python profiles/tuple_analysis_rate.py [--games N] [--out profiles/tuple_analysis_rate.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/tuple_analysis_rate.py --repeat 1

Times are device events around the calls (outputs allocated beforehand by the runners' own code paths are included),
median of `--repeat` after a warm-up, with the spread (min, max); under rocprofv3 the per-kernel times are in its
kernel_stats file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
RF = dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])
CONFIGS = {"MIXED": {"agents": [dict(AG), dict(RF)], "environment": dict(ENV)},
           "NN2": {"agents": [dict(RF, actions=32), dict(RF, name="ActorCritic", actions=21)], "environment": dict(ENV)}}
TWO = {"agents": [dict(AG), dict(AG, alpha=0.3, gamma=0.9)], "environment": dict(ENV)}


def timed(fn, repeat, torch):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, tuple_play as tp
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.mixed import MixedGameBatch
    G = a.games
    res = {"games": G, "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    for name, config in CONFIGS.items():
        mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
        tabs = tp.tables(config)
        rs = np.random.RandomState(0)
        n = min(G, 4096)
        for rb in mb.nn.values():           # 4,096 distinct networks whose greedy action moves with the price
            w = np.zeros((n, rb.P), np.float32)
            w1 = rs.uniform(-1, 1, (n, 256))
            w[:, :256], w[:, 256:512] = w1, -w1 * rs.uniform(tabs["price"].min(), tabs["price"].max(), (n, 256))
            n2 = rb.A * 256 + rb.A
            w[:, 512:512 + n2] = rs.uniform(-1, 1, (n, n2))
            rb.params.copy_(torch.from_numpy(w).to(mb.device).repeat((G + n - 1) // n, 1)[:G])
        mb.run(20, per_game_logs=False)
        r = {"tuples": int(tabs["T"])}
        r["extract"] = timed(lambda: tp.extract(mb, tabs), a.repeat, torch)
        pol = tp.extract(mb, tabs)
        start = tp.start_tuples(mb, tabs)
        out = {}
        r["deviation"] = timed(lambda: out.update(d=mb.greedy_deviation(deviator=1, start=start, tuple_policy=pol)), a.repeat, torch)
        r["equilibrium"] = timed(lambda: out.update(e=mb.greedy_equilibrium(start=start, tuple_policy=pol)), a.repeat, torch)
        e, d = out["e"], out["d"]
        r.update(no_start=int((e["mu"] < 0).sum()), mean_mu_plus_lam=float((e["mu"] + e["lam"]).mean()),
                 iters_mean=float(e["iters"].mean()), iters_max=int(e["iters"].max()),
                 iters_ge_1=float((e["iters"] >= 1).mean()), nash=float(e["nash"].mean()), perfect=float(e["perfect"].mean()),
                 returned=float((d["ret_step"] >= 0).mean()), unprofitable=float((d["gain"] < 0).mean()))
        res[name] = r
        del mb, pol
        torch.cuda.empty_cache()
    gb = GameBatch(TWO, n_games=G, dtype="float32", seed=1).init_tables()
    gb.run(20, logs=False)
    out = {}
    r = {"equilibrium": timed(lambda: out.update(e=gb.equilibrium()), a.repeat, torch),
         "deviation": timed(lambda: gb.deviation(deviator=1), a.repeat, torch)}
    r.update(states=int(out["e"]["n_states"]), iters_mean=float(out["e"]["iters"].mean()))
    res["QTABLE_rows"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
