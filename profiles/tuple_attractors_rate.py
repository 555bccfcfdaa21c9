"""Rate of the attractor analysis in tuple form (thrl_tuple_attractors), float32 tables, networks with kinks inside the
price range, with uniform start weights:

  MIXED   QTable vs Reinforce, 21 x 21 actions, T = 441, 65,536 games after 20 training episodes, from the states
          training stopped at
  BIG     QTable (128 actions) vs Reinforce (32), T = 4096, 4,096 untrained games (fresh tables: the QTable's greedy
          action is 0 everywhere until it has learnt) from random start tuples

beside thrl_tuple_walk (the one path from the training tuple) on the same strategies and starts, and the extraction
(thrl_tuple_policy) of each config.

    python profiles/tuple_attractors_rate.py [--games N] [--games-big N] [--out profiles/tuple_attractors_rate.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/tuple_attractors_rate.py --repeat 1

Times are device events around the calls (outputs allocated beforehand by the runners' own code paths and their copies to
the host are included), median of `--repeat` after a warm-up, with the spread (min, max); games/s is games over the
median.  Under rocprofv3 the per-kernel times are in its kernel_stats file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
RF = dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])
CONFIGS = {"MIXED": {"agents": [dict(AG), dict(RF)], "environment": dict(ENV)},
           "BIG": {"agents": [dict(AG, actions=128), dict(RF, actions=32)], "environment": dict(ENV)}}


def timed(fn, repeat, torch, games):
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
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "games_per_s": games / (med * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--games-big", type=int, default=1 << 12)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "tuple_attractors_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, tuple_play as tp
    from th_rl_amd.mixed import MixedGameBatch
    res = {"build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    for name, config in CONFIGS.items():
        G = a.games if name == "MIXED" else a.games_big
        mb = MixedGameBatch(config, n_games=G, dtype="float32", seed=1).init_tables()
        tabs = tp.tables(config)
        rs = np.random.RandomState(0)
        n = min(G, 4096)
        for rb in mb.nn.values():           # up to 4,096 distinct networks whose greedy action moves with the price
            w = np.zeros((n, rb.P), np.float32)
            w1 = rs.uniform(-1, 1, (n, 256))
            w[:, :256], w[:, 256:512] = w1, -w1 * rs.uniform(tabs["price"].min(), tabs["price"].max(), (n, 256))
            n2 = rb.A * 256 + rb.A
            w[:, 512:512 + n2] = rs.uniform(-1, 1, (n, n2))
            rb.params.copy_(torch.from_numpy(w).to(mb.device).repeat((G + n - 1) // n, 1)[:G])
        if name == "MIXED":
            mb.run(20, per_game_logs=False)
        r = {"games": G, "tuples": int(tabs["T"])}
        r["extract"] = timed(lambda: tp.extract(mb, tabs), a.repeat, torch, G)
        pol = tp.extract(mb, tabs)
        if name == "MIXED":
            start = tp.start_tuples(mb, tabs)
        else:
            start = torch.from_numpy(rs.randint(0, int(tabs["T"]), G).astype(np.int32)).to(mb.device)
        out = {}
        r["attractors"] = timed(lambda: out.update(a=mb.greedy_attractors(start=start, tuple_policy=pol)), a.repeat, torch, G)
        r["walk"] = timed(lambda: out.update(w=tp.run(mb, start=start, tuple_policy=pol, tabs=tabs)), a.repeat, torch, G)
        at, wk = out["a"], out["w"]
        has = at["start"] >= 0
        assert np.array_equal(wk["mu"][has], at["mu_x0"][has])
        r.update(no_start=int((~has).sum()), single=float((at["n_attr"] == 1).mean()), n_attr_mean=float(at["n_attr"].mean()),
                 n_attr_max=int(at["n_attr"].max()), mu_max_mean=float(at["mu_max"].mean()), mu_max_max=int(at["mu_max"].max()),
                 lam_max=int(at["lam"].max()), train_is_largest=float((at["slot_x0"][has] == 0).mean()) if has.any() else None,
                 mass_other_max=float(at["start_mass_other"].max()))
        res[name] = r
        del mb, pol
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
