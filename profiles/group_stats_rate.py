"""Cost of the per-group statistics (thrl_group_stats) on the headline shape, in one process:

    python profiles/group_stats_rate.py [--reps 5] [--step-timeout 300] [--out OUT.json]
    python profiles/group_stats_rate.py --kernel-only        # under rocprofv3 --kernel-trace --stats

Throughput: 2^20 games, two QTable agents, float32, an 8-value gamma sweep (8 groups of 131,072 games), launches of
game_log_chunk() episodes as train_one makes them with training.group_stats, each chunk's statistics fetched and
finalised on the host (mean / std / quantiles) as train_one does.  The runs with and without statistics alternate
chunk by chunk from the same start; env-steps/s per run and the check that tables, counters, state, epsilon and the
mean logs are bit-identical between them are recorded.

--kernel-only: 16 episodes with statistics on a fresh table, then the same on a near-greedy state (trained until
epsilon = eps_end = 0.001: the late-training case where a group's values fall into a handful of bins), for the
kernel trace.  Each step is guarded by its own time limit (faulthandler: the process dumps its stack and exits).
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
HEADLINE = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
LATE = {"agents": [dict(AG, eps_step=0.995), dict(AG, eps_step=0.995)], "environment": dict(ENV)}
G = 1 << 20
GAMMAS = [0.35, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99]


def _sweep():
    return {"gamma": np.asarray([GAMMAS[g % len(GAMMAS)] for g in range(G)])}


def _guard(limit):
    faulthandler.dump_traceback_later(limit, exit=True)


def _spec(config, sweep):
    from th_rl_amd.group_stats import GroupSpec
    return GroupSpec.from_config(config, G, True, sweep=sweep)


def kernel_only(a):
    import torch
    from th_rl_amd.batched import GameBatch
    res = {}
    for name, config, train in (("fresh", HEADLINE, 0), ("near_greedy", LATE, 1600)):
        sw = _sweep()
        gb = GameBatch(config, n_games=G, dtype="float32", seed=3, sweep=sw).init_tables()
        spec = _spec(config, sw)
        done = 0
        while done < train:
            _guard(a.step_timeout)
            gb.run(20, logs=False, sync=False)
            torch.cuda.synchronize()
            done += 20
        _guard(a.step_timeout)
        out = gb.run(16, group_stats=spec)
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()
        h = out["group_stats"]["hist"]
        res[name] = dict(eps=[float(x) for x in gb.sweep["eps"][:, 0].cpu()] if "eps" in gb.sweep else gb.eps,
                         nonzero_bins_per_cell=float((h > 0).sum(axis=-1).mean()))
        print(json.dumps({name: res[name]}), flush=True)
        del gb
        torch.cuda.empty_cache()
    return res


def rate(a):
    import torch
    from th_rl_amd import trainer
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import finalize
    config = HEADLINE
    T = config["environment"]["max_steps"]
    sw = _sweep()
    on = GameBatch(config, n_games=G, dtype="float32", seed=3, sweep=sw).init_tables()
    off = GameBatch(config, n_games=G, dtype="float32", seed=3, sweep=sw)
    off.set_tables(on.tables_numpy(), on.states_numpy())
    spec = _spec(config, sw)
    desc = spec.describe()
    E = trainer.game_log_chunk(2, G, 1)
    rates = {"on": [], "off": []}
    ok = True
    for rep in range(a.reps + 1):                  # rep 0: warm-up (code objects, first touch), not recorded
        for tag, b in (("off", off), ("on", on)) if rep % 2 else (("on", on), ("off", off)):
            _guard(a.step_timeout)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = b.run(E, group_stats=spec if tag == "on" else None)
            if tag == "on":
                finalize(out["group_stats"], desc)
            dt = time.perf_counter() - t0
            faulthandler.cancel_dump_traceback_later()
            assert out["kernel"] == "wave", out["kernel"]
            if tag == "on":
                o_on = out
            else:
                o_off = out
            if rep:
                rates[tag].append(G * E * T / dt)
        ok &= bool(np.array_equal(o_on["reward_log"], o_off["reward_log"])
                   and np.array_equal(o_on["action_log"], o_off["action_log"]))
    ok &= bool(torch.equal(on.q, off.q) and torch.equal(on.counter, off.counter) and torch.equal(on.state, off.state))
    ok &= on.eps == off.eps and all(torch.equal(on.sweep[k], off.sweep[k]) for k in on.sweep)
    r = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=v) for k, v in rates.items()}
    r["on_over_off"] = r["on"]["median"] / r["off"]["median"]
    r["outputs_match"] = ok
    r.update(games=G, groups=spec.n_groups, episodes_per_launch=E, max_steps=T, reps=a.reps, bins=spec.bins)
    print(json.dumps({k: v for k, v in r.items() if k not in ("on", "off")} | {
        "on": r["on"]["median"], "off": r["off"]["median"]}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    res = kernel_only(a) if a.kernel_only else rate(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.kernel_only and not res["outputs_match"]:
        sys.exit("outputs differ between the runs with and without group statistics")


if __name__ == "__main__":
    main()
