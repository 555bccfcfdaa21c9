"""Cost of convergence tracking (thrl_policy_track) on the headline shape, in one process:

    python profiles/convergence_rate.py [--reps 10] [--loops 3] [--step-timeout 300] [--out OUT.json]
    python profiles/convergence_rate.py --reps 3 --loops 1 --out OUT.json     # under rocprofv3 --kernel-trace --stats

2^20 games, two QTable agents (21 actions, 101 rows: P = 202 policy entries, stride 4,242), window 1,000, on two kinds
of tables: fresh (Philox init) and near-greedy (the LATE config of group_stats_rate.py trained 1,600 episodes in
float32; the float64 batch gets the same tables converted).  Per dtype and kind: the kernel time of one check (HIP
events around the launch, median over reps after one warm-up) and its effective read rate (G * stride * sizeof(q)
bytes per check) against the 6.3 TB/s achievable HBM rate.  Then the train-loop rate: `loops` rounds of 10 launches
of 20 episodes each, alternated, on the fresh float32 headline batch: untracked; tracked (a check after every launch,
no count copied: the trainer without `stop` between progress lines); tracked_counted (the count copied to the host
after every check, which waits for the device: the trainer with `stop`).  Each GPU step runs under its own time limit (faulthandler:
the process dumps its stack and exits).
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
HBM = 6.3e12
WINDOW = 1000


def _guard(limit):
    faulthandler.dump_traceback_later(limit, exit=True)


def _timed(limit, fn):
    import torch
    _guard(limit)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    faulthandler.cancel_dump_traceback_later()
    return out, dt


def kernel_ms(tr, a):
    """Median kernel time of one check (HIP events around the launch only)."""
    import torch
    times = []
    for k in range(a.reps + 1):
        _guard(a.step_timeout)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tr.batch.episode += 20
        e0.record()
        tr._launch(0)
        e1.record()
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()
        if k:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def measure(gb, a):
    tr = gb.track_convergence(window=WINDOW, every=20)
    med, mn = kernel_ms(tr, a)
    nbytes = G * gb.stride * gb.q.element_size()
    r = dict(kernel_ms=dict(median=med, min=mn), bytes_read=nbytes, gb_per_s=nbytes / (med * 1e-3) / 1e9,
             fraction_of_hbm=nbytes / (med * 1e-3) / HBM, changes_mean=float(tr.changes.double().mean()))
    del tr
    return r


def train(gb, episodes, a):
    for _ in range(episodes // 20):
        _timed(a.step_timeout, lambda: gb.run(20, logs=False, sync=False))


def loop_rate(gb, a):
    """Episodes per second of 10 launches of 20 episodes, untracked and tracked, alternated `loops` times."""
    import torch
    tr = gb.track_convergence(window=WINDOW, every=20)
    rates = {"untracked": [], "tracked": [], "tracked_counted": []}
    for _ in range(a.loops):
        for kind in ("untracked", "tracked", "tracked_counted"):
            _guard(a.step_timeout)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                gb.run(20, logs=False, sync=False)
                if kind != "untracked":
                    tr.check(count=kind == "tracked_counted")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            faulthandler.cancel_dump_traceback_later()
            rates[kind].append(200 / dt)
    u, t, c = (float(np.median(rates[k])) for k in ("untracked", "tracked", "tracked_counted"))
    return dict(episodes_per_s=rates, untracked_median=u, tracked_median=t, tracked_counted_median=c, ratio=t / u,
                ratio_counted=c / u, launch_20_ms_untracked=20e3 / u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd.batched import GameBatch
    res = dict(games=G, stride=None, policy_entries=202, window=WINDOW, reps=a.reps, hbm_bytes_per_s=HBM)
    gb = GameBatch(HEADLINE, n_games=G, dtype="float32", seed=3).init_tables()
    res["stride"] = gb.stride
    res["loop"] = loop_rate(gb, a)
    print(json.dumps({"loop": res["loop"]}), flush=True)
    del gb
    torch.cuda.empty_cache()
    late = GameBatch(LATE, n_games=G, dtype="float32", seed=3).init_tables()
    train(late, 1600, a)
    q_late, s_late = late.q, late.state
    for dtype in ("float32", "float64"):
        gb = GameBatch(HEADLINE, n_games=G, dtype=dtype, seed=3, counters=False).init_tables()
        res[dtype + "_fresh"] = measure(gb, a)
        print(json.dumps({dtype + "_fresh": res[dtype + "_fresh"]}), flush=True)
        gb.q.copy_(q_late)
        gb.state.copy_(s_late)
        res[dtype + "_near_greedy"] = measure(gb, a)
        print(json.dumps({dtype + "_near_greedy": res[dtype + "_near_greedy"]}), flush=True)
        del gb
        torch.cuda.empty_cache()
    res["near_greedy_eps"] = list(late.eps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
