"""Cost of the equilibrium check (thrl_equilibrium) on the headline shape, in one process:

    python profiles/equilibrium_rate.py [--reps 5] [--step-timeout 300] [--out OUT.json]
    python profiles/equilibrium_rate.py --reps 1 --out OUT.json      # under rocprofv3 --kernel-trace --stats

2^20 games, two QTable agents (21 actions, 101 rows, S = 41 states), float32 tables, both agents solved, on three kinds
of tables: fresh (Philox init), after 200 training episodes, and near-greedy (the LATE config trained 1,600 episodes,
as in deviation_rate.py).  Per kind: the kernel time from device events around the library call alone (median over
reps after one warm-up; outputs preallocated, nothing downloaded inside the timed region), the synchronised time of
GameBatch.equilibrium (which allocates and downloads the per-game outputs), the mean policy-iteration count, the
fractions nash / perfect, and one 20-episode training launch of the same batch timed in the same process: the
yardstick is "no more than one launch".  THRL_LIB selects the library, so the same script times the launch on another
build of the same ABI.  Each GPU step runs under its own time limit (faulthandler: the process dumps its stack and
exits).
"""
import argparse
import ctypes
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


def _timed(limit, fn):
    import torch
    faulthandler.dump_traceback_later(limit, exit=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    faulthandler.cancel_dump_traceback_later()
    return out, dt


def kernel_ms(gb, a):
    """Device-event time of thrl_equilibrium alone, both agents."""
    import torch
    from th_rl_amd import _lib, equilibrium as eq
    x = _lib.EquilibriumArgs()
    x.n_games, x.agents = gb.G, 3
    keep = [torch.zeros((gb.G,), dtype=torch.int32, device=gb.device) for _ in range(2)]
    keep += [torch.zeros((2, gb.G), dtype=torch.int32, device=gb.device) for _ in eq.INT_FIELDS]
    keep += [torch.zeros((2, gb.G), dtype=torch.float64, device=gb.device) for _ in eq.FLOAT_FIELDS]
    for f, t in zip(("mu", "lam") + eq.INT_FIELDS + eq.FLOAT_FIELDS, keep):
        setattr(x, f, t.data_ptr())
    x.state0 = gb.state.data_ptr()
    times = []
    for rep in range(a.reps + 1):
        faulthandler.dump_traceback_later(a.step_timeout, exit=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(gb.L.thrl_equilibrium(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(x), gb._stream()),
                   "thrl_equilibrium")
        e1.record()
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()
        if rep:
            times.append(e0.elapsed_time(e1))
    return dict(median=float(np.median(times)), min=float(np.min(times)), all=times)


def measure(gb, a):
    if a.launch_only:
        return {}
    out, t_call = _timed(a.step_timeout, lambda: gb.equilibrium())
    return dict(kernel_ms=kernel_ms(gb, a), call_ms=1e3 * t_call, iters_mean=float(out["iters"].mean()),
                iters_max=int(out["iters"].max()), capped=int((out["iters"] < 0).sum()),
                nash=float(out["nash"].mean()), perfect=float(out["perfect"].mean()),
                mu_plus_lam=float(np.mean(out["mu"].astype(np.int64) + out["lam"])))


def train(gb, episodes, a):
    """episodes in launches of 20; returns the times of the last three launches (ms)."""
    import torch
    dts = []
    for _ in range(episodes // 20):
        dts.append(_timed(a.step_timeout, lambda: gb.run(20, logs=False, sync=False))[1])
    torch.cuda.synchronize()
    return [1e3 * t for t in dts[-3:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300)
    ap.add_argument("--launch-only", action="store_true", help="time the training launches only (any build of the ABI)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib
    from th_rl_amd.batched import GameBatch
    res = dict(games=G, agents=[0, 1], n_states=41, dtype="float32", reps=a.reps, build=_lib.build_info())
    gb = GameBatch(HEADLINE, n_games=G, dtype="float32", seed=3).init_tables()
    res["fresh"] = measure(gb, a)
    res["fresh"]["train_20_episodes_ms"] = train(gb, 20, a)
    print(json.dumps({"fresh": res["fresh"]}), flush=True)
    t = train(gb, 180, a)
    res["trained_200"] = measure(gb, a)
    res["trained_200"]["train_20_episodes_ms"] = t
    print(json.dumps({"trained_200": res["trained_200"]}), flush=True)
    del gb
    torch.cuda.empty_cache()
    gb = GameBatch(LATE, n_games=G, dtype="float32", seed=3).init_tables()
    t = train(gb, 1600, a)
    res["near_greedy"] = measure(gb, a)
    res["near_greedy"]["train_20_episodes_ms"] = t
    res["near_greedy"]["eps"] = list(gb.eps)
    print(json.dumps({"near_greedy": res["near_greedy"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
