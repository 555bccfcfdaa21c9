"""Cost of the smoothed learning curves (thrl_ewm_rows, training.group_stats.smooth) on the headline shape:

    python profiles/ewm_rate.py [--reps 5] [--step-timeout 300] [--out OUT.json]
    python profiles/ewm_rate.py --kernel-only        # the kernel alone; also the run to put under rocprofv3 --kernel-trace --stats

--kernel-only: k_ewm_rows at N = 2, G = 2^20, E = game_log_chunk() episodes (the launch train_one makes), in place on
rows that already hold values, timed with device events around each call after a warm-up; the bytes are one read and
one write of the rows plus one read and one write of the state, computed from the shapes.

Throughput: 2^20 games, two QTable agents, float32, an 8-value gamma sweep, launches of game_log_chunk() episodes with
training.group_stats as train_one makes them, each chunk's statistics fetched and finalised on the host.  The runs
with smoothing (two reductions and the smoothing kernel per chunk, both sets finalised) and without alternate chunk by
chunk from the same start; env-steps/s per run and the check that tables, counters, state, epsilon, the mean logs and
the raw statistics are bit-identical between them are recorded.  Each step is guarded by its own time limit
(faulthandler: the process dumps its stack and exits).
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
G = 1 << 20
N = 2
HALFLIFE = 1000.0
GAMMAS = [0.35, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99]


def _guard(limit):
    faulthandler.dump_traceback_later(limit, exit=True)


def kernel_only(a):
    import torch
    from th_rl_amd import _lib, trainer
    from th_rl_amd.group_stats import Smoother
    L = _lib.load()
    E = trainer.game_log_chunk(N, G, 1)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rew = torch.rand((E, N, G), dtype=torch.float64, device="cuda", generator=gen) * 25.0
    act = torch.rand((E, N, G), dtype=torch.float64, device="cuda", generator=gen)
    sm = Smoother(N, G, HALFLIFE, "cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    us = []
    for rep in range(a.reps + 3):                   # the first three: warm-up (code object, first touch), not recorded
        _guard(a.step_timeout)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        sm.apply(L, rew, act, E, stream)            # in place: smoothing smoothed rows again costs the same
        t1.record()
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()
        if rep >= 3:
            us.append(1e3 * t0.elapsed_time(t1))
    moved = 2 * (2 * E * N * G * 8) + 2 * (2 * N * G * 8)     # rows read + written, state read + written
    med = float(np.median(us))
    res = dict(games=G, agents=N, episodes_per_launch=E, halflife=HALFLIFE, reps=a.reps, bytes_moved=moved,
               call_us=dict(median=med, min=float(np.min(us)), max=float(np.max(us)), all=us),
               gb_per_s_at_median=moved / med / 1e3, timer="device events around thrl_ewm_rows, one kernel per call")
    print(json.dumps({k: v for k, v in res.items() if k != "call_us"} | {"call_us_median": med}), flush=True)
    return res


def rate(a):
    import torch
    from th_rl_amd import trainer
    from th_rl_amd.batched import GameBatch
    from th_rl_amd.group_stats import GroupSpec, Smoother, finalize
    config = HEADLINE
    T = config["environment"]["max_steps"]
    sw = {"gamma": np.asarray([GAMMAS[g % len(GAMMAS)] for g in range(G)])}
    on = GameBatch(config, n_games=G, dtype="float32", seed=3, sweep=sw).init_tables()
    off = GameBatch(config, n_games=G, dtype="float32", seed=3, sweep=sw)
    off.set_tables(on.tables_numpy(), on.states_numpy())
    spec = GroupSpec.from_config(config, G, {"smooth": HALFLIFE}, sweep=sw)
    desc = spec.describe()
    sm = Smoother(N, G, HALFLIFE, on.device)
    E = trainer.game_log_chunk(N, G, 1)
    rates = {"on": [], "off": []}
    ok = True
    for rep in range(a.reps + 1):                  # rep 0: warm-up, not recorded
        for tag, b in (("off", off), ("on", on)) if rep % 2 else (("on", on), ("off", off)):
            _guard(a.step_timeout)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = b.run(E, group_stats=spec, smooth=sm if tag == "on" else None)
            finalize(out["group_stats"], desc)
            if tag == "on":
                finalize(out["group_stats_smooth"], desc)
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
        ok &= all(np.array_equal(o_on["group_stats"][k], o_off["group_stats"][k]) for k in ("hist", "sums", "minmax"))
    ok &= bool(torch.equal(on.q, off.q) and torch.equal(on.counter, off.counter) and torch.equal(on.state, off.state))
    ok &= on.eps == off.eps and all(torch.equal(on.sweep[k], off.sweep[k]) for k in on.sweep)
    r = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=v) for k, v in rates.items()}
    r["on_over_off"] = r["on"]["median"] / r["off"]["median"]
    r["epochs_per_s"] = {k: r[k]["median"] / (G * T) for k in ("on", "off")}
    r["outputs_match"] = ok
    r.update(games=G, groups=spec.n_groups, episodes_per_launch=E, max_steps=T, reps=a.reps, bins=spec.bins,
             halflife=HALFLIFE, rows_smoothed=sm.rows)
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
        sys.exit("outputs differ between the runs with and without smoothing")


if __name__ == "__main__":
    main()
