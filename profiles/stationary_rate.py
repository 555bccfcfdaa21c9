"""Rates of the stationary analysis (thrl_stationary) at 2^20 headline games, float32, fresh tables, with its
yardsticks in the same process:

  extract      the extraction pass alone (thrl_crossplay with one throw-away match)
  given_p05    the call with THRL_STAT_POLICY_GIVEN at noise_prob 0.05 (101 cells, tol 1e-12, at most 8192 steps)
  given_p01    the same at noise_prob 0.01
  iters_*      the distribution of the steps taken
  sampled      the sampled route: thrl_play_greedy for 100 iterations (episodes of 100 steps from a reset) in the
               environment with noise_prob 0.05, its time, and the mean absolute gap between its per-game mean reward
               and stat_reward -- evidence, no threshold: the sample carries the transient from every reset and a
               sampling error whose autocorrelation nobody has measured
  launch       one 20-episode training launch of the same batch, for scale

    python profiles/stationary_rate.py [--games N] [--out profiles/stationary_rate.json]

Times are device events around the calls, median of `--repeat` after a warm-up, with the spread (min, max)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AG = dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001,
          epsilon=0.5, eps_step=0.9995, action_range=[0.2, 0.4])
ENV = dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}
NOISY = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV, noise_prob=0.05)}


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


def iters_stats(it):
    it = np.asarray(it)
    q = np.quantile(it, [0.25, 0.5, 0.75])
    return {"min": int(it.min()), "q25": float(q[0]), "q50": float(q[1]), "q75": float(q[2]), "max": int(it.max()),
            "mean": float(it.mean()), "not_converged": int((it >= 8192).sum()), "not_solved": int((it < 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, attractors as at, crossplay as xp, deviation as dv, stationary as sn
    from th_rl_amd.batched import GameBatch
    G = a.games
    # fresh tables, initialised in slices of 2^15 games (one thrl_qtable_init call over 2^32 elements or
    # more leaves most tables unwritten)
    gb = GameBatch(CFG, n_games=G, dtype="float32", seed=1)
    for lo in range(0, G, 1 << 15):
        part = GameBatch(CFG, n_games=min(1 << 15, G - lo), dtype="float32", seed=1, game_offset=lo, counters=False).init_tables()
        gb.q[lo:lo + part.G].copy_(part.q)
        gb.state[lo:lo + part.G].copy_(part.state)
        del part
    gb.initialized = True
    dev = gb.device
    N, P = gb.N, at.policy_entries(gb)
    tabs = sn.tables(CFG)
    J, W = tabs["n_cells"], tabs["band_w"]
    keep = {f: torch.from_numpy(np.ascontiguousarray(tabs[f])).to(dev)
            for f in ("cell_rows", "cell_w", "det_cell", "band_lo", "band", "noise_reward", "noise_price")}
    pol = torch.empty((G, P), dtype=torch.int16, device=dev)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    out = {"iters": torch.zeros((G,), dtype=torch.int32, device=dev), "change": f64(G), "mass": f64(G),
           "stat_reward": f64(N, G), "stat_action": f64(N, G), "stat_price": f64(G)}
    x = _lib.StationaryArgs()
    x.n_games, x.n_cells, x.band_w, x.max_iters, x.tol, x.flags = G, J, W, 8192, 1e-12, _lib.STAT_POLICY_GIVEN
    x.policy = pol.data_ptr()
    for f, t in list(keep.items()) + list(out.items()):
        setattr(x, f, t.data_ptr())

    def stationary(p):
        x.noise_prob = p
        _lib.check(gb.L.thrl_stationary(ctypes.byref(gb.cfg), None, ctypes.byref(x), gb._stream()), "thrl_stationary")

    # the extraction pass: cross-play with one throw-away match
    seat = torch.from_numpy(xp.identity(N, G)).to(dev)
    c = _lib.CrossplayArgs()
    c.n_games, c.n_matches, c.horizon, c.policy, c.seat = G, 1, dv.default_horizon([21, 21]), pol.data_ptr(), seat.data_ptr()
    cout = {"mu": torch.zeros((G,), dtype=torch.int32, device=dev), "lam": torch.zeros((G,), dtype=torch.int32, device=dev),
            "cycle_reward": f64(N, G), "cycle_action": f64(N, G)}
    for f, t in cout.items():
        setattr(c, f, t.data_ptr())
    c.state0 = gb.state.data_ptr()

    def extract():
        _lib.check(gb.L.thrl_crossplay(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(c), gb._stream()), "thrl_crossplay")

    res = {"games": G, "n_cells": J, "band_w": W, "band_bytes": int(tabs["band"].nbytes), "tol": 1e-12, "max_iters": 8192,
           "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["extract"] = timed(extract, a.repeat, torch)
    res["given_p05"] = timed(lambda: stationary(0.05), a.repeat, torch)
    res["iters_p05"] = iters_stats(out["iters"].cpu().numpy())
    mass = out["mass"].cpu().numpy()
    res["mass_max_err_p05"] = float(np.abs(mass - 1.0).max())
    stat = out["stat_reward"].cpu().numpy().copy()
    nash, cartel = dv.optimal(CFG)
    res["delta_noise_mean_p05"] = float(dv.profit_gain(stat, nash, cartel).mean())
    res["given_p01"] = timed(lambda: stationary(0.01), a.repeat, torch)
    res["iters_p01"] = iters_stats(out["iters"].cpu().numpy())

    # the sampled route in the noisy environment, on the same tables
    gn = GameBatch(NOISY, n_games=G, dtype="float32", seed=1)
    iters = 100
    mr, ma = f64(iters, N, G), f64(iters, N, G)

    def sampled():
        _lib.check(gn.L.thrl_play_greedy(ctypes.byref(gn.cfg), gb.q.data_ptr(), None, iters, gn.seed, gn.game_offset,
                                         mr.data_ptr(), ma.data_ptr(), gb._stream()), "thrl_play_greedy")

    res["sampled"] = dict(timed(sampled, 3, torch), iterations=iters, steps_per_iteration=int(NOISY["environment"]["max_steps"]))
    mean = mr.mean(dim=0).cpu().numpy()
    res["sampled"]["mean_abs_gap_to_stat_reward"] = float(np.abs(mean - stat).mean())
    res["sampled"]["mean_gap_to_stat_reward"] = float((mean - stat).mean())
    res["sampled"]["stat_reward_mean"] = float(stat.mean())
    del mr, ma
    res["training_launch_20"] = timed(lambda: gb.run(20, logs=False, sync=False), 3, torch)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
