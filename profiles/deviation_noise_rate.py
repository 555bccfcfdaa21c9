"""Rate of the deviation test under demand noise (thrl_deviation_noise) on 65,536 trained headline games (J = 101),
float32, noise_prob 0.05, deviator 0, best response, K = 32, L = 1, with its yardstick on the same batch in the same
process:

  stationary     thrl_stationary with THRL_STAT_POLICY_GIVEN (pi stored: the weights of the test), tol 1e-12
  noise          thrl_deviation_noise with THRL_STAT_POLICY_GIVEN, weights = that pi, no rows
  noise_rows     the same with reward_rows / action_rows / dist_rows of all K periods

    python profiles/deviation_noise_rate.py [--games N] [--episodes E] [--out profiles/deviation_noise_rate.json]

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
ENV = dict(name="NoisyPriceState", noise_prob=0.05, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(AG), dict(AG)], "environment": dict(ENV)}


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
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--dev-len", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, crossplay as xp, stationary as sn
    from th_rl_amd.batched import GameBatch
    G, K = a.games, a.steps
    gb = GameBatch(CFG, n_games=G, dtype="float32", seed=1).init_tables()
    gb.run(a.episodes, logs=False)
    dev = gb.device
    N = gb.N
    tabs = sn.tables(CFG)
    J, W = tabs["n_cells"], tabs["band_w"]
    keep = {f: torch.from_numpy(np.ascontiguousarray(tabs[f])).to(dev)
            for f in ("cell_rows", "cell_w", "det_cell", "band_lo", "band", "noise_reward", "noise_price")}
    pol = xp.extract(gb)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)

    # thrl_stationary from the policy, pi stored
    sout = {"iters": i32(G), "change": f64(G), "mass": f64(G), "stat_reward": f64(N, G), "stat_action": f64(N, G),
            "stat_price": f64(G), "pi": f64(G, J)}
    x = _lib.StationaryArgs()
    x.n_games, x.n_cells, x.band_w, x.max_iters, x.tol, x.flags = G, J, W, 8192, 1e-12, _lib.STAT_POLICY_GIVEN
    x.noise_prob, x.policy = 0.05, pol.data_ptr()
    for f, t in list(keep.items()) + list(sout.items()):
        setattr(x, f, t.data_ptr())

    def stationary():
        _lib.check(gb.L.thrl_stationary(ctypes.byref(gb.cfg), None, ctypes.byref(x), gb._stream()), "thrl_stationary")

    # thrl_deviation_noise from the policy, started from pi
    n = _lib.DeviationNoiseArgs()
    n.n_games, n.flags, n.n_cells, n.band_w = G, _lib.STAT_POLICY_GIVEN, J, W
    n.deviator, n.dev_len, n.n_steps, n.dev_action = 0, a.dev_len, K, -1
    n.noise_prob, n.ret_tol, n.policy, n.weights = 0.05, 1e-6, pol.data_ptr(), sout["pi"].data_ptr()
    nout = {f: f64(N, G) for f in ("base_reward", "base_action")}
    nout.update({f: f64(G) for f in ("dev_share", "gain", "gain_dev", "low", "dist", "mass")})
    nout.update({f: i32(G) for f in ("low_step", "ret_step")})
    for f in ("cell_rows", "det_cell", "band_lo", "band", "noise_reward"):
        setattr(n, f, keep[f].data_ptr())
    for f, t in nout.items():
        setattr(n, f, t.data_ptr())
    rows = {"reward_rows": f64(K, N, G), "action_rows": f64(K, N, G), "dist_rows": f64(K, G)}

    def noise(with_rows):
        n.row_begin, n.row_count = 0, K if with_rows else 0
        for f, t in rows.items():
            setattr(n, f, t.data_ptr() if with_rows else None)
        _lib.check(gb.L.thrl_deviation_noise(ctypes.byref(gb.cfg), None, ctypes.byref(n), gb._stream()),
                   "thrl_deviation_noise")

    res = {"games": G, "episodes": a.episodes, "n_cells": J, "band_w": W, "noise_prob": 0.05, "deviator": 0,
           "steps": K, "dev_len": a.dev_len, "action": "best_response",
           "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["stationary"] = timed(stationary, a.repeat, torch)
    it = sout["iters"].cpu().numpy()
    res["stationary_iters"] = {"min": int(it.min()), "q50": float(np.median(it)), "max": int(it.max()), "mean": float(it.mean())}
    res["noise"] = timed(lambda: noise(False), a.repeat, torch)
    res["noise_rows"] = timed(lambda: noise(True), a.repeat, torch)
    res["games_per_s"] = G / (res["noise"]["median_ms"] * 1e-3)
    res["cell_updates_per_s"] = float(G) * K * J / (res["noise"]["median_ms"] * 1e-3)
    res["noise_over_stationary"] = res["noise"]["median_ms"] / res["stationary"]["median_ms"]
    res["dev_share_mean"] = float(nout["dev_share"].mean().item())
    res["unprofitable"] = float((nout["gain"] < 0).double().mean().item())
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
