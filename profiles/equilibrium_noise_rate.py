"""Rate of the equilibrium check under demand noise (thrl_equilibrium_noise) on 65,536 trained headline games, float32,
noise_prob 0.05, both agents, with its yardsticks on the same batch in the same process:

  extract        the extraction pass alone (thrl_crossplay with one throw-away match)
  stationary     thrl_stationary with THRL_STAT_POLICY_GIVEN (pi stored: the weights of the check)
  equilibrium    thrl_equilibrium, the noise-free check, both agents
  noise          thrl_equilibrium_noise with THRL_EQN_POLICY_GIVEN, weights = that pi, eval_tol 1e-12, max_sweeps 8192
  noise_1e-9     the same at eval_tol 1e-9
  iters, sweeps  the distribution of the rounds and of the evaluation sweeps per (agent, game)

    python profiles/equilibrium_noise_rate.py [--games N] [--episodes E] [--out profiles/equilibrium_noise_rate.json]

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


def stats(x):
    x = np.asarray(x)
    q = np.quantile(x, [0.25, 0.5, 0.75])
    return {"min": int(x.min()), "q25": float(q[0]), "q50": float(q[1]), "q75": float(q[2]), "max": int(x.max()),
            "mean": float(x.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, attractors as at, crossplay as xp, deviation as dv, stationary as sn
    from th_rl_amd.batched import GameBatch
    G = a.games
    gb = GameBatch(CFG, n_games=G, dtype="float32", seed=1).init_tables()
    gb.run(a.episodes, logs=False)
    dev = gb.device
    N, P = gb.N, at.policy_entries(gb)
    tabs = sn.tables(CFG)
    J, W = tabs["n_cells"], tabs["band_w"]
    keep = {f: torch.from_numpy(np.ascontiguousarray(tabs[f])).to(dev)
            for f in ("cell_rows", "cell_w", "det_cell", "band_lo", "band", "noise_reward", "noise_price")}
    pol = torch.empty((G, P), dtype=torch.int16, device=dev)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)

    # the extraction pass: cross-play with one throw-away match
    seat = torch.from_numpy(xp.identity(N, G)).to(dev)
    c = _lib.CrossplayArgs()
    c.n_games, c.n_matches, c.horizon, c.policy, c.seat = G, 1, dv.default_horizon([21, 21]), pol.data_ptr(), seat.data_ptr()
    cout = {"mu": i32(G), "lam": i32(G), "cycle_reward": f64(N, G), "cycle_action": f64(N, G)}
    for f, t in cout.items():
        setattr(c, f, t.data_ptr())
    c.state0 = gb.state.data_ptr()

    def extract():
        _lib.check(gb.L.thrl_crossplay(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(c), gb._stream()), "thrl_crossplay")

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

    # thrl_equilibrium, the noise-free check
    e = _lib.EquilibriumArgs()
    e.n_games, e.agents, e.state0 = G, 3, gb.state.data_ptr()
    eout = {"mu": i32(G), "lam": i32(G)}
    eout.update({f: i32(N, G) for f in ("iters", "n_diff_all", "n_diff_on")})
    eout.update({f: f64(N, G) for f in ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on")})
    for f, t in eout.items():
        setattr(e, f, t.data_ptr())

    def equilibrium():
        _lib.check(gb.L.thrl_equilibrium(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(e), gb._stream()), "thrl_equilibrium")

    # thrl_equilibrium_noise from the policy, weighted by pi
    n = _lib.EquilibriumNoiseArgs()
    n.n_games, n.agents, n.flags, n.n_cells, n.band_w, n.max_sweeps = G, 3, _lib.EQN_POLICY_GIVEN, J, W, 8192
    n.noise_prob, n.policy, n.weights = 0.05, pol.data_ptr(), sout["pi"].data_ptr()
    nout = {f: i32(N, G) for f in ("iters", "sweeps", "n_diff_all")}
    nout.update({f: f64(N, G) for f in ("loss_all", "loss_all_mean", "loss_w", "diff_w", "v_w")})
    for f in ("cell_rows", "det_cell", "band_lo", "band", "noise_reward"):
        setattr(n, f, keep[f].data_ptr())
    for f, t in nout.items():
        setattr(n, f, t.data_ptr())

    def noise(eval_tol):
        n.eval_tol = eval_tol
        _lib.check(gb.L.thrl_equilibrium_noise(ctypes.byref(gb.cfg), None, ctypes.byref(n), gb._stream()),
                   "thrl_equilibrium_noise")

    res = {"games": G, "episodes": a.episodes, "n_cells": J, "band_w": W, "noise_prob": 0.05, "agents": [0, 1],
           "max_sweeps": 8192, "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["extract"] = timed(extract, a.repeat, torch)
    res["stationary"] = timed(stationary, a.repeat, torch)
    res["equilibrium"] = timed(equilibrium, a.repeat, torch)
    res["noise"] = timed(lambda: noise(1e-12), a.repeat, torch)
    it, sw = nout["iters"].cpu().numpy(), nout["sweeps"].cpu().numpy()
    res["capped"] = int((it < 0).sum())
    res["iters"], res["sweeps"] = stats(it[it >= 0]), stats(sw)
    res["br_all"] = float((nout["loss_all"].cpu().numpy() <= 0.0).mean())
    res["br_w"] = float((nout["loss_w"].cpu().numpy() <= 0.0).mean())
    res["solves_per_s"] = N * G / (res["noise"]["median_ms"] * 1e-3)
    res["cell_updates_per_s"] = float(sw.sum()) * J / (res["noise"]["median_ms"] * 1e-3)
    res["noise_1e-9"] = timed(lambda: noise(1e-9), a.repeat, torch)
    res["sweeps_1e-9"] = stats(nout["sweeps"].cpu().numpy())
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
