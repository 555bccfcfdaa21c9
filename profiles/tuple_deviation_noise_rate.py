"""Rate of the deviation test under demand noise in tuple form (thrl_tuple_deviation_noise) on 65,536 games of the
reference's example pairing (QTable gamma 0.95 against Reinforce gamma 0.995, 21 actions each, 100 states,
NoisyPriceState noise_prob 0.05) after a short training, resolution 1024, float32, deviator 0, best response, K = 32,
L = 1, strategies and pi given, with its yardstick on the same batch in the same process:

  stationary     tuple_stationary.run with the strategies given and pi stored (thrl_tuple_stationary, tol 1e-12): the
                 weights of the test; the upload of the tables and the download of the outputs are inside the events
  noise          thrl_tuple_deviation_noise on device arrays, weights = that pi, no rows
  noise_rows     the same with reward_rows / action_rows / dist_rows of all K periods

    python profiles/tuple_deviation_noise_rate.py [--games N] [--episodes E] [--out profiles/tuple_deviation_noise_rate.json]

Times are device events around the calls, median of `--repeat` after a warm-up, with the spread (min, max)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENV = dict(name="NoisyPriceState", noise_prob=0.05, a=10, b=1, nplayers=2, max_steps=100)
CFG = {"agents": [dict(name="QTable", gamma=0.95, actions=21, states=100, alpha=0.1, eps_end=0.001, epsilon=0.5,
                       eps_step=0.9995, action_range=[0.2, 0.4]),
                  dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
       "environment": dict(ENV)}


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
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--dev-len", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuple_deviation_noise_rate.json"))
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, tuple_play as tp, tuple_stationary as ts
    from th_rl_amd.mixed import MixedGameBatch
    G, K = a.games, a.steps
    mb = MixedGameBatch(CFG, n_games=G, dtype="float32", seed=1).init_tables()
    mb.run(a.episodes, per_game_logs=False)
    dev, N = mb.device, mb.N
    tabs = ts.tables(CFG, a.resolution)
    T, J, W = int(tabs["n_tuples"]), int(tabs["n_cells"]), int(tabs["band_w"])
    tpol, cpol = tp.extract(mb, tabs), ts.extract_cells(mb, tabs)
    st = {}

    def stationary():
        st.update(ts.run(mb, pi=True, tuple_policy=tpol, cell_policy=cpol, tabs=tabs))

    res = {"games": G, "episodes": a.episodes, "resolution": a.resolution, "n_tuples": T, "n_cells": J, "band_w": W,
           "lds_bytes": (28 * T + 10 * J + 512 * (2 * N + 2) + 6 + 15) // 16 * 16, "noise_prob": 0.05, "deviator": 0,
           "steps": K, "dev_len": a.dev_len, "action": "best_response",
           "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["stationary"] = timed(stationary, a.repeat, torch)
    it = np.asarray(st["iters"])
    res["stationary_iters"] = {"min": int(it.min()), "q50": float(np.median(it)), "max": int(it.max()), "mean": float(it.mean())}

    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    keep = {f: torch.from_numpy(np.ascontiguousarray(tabs[f], dt)).to(dev)
            for f, dt in (("reward", np.float64), ("scaled", np.float64), ("band_lo", np.int32), ("band", np.float64),
                          ("noise_reward", np.float64))}
    pi = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
    n = _lib.TupleDeviationNoiseArgs()
    n.n_games, n.n_tuples, n.n_cells, n.band_w = G, T, J, W
    n.deviator, n.dev_len, n.n_steps, n.dev_action = 0, a.dev_len, K, -1
    n.noise_prob, n.ret_tol = 0.05, 1e-6
    for i, k in enumerate(tp._kinds(mb)):
        n.kind[i] = tp.KINDS[k]
    gam = torch.from_numpy(np.repeat(np.array([[0.95], [0.995]]), G, axis=1).copy()).to(dev)
    n.sweep_gamma, n.tuple_policy, n.cell_policy, n.weights = gam.data_ptr(), tpol.data_ptr(), cpol.data_ptr(), pi.data_ptr()
    nout = {f: f64(N, G) for f in ("base_reward", "base_action")}
    nout.update({f: f64(G) for f in ("dev_share", "gain", "gain_dev", "low", "dist", "mass")})
    nout.update({f: i32(G) for f in ("low_step", "ret_step")})
    for f, t in list(keep.items()) + list(nout.items()):
        setattr(n, f, t.data_ptr())
    rows = {"reward_rows": f64(K, N, G), "action_rows": f64(K, N, G), "dist_rows": f64(K, G)}

    def noise(with_rows):
        n.row_begin, n.row_count = 0, K if with_rows else 0
        for f, t in rows.items():
            setattr(n, f, t.data_ptr() if with_rows else None)
        _lib.check(mb.L.thrl_tuple_deviation_noise(ctypes.byref(mb.cfg), ctypes.byref(n), mb._stream()),
                   "thrl_tuple_deviation_noise")

    res["noise"] = timed(lambda: noise(False), a.repeat, torch)
    res["noise_rows"] = timed(lambda: noise(True), a.repeat, torch)
    res["games_per_s"] = G / (res["noise"]["median_ms"] * 1e-3)
    res["noise_over_stationary"] = res["noise"]["median_ms"] / res["stationary"]["median_ms"]
    res["steps_over_stationary_steps"] = K / res["stationary_iters"]["mean"]
    solved = it >= 0
    res["base_equals_stat_reward"] = bool(np.array_equal(nout["base_reward"].cpu().numpy()[:, solved],
                                                         np.asarray(st["stat_reward"])[:, solved]))
    res["dev_share_mean"] = float(nout["dev_share"].mean().item())
    res["unprofitable"] = float((nout["gain"] < 0).double().mean().item())
    res["returned"] = float((nout["ret_step"] >= 0).double().mean().item())
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
