"""Rates of cross-play (thrl_crossplay) at 2^20 headline games, float32, at three points of training (fresh, after 200
episodes, after 1,600), each against its yardsticks in the same process:

  extract      the extraction pass alone (a one-match call) against thrl_policy_track with THRL_TRACK_BASELINE on the
               same batch: same bytes read, same bytes written
  rounds       16 rounds of "rotate": one extraction + 16 walks, against the only route without this entry point:
               16 x (torch gather of the partner tables into a second batch + thrl_deviation without rows)
  launch       one 20-episode training launch of the same batch

    python profiles/crossplay_rate.py [--games N] [--out profiles/crossplay_rate.json]

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
CFG = {"agents": [dict(AG), dict(AG)],
       "environment": dict(name="NoisyPriceState", noise_prob=0, a=10, b=1, nplayers=2, max_steps=100)}


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
    ap.add_argument("--games", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, crossplay as xp, deviation as dv
    from th_rl_amd.batched import GameBatch
    G, R = a.games, a.rounds
    gb = GameBatch(CFG, n_games=G, dtype="float32", seed=1).init_tables()
    dev = gb.device
    rounds = xp.pairings(np.zeros(G, int), 1, "rotate", R)
    seats = [torch.from_numpy(s).to(dev) for s in rounds]
    H = dv.default_horizon([21, 21])
    P = xp.policy_entries(gb)
    pol = torch.empty((G, P), dtype=torch.int16, device=dev)
    out = {"mu": torch.zeros((G,), dtype=torch.int32, device=dev), "lam": torch.zeros((G,), dtype=torch.int32, device=dev),
           "cycle_reward": torch.zeros((2, G), dtype=torch.float64, device=dev),
           "cycle_action": torch.zeros((2, G), dtype=torch.float64, device=dev)}
    x = _lib.CrossplayArgs()
    x.n_games, x.horizon, x.policy, x.state0 = G, H, pol.data_ptr(), gb.state.data_ptr()
    for f, t in out.items():
        setattr(x, f, t.data_ptr())

    def call(seat, matches, flags):
        x.seat, x.n_matches, x.flags = seat.data_ptr(), matches, flags
        _lib.check(gb.L.thrl_crossplay(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(x), gb._stream()), "thrl_crossplay")

    def extract():
        call(seats[0], 1, 0)

    def play_rounds():
        call(seats[0], G, 0)
        for s in seats[1:]:
            call(s, G, _lib.XPLAY_POLICY_GIVEN)

    tr = gb.track_convergence(window=1000)

    def baseline():
        tr._launch(_lib.TRACK_BASELINE)

    # the route without thrl_crossplay: gather agent 1's tables of the partners into a second batch, thrl_deviation
    other = GameBatch(CFG, n_games=G, dtype="float32", seed=1, counters=False)
    other.initialized = True
    off1 = gb.offsets[1]
    d = _lib.DeviationArgs()
    d.n_games, d.deviator, d.dev_len, d.n_steps, d.horizon, d.dev_action = G, 0, 1, 1, H, -1
    d.state0 = gb.state.data_ptr()
    dout = {f: torch.zeros((G,), dtype=torch.int32, device=dev) for f in dv.INT_FIELDS}
    dout.update(cycle_reward=out["cycle_reward"].clone(), cycle_action=out["cycle_action"].clone(),
                gain=torch.zeros((G,), dtype=torch.float64, device=dev))
    for f, t in dout.items():
        setattr(d, f, t.data_ptr())

    def gather_route():
        for s in seats:
            other.q[:, :off1].copy_(gb.q[:, :off1])
            other.q[:, off1:].copy_(gb.q[:, off1:].index_select(0, s[1].long()))
            _lib.check(gb.L.thrl_deviation(ctypes.byref(gb.cfg), other.q.data_ptr(), ctypes.byref(d), gb._stream()),
                       "thrl_deviation")

    def launch():
        gb.run(20, logs=False, sync=False)

    res = {"games": G, "rounds": R, "horizon": H, "policy_bytes_per_game": 2 * P, "table_bytes_per_game": 4 * gb.stride,
           "build": {k: v for k, v in _lib.build_info().items() if k != "path"}, "points": []}
    done = 0
    for name, upto in (("fresh", 0), ("200 episodes", 200), ("1,600 episodes", 1600)):
        while done < upto:
            n = min(100, upto - done)
            gb.run(n, logs=False)
            done += n
        pt = {"point": name, "episodes": done, "epsilon": float(gb.eps[0])}
        pt["extract"] = timed(extract, a.repeat, torch)
        pt["policy_track_baseline"] = timed(baseline, a.repeat, torch)
        pt["rounds"] = timed(play_rounds, a.repeat, torch)
        call(seats[R // 2], G, _lib.XPLAY_POLICY_GIVEN)
        one = timed(lambda: call(seats[R // 2], G, _lib.XPLAY_POLICY_GIVEN), a.repeat, torch)
        pt["one_walk"] = one
        mu, lam = out["mu"].cpu().numpy(), out["lam"].cpu().numpy()
        pt["mean_mu_plus_lam"] = float((mu + lam).mean())
        pt["max_mu_plus_lam"] = int((mu + lam).max())
        pt["gather_route"] = timed(gather_route, max(2, a.repeat // 2), torch)
        # the two routes give the same numbers (last round)
        call(seats[-1], G, _lib.XPLAY_POLICY_GIVEN)
        torch.cuda.synchronize()
        pt["routes_agree"] = bool(torch.equal(out["mu"], dout["mu"]) and torch.equal(out["lam"], dout["lam"])
                                  and torch.equal(out["cycle_reward"], dout["cycle_reward"]))
        saved = (gb.q.clone(), gb.counter.clone(), gb.state.clone(), list(gb.eps), gb.episode, list(gb.mem_count))
        pt["training_launch_20"] = timed(launch, 3, torch)
        gb.q.copy_(saved[0]); gb.counter.copy_(saved[1]); gb.state.copy_(saved[2])
        gb.eps, gb.episode, gb.mem_count = saved[3], saved[4], saved[5]
        del saved
        pt["ratio_gather_over_rounds"] = pt["gather_route"]["median_ms"] / pt["rounds"]["median_ms"]
        pt["ratio_rounds_over_launch"] = pt["rounds"]["median_ms"] / pt["training_launch_20"]["median_ms"]
        res["points"].append(pt)
        print(json.dumps(pt), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
