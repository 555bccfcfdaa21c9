"""Rates of the tuple form of greedy play (thrl_tuple_policy, thrl_tuple_walk) at 65,536 games of the QTable-vs-Reinforce
config (21 x 21 actions, T = 441 tuples), float32 tables, after 20 training episodes, each against its yardstick in the
same process:

  extract      thrl_tuple_policy: both agents' strategies [G, 2, T]
  looped       the route without it: T calls of thrl_nn_act at one price each (the prices laid out beforehand, the
               actions written straight into a [T, G] array), thrl_crossplay's extraction of the table rows and a torch
               gather of the rows of the tuple prices, assembled with torch into the same [G, 2, T] array
  self_walk    one thrl_tuple_walk with identity seats from the training states
  rounds_8     8 re-seated rounds ("rotate") from the same strategies
  launch       one 10-episode training launch of the same batch (episode kernel + one Reinforce update), for scale

    python profiles/tuple_play_rate.py [--games N] [--out profiles/tuple_play_rate.json]

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
CFG = {"agents": [dict(AG), dict(name="Reinforce", gamma=0.995, actions=21, states=1, action_range=[0.2, 0.4])],
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
    ap.add_argument("--games", type=int, default=1 << 16)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, crossplay as xp, deviation as dv, tuple_play as tp
    from th_rl_amd.mixed import MixedGameBatch
    G, R = a.games, a.rounds
    mb = MixedGameBatch(CFG, n_games=G, dtype="float32", seed=1).init_tables()
    dev = mb.device
    tabs = tp.tables(CFG)
    T, N = int(tabs["T"]), 2
    # networks whose greedy action moves with the price (kinks inside the price range), 4,096 distinct ones
    rs = np.random.RandomState(0)
    rb = mb.nn[1]
    n = min(G, 4096)
    w = np.zeros((n, rb.P), np.float32)
    w1 = rs.uniform(-1, 1, (n, 256))
    w[:, :256], w[:, 256:512] = w1, -w1 * rs.uniform(tabs["price"].min(), tabs["price"].max(), (n, 256))
    w[:, 512:] = rs.uniform(-1, 1, (n, rb.P - 512))
    rb.params.copy_(torch.from_numpy(w).to(dev).repeat((G + n - 1) // n, 1)[:G])
    mb.run(20, per_game_logs=False)

    price = torch.from_numpy(tabs["price"]).to(dev)
    pol = torch.empty((G, N, T), dtype=torch.int16, device=dev)
    p = _lib.TuplePolicyArgs()
    p.n_games, p.n_tuples = G, T
    p.kind[0], p.kind[1] = 0, 1
    p.nn_params[1] = rb.params.data_ptr()
    p.price, p.tuple_policy = price.data_ptr(), pol.data_ptr()

    def extract():
        _lib.check(mb.L.thrl_tuple_policy(ctypes.byref(mb.cfg), mb.q.data_ptr(), ctypes.byref(p), mb._stream()),
                   "thrl_tuple_policy")

    # the looped route
    price_rows = price[:, None].expand(T, G).contiguous()
    acts = torch.zeros((T, G), dtype=torch.int32, device=dev)
    row = torch.from_numpy(np.clip(np.rint(tabs["price"] / 10.0 * 100.0), 0, 100).astype(np.int64)).to(dev)
    P = xp.policy_entries(mb)
    rows_pol = torch.empty((G, P), dtype=torch.int16, device=dev)
    keep = [torch.zeros((N, 1), dtype=torch.int32, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev),
            torch.zeros((2, N), dtype=torch.float64, device=dev)]
    x = _lib.CrossplayArgs()
    x.n_games, x.n_matches, x.horizon = G, 1, 1
    x.seat, x.state0, x.policy = keep[0].data_ptr(), mb.state.data_ptr(), rows_pol.data_ptr()
    x.mu, x.lam = keep[1][:1].data_ptr(), keep[1][1:].data_ptr()
    x.cycle_reward, x.cycle_action = keep[2][0].data_ptr(), keep[2][1].data_ptr()
    looped_out = {}

    def looped():
        for t in range(T):
            _lib.check(mb.L.thrl_nn_act(G, rb.A, rb.params.data_ptr(), price_rows[t].data_ptr(), None, acts[t].data_ptr(),
                                        None, mb._stream()), "thrl_nn_act")
        _lib.check(mb.L.thrl_crossplay(ctypes.byref(mb.cfg), mb.q.data_ptr(), ctypes.byref(x), mb._stream()), "thrl_crossplay")
        looped_out["pol"] = torch.stack([rows_pol[:, :101].index_select(1, row), acts.t().to(torch.int16)], dim=1)

    # the walks
    H = dv.default_horizon([21, 21])
    d_rew, d_sca = torch.from_numpy(tabs["reward"]).to(dev), torch.from_numpy(tabs["scaled"]).to(dev)
    start = tp.start_tuples(mb, tabs).contiguous()
    seats = [torch.from_numpy(s).to(dev) for s in [xp.identity(N, G)] + xp.pairings(np.zeros(G, int), 1, "rotate", R)]
    out = {"mu": torch.zeros((G,), dtype=torch.int32, device=dev), "lam": torch.zeros((G,), dtype=torch.int32, device=dev),
           "cycle_start": torch.zeros((G,), dtype=torch.int32, device=dev),
           "cycle_reward": torch.zeros((N, G), dtype=torch.float64, device=dev),
           "cycle_action": torch.zeros((N, G), dtype=torch.float64, device=dev)}
    wk = _lib.TupleWalkArgs()
    wk.n_games, wk.n_matches, wk.n_tuples, wk.horizon = G, G, T, H
    wk.start, wk.tuple_policy, wk.reward, wk.scaled = start.data_ptr(), pol.data_ptr(), d_rew.data_ptr(), d_sca.data_ptr()
    for f, t in out.items():
        setattr(wk, f, t.data_ptr())

    def walk(seat):
        wk.seat = seat.data_ptr()
        _lib.check(mb.L.thrl_tuple_walk(ctypes.byref(mb.cfg), ctypes.byref(wk), mb._stream()), "thrl_tuple_walk")

    res = {"games": G, "tuples": T, "rounds": R, "horizon": H, "episodes": mb.episode,
           "policy_bytes_per_game": 2 * N * T, "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["extract"] = timed(extract, a.repeat, torch)
    res["looped"] = timed(looped, max(2, a.repeat // 2), torch)
    res["routes_agree"] = bool(torch.equal(pol, looped_out["pol"]))
    pn = pol.cpu().numpy().view(np.uint16)
    sample = pn[:: max(1, G // 4096), 1, :]
    res["neural_rows_with_3_or_more_actions"] = float(np.mean([np.unique(r).size >= 3 for r in sample]))
    res["self_walk"] = timed(lambda: walk(seats[0]), a.repeat, torch)
    mu, lam = out["mu"].cpu().numpy(), out["lam"].cpu().numpy()
    res["no_start"] = int((start.cpu().numpy() < 0).sum())
    res["self_mean_mu_plus_lam"] = float((mu + lam)[mu >= 0].mean())
    res["self_max_mu_plus_lam"] = int((mu + lam).max())
    res["self_fixed_points"] = int((lam == 1).sum())
    res["rounds_%d" % R] = timed(lambda: [walk(s) for s in seats[1:]], a.repeat, torch)
    mu, lam = out["mu"].cpu().numpy(), out["lam"].cpu().numpy()
    res["cross_mean_mu_plus_lam"] = float((mu + lam)[mu >= 0].mean())
    res["cross_max_mu_plus_lam"] = int((mu + lam).max())
    res["training_launch_10"] = timed(lambda: mb.run(10, per_game_logs=False), 3, torch)
    res["ratio_looped_over_extract"] = res["looped"]["median_ms"] / res["extract"]["median_ms"]
    res["ratio_extract_over_launch"] = res["extract"]["median_ms"] / res["training_launch_10"]["median_ms"]
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["routes_agree"] and res["ratio_looped_over_extract"] >= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
