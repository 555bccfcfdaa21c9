"""Cost of the deviation analysis (thrl_deviation) on the headline shape, in one process:

    python profiles/deviation_rate.py [--reps 5] [--step-timeout 300] [--out OUT.json]
    python profiles/deviation_rate.py --reps 1 --out OUT.json      # under rocprofv3 --kernel-trace --stats

2^20 games, two QTable agents (21 actions, 101 rows), float32 tables, deviator 0, K = 32, L = 1, best response,
default horizon (442), on three kinds of tables: fresh (Philox init), after 200 training episodes, and near-greedy
(the LATE config trained 1,600 episodes, as in group_stats_rate.py).  Per kind: the synchronised call time of
GameBatch.deviation (median over reps after one warm-up; the call includes the download of the per-game outputs), the
per-game mean of mu + lam and of mu_post + lam_post, one 20-episode training launch timed in the same process, and
one k_play_greedy iteration (max_steps 100) for scale.  Each GPU step runs under its own time limit (faulthandler:
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


def measure(gb, a):
    call = lambda: gb.deviation(deviator=0, steps=32, dev_len=1, action="best_response")
    out, _ = _timed(a.step_timeout, call)                         # warm-up
    times = [_timed(a.step_timeout, call)[1] for _ in range(a.reps)]
    _, t_play = _timed(a.step_timeout, lambda: gb.play_greedy(iters=1))
    _, t_play = _timed(a.step_timeout, lambda: gb.play_greedy(iters=1))
    return dict(call_ms=dict(median=1e3 * float(np.median(times)), min=1e3 * float(np.min(times)),
                             all=[1e3 * t for t in times]),
                mu_plus_lam=float(np.mean(out["mu"].astype(np.int64) + out["lam"])),
                post_mu_plus_lam=float(np.mean(out["mu_post"].astype(np.int64) + out["lam_post"])),
                lam_found=float(np.mean(out["lam"] > 0)), fixed_points=float(np.mean(out["lam"] == 1)),
                returned=float(np.mean(out["ret_step"] >= 0)), play_greedy_1_iter_ms=1e3 * t_play)


def train(gb, episodes, a):
    """episodes in launches of 20; returns the time of the last launch (ms)."""
    import torch
    dt = None
    for _ in range(episodes // 20):
        _, dt = _timed(a.step_timeout, lambda: gb.run(20, logs=False, sync=False))
    torch.cuda.synchronize()
    return 1e3 * dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd.batched import GameBatch
    res = dict(games=G, steps=32, dev_len=1, action="best_response", horizon=442, dtype="float32", reps=a.reps)
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
    for k in ("fresh", "trained_200", "near_greedy"):
        r = res[k]
        r["call_over_train_20"] = r["call_ms"]["median"] / r["train_20_episodes_ms"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
