"""Throughput of the wave and tuple kernels with and without per-game logs (thrl_buffers.game_reward_log /
game_action_log), in one process, the two runs of each case alternating launch by launch from the same start:

    python profiles/game_logs_rate.py [--reps 5] [--step-timeout 300] [--out OUT.json] [--no-generic]

Cases: the headline shape (2^20 games, two QTable agents, float32, 20-episode launches) and the three-player tuple
shape (65,536 games).  Each step (one launch of one run) is guarded by its own time limit (faulthandler: the process
dumps its stack and exits).  Records env-steps/s per run and checks that the logged run's tables, counters, state and
mean logs equal the unlogged run's (bit for bit; the tuple kernel's atomically summed mean logs to 1e-12), and that the
mean over games of the per-game rows is the mean log.  One launch of the generic kernel with per-game logs (the route
AUTO + per_game_logs took before the wave and tuple kernels wrote them) is timed for comparison.
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
THREE = {"agents": [dict(AG, actions=11, states=50, action_range=[0.1, 0.3], min_memory=25),
                    dict(AG, actions=21, states=100, action_range=[0.15, 0.35], min_memory=25),
                    dict(AG, actions=5, states=20, action_range=[0.0, 0.3], min_memory=25, max_state=10)],
         "environment": dict(ENV, nplayers=3, max_steps=25)}
CASES = [("headline_wave", HEADLINE, 1 << 20, 20, "wave"), ("three_players_tuple", THREE, 65536, 32, "tuple")]


def _timed(batch, E, logs, limit):
    import torch
    faulthandler.dump_traceback_later(limit, exit=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = batch.run(E, per_game_logs=logs, sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    faulthandler.cancel_dump_traceback_later()
    return out, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-generic", action="store_true")
    a = ap.parse_args()
    import torch
    from th_rl_amd.batched import GameBatch
    res = {}
    for name, config, G, E, kernel in CASES:
        T = config["environment"]["max_steps"]
        on = GameBatch(config, n_games=G, dtype="float32", seed=3).init_tables()
        off = GameBatch(config, n_games=G, dtype="float32", seed=3)
        off.set_tables(on.tables_numpy(), on.states_numpy())
        rates = {"on": [], "off": []}
        ok = True
        for rep in range(a.reps + 1):                  # rep 0: warm-up (code objects, first touch), not recorded
            for tag, b in (("off", off), ("on", on)) if rep % 2 else (("on", on), ("off", off)):
                out, dt = _timed(b, E, tag == "on", a.step_timeout)
                assert out["kernel"] == kernel, out["kernel"]
                if tag == "on":
                    o_on = out
                else:
                    o_off = out
                if rep:
                    rates[tag].append(G * E * T / dt)
            if kernel == "wave":       # fixed-point mean logs: the same bits; the tuple kernel's float64 atomics: 1e-12
                ok &= bool(torch.equal(o_on["reward_log"], o_off["reward_log"]) and torch.equal(o_on["action_log"], o_off["action_log"]))
            else:
                ok &= bool(torch.allclose(o_on["reward_log"], o_off["reward_log"], rtol=1e-12, atol=0)
                           and torch.allclose(o_on["action_log"], o_off["action_log"], rtol=1e-12, atol=0))
            ok &= bool(torch.allclose(o_on["game_reward_log"].mean(dim=2), o_on["reward_log"], rtol=1e-12, atol=0))
            del o_on, o_off
        ok &= bool(torch.equal(on.q, off.q) and torch.equal(on.counter, off.counter) and torch.equal(on.state, off.state))
        ok &= on.eps == off.eps
        r = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=v) for k, v in rates.items()}
        r["on_over_off"] = r["on"]["median"] / r["off"]["median"]
        r["outputs_match"] = ok
        r.update(games=G, episodes_per_launch=E, max_steps=T, reps=a.reps)
        del on, off
        torch.cuda.empty_cache()
        if not a.no_generic:                           # today's route for AUTO + per-game logs: one launch
            gen = GameBatch(config, n_games=G, dtype="float32", seed=3, kernel="generic").init_tables()
            out, dt = _timed(gen, E, True, a.step_timeout)
            r["generic_logged"] = G * E * T / dt
            r["gain_over_generic"] = r["on"]["median"] / r["generic_logged"]
            del gen, out
            torch.cuda.empty_cache()
        res[name] = r
        print(json.dumps({name: {k: v for k, v in r.items() if k not in ("on", "off")} | {
            "on": r["on"]["median"], "off": r["off"]["median"]}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(r["outputs_match"] for r in res.values()):
        sys.exit("outputs differ between the logged and the unlogged runs")


if __name__ == "__main__":
    main()
