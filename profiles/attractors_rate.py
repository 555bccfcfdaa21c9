"""Rates of the attractor analysis (thrl_attractors) at 2^20 headline games, float32, fresh tables, against its
yardsticks in the same process:

  given        the call with THRL_ATTR_POLICY_GIVEN (101 reset starts, per-state outputs)
  extract      the extraction pass alone (thrl_crossplay with one throw-away match)
  both         the call without the flag: extraction + analysis
  crossplay_route   the only route without this entry point: S identity-seat thrl_crossplay calls with
               THRL_XPLAY_POLICY_GIVEN, one per state, each started at a price that encodes to that state's rows.  It
               yields mu and lam of every state's path (no basins, no reset masses); the script asserts that both
               routes give the same lam for every state.
  launch       one 20-episode training launch of the same batch, for scale

    python profiles/attractors_rate.py [--games N] [--out profiles/attractors_rate.json]

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


def state_rows(at):
    """Row of state s (both agents share the grid): the states are the distinct rows in tuple order (include/thrl.h)."""
    act = np.arange(21, dtype=np.float64) / 20.0 * 0.2 + 0.2
    A = 10.0 / 1.0 * act
    p = 10.0 - 1.0 * ((0.0 + A[:, None]) + A[None, :])
    rows = at.encode64(np.where(p > 0.0, p, 0.0).ravel(), 100, 10.0)
    seen = []
    for r in rows.tolist():
        if r not in seen:
            seen.append(r)
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from th_rl_amd import _lib, attractors as at, crossplay as xp, deviation as dv
    from th_rl_amd.batched import GameBatch
    G = a.games
    # Fresh tables, initialised in slices of 2^15 games: one thrl_qtable_init call over G * stride >= 2^32 elements
    # (the headline config from 1,012,478 games on) launches more threads than a grid holds and leaves all but the first
    # (G * stride mod 2^32) / stride games' tables unwritten, which would make the analysis trivial.  Game g of a slice
    # with game_offset is game g of the whole batch (Philox streams are keyed by the global game id).
    gb = GameBatch(CFG, n_games=G, dtype="float32", seed=1)
    for lo in range(0, G, 1 << 15):
        part = GameBatch(CFG, n_games=min(1 << 15, G - lo), dtype="float32", seed=1, game_offset=lo, counters=False).init_tables()
        gb.q[lo:lo + part.G].copy_(part.q)
        gb.state[lo:lo + part.G].copy_(part.state)
        del part
    gb.initialized = True
    dev = gb.device
    S, P, K, N = at.n_states(gb), at.policy_entries(gb), at.KEEP, gb.N
    rows, w = at.starts(CFG)
    t_rows, t_w = torch.from_numpy(rows).to(dev), torch.from_numpy(w).to(dev)
    pol = torch.empty((G, P), dtype=torch.int16, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    out = {f: i32(G) for f in at.GAME_INT}
    out.update({f: i32(K, G) for f in at.SLOT_INT})
    out.update({f: f64(K, N, G) for f in at.SLOT_FLOAT})
    out.update(reset_mass=f64(K, G), reset_mass_other=f64(G), reset_reward=f64(N, G))
    out.update(state_rep=torch.zeros((G, S), dtype=torch.int16, device=dev),
               state_mu=torch.zeros((G, S), dtype=torch.int16, device=dev))
    x = _lib.AttractorsArgs()
    x.n_games, x.n_starts, x.start_rows, x.start_w = G, int(w.size), t_rows.data_ptr(), t_w.data_ptr()
    x.state0, x.policy = gb.state.data_ptr(), pol.data_ptr()
    for f, t in out.items():
        setattr(x, f, t.data_ptr())

    def attractors(flags):
        x.flags = flags
        _lib.check(gb.L.thrl_attractors(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(x), gb._stream()), "thrl_attractors")

    # cross-play: identity seats, one call per state
    seat = torch.from_numpy(xp.identity(N, G)).to(dev)
    c = _lib.CrossplayArgs()
    c.n_games, c.n_matches, c.horizon, c.policy, c.seat = G, G, dv.default_horizon([21, 21]), pol.data_ptr(), seat.data_ptr()
    cout = {"mu": i32(G), "lam": i32(G), "cycle_reward": f64(N, G), "cycle_action": f64(N, G)}
    for f, t in cout.items():
        setattr(c, f, t.data_ptr())
    # headline: both agents share the grid, state s is the row pair (r, r), and price r / 10 encodes to row r
    plan_rows = sorted(set(range(20, 61)))
    assert len(plan_rows) == S
    prices = [torch.full((G,), r * 10.0 / 100.0, dtype=torch.float64, device=dev) for r in plan_rows]

    def xplay(price, flags):
        c.state0, c.flags = price.data_ptr(), flags
        _lib.check(gb.L.thrl_crossplay(ctypes.byref(gb.cfg), gb.q.data_ptr(), ctypes.byref(c), gb._stream()), "thrl_crossplay")

    def extract():
        c.n_matches = 1
        xplay(prices[0], 0)
        c.n_matches = G

    def crossplay_route():
        for p in prices:
            xplay(p, _lib.XPLAY_POLICY_GIVEN)

    def launch():
        gb.run(20, logs=False, sync=False)

    res = {"games": G, "n_states": S, "n_starts": int(w.size), "policy_bytes_per_game": 2 * P,
           "build": {k: v for k, v in _lib.build_info().items() if k != "path"}}
    res["extract"] = timed(extract, a.repeat, torch)
    res["given"] = timed(lambda: attractors(_lib.ATTR_POLICY_GIVEN), a.repeat, torch)
    res["both"] = timed(lambda: attractors(0), a.repeat, torch)
    res["crossplay_route"] = timed(crossplay_route, a.repeat, torch)
    # the two routes agree on lam of every state (the states of games with more than KEEP attractors are left out)
    attractors(_lib.ATTR_POLICY_GIVEN)
    torch.cuda.synchronize()
    srow = state_rows(at)
    assert len(srow) == S
    srep = out["state_rep"].to(torch.int32)
    agree, compared = True, 0
    for s in range(S):
        xplay(prices[plan_rows.index(int(srow[s]))], _lib.XPLAY_POLICY_GIVEN)
        lam_s = torch.zeros((G,), dtype=torch.int32, device=dev)
        known = torch.zeros((G,), dtype=torch.bool, device=dev)
        for k in range(K):
            hit = out["rep"][k] == srep[:, s]
            lam_s = torch.where(hit, out["lam"][k], lam_s)
            known |= hit
        agree = agree and bool(torch.equal(lam_s[known], cout["lam"][known]))
        agree = agree and bool(torch.equal(out["state_mu"][:, s].to(torch.int32)[known], cout["mu"][known]))
        compared += int(known.sum())
    res["routes_agree"], res["states_compared"] = agree, compared
    assert agree, "thrl_attractors and the cross-play route disagree on lam / mu of some state"
    n_attr = out["n_attr"].cpu().numpy()
    res["n_attr_mean"], res["n_attr_max"] = float(n_attr.mean()), int(n_attr.max())
    res["share_two_or_more"] = float((n_attr >= 2).mean())
    res["largest_basin_share_mean"] = float(out["basin"][0].double().mean().item() / S)
    assert res["share_two_or_more"] >= 0.5, "the tables are not the fresh seeded ones"
    res["training_launch_20"] = timed(launch, 3, torch)
    res["ratio_route_over_given"] = res["crossplay_route"]["median_ms"] / res["given"]["median_ms"]
    res["beats_route_by_more_than_both_spreads"] = bool(
        res["crossplay_route"]["min_ms"] - res["given"]["max_ms"]
        > (res["crossplay_route"]["max_ms"] - res["crossplay_route"]["min_ms"]) + (res["given"]["max_ms"] - res["given"]["min_ms"]))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
