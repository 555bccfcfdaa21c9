"""Deviation analysis of trained QTable games (thrl_deviation, include/thrl.h): the test of the algorithmic-collusion
literature (Calvano, Calzolari, Denicolo, Pastorello, AER 2020) that tells agents who sustain high prices by
threatening punishment from agents who never learned to undercut.  Take the greedy policies, find the limit cycle of
greedy play, force one agent to deviate for dev_len periods, and watch whether the others punish, whether play
returns to the cycle and whether the deviation paid.

The per-game outputs (mu, lam: the pre-shock cycle; mu_post, lam_post, ret_step: the return; act_dev; gain; the
cycle's mean reward and action per agent) come from one kernel; the definitions are in include/thrl.h.  This module
parses training.deviation, runs the kernel for a GameBatch or an all-QTable MixedGameBatch (the response rows either
downloaded or reduced per group on the device by group_stats), and summarises per (group, deviator) on the host:

    games, cycles (lam > 0), fixed_points (lam == 1), returned (ret_step >= 0), unprofitable (gain < 0)
    lam_hist        counts of lam in LAM_BINS
    ret_step_mean   mean ret_step over the games that returned
    delta_mean, delta_q25 / q50 / q75   the profit gain over the games with lam > 0:
                    delta = (sum_i cycle_reward_i - Nash) / (Cartel - Nash), Nash and Cartel from
                    environment.get_optimal(), the sum in agent order in float64
    gain_mean       mean gain over all games

Statistics that have no games are None.  Shards combine exactly: their per-game arrays are concatenated in global game
order (combine) and summarised as one run.
"""
import ctypes
import os
import types

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .analysis import save_json  # noqa: F401  (dv.save_json stays a public name)

DEFAULTS = dict(steps=32, dev_len=1, action="best_response", horizon=None)
ROW_BUDGET = 256 << 20          # bytes per device row buffer and chunk (trainer.GAME_LOG_BUDGET)
MAX_DEFAULT_HORIZON = 65536
INT_FIELDS = ("mu", "lam", "mu_post", "lam_post", "ret_step", "act_dev")
LAM_BINS = ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 8), (9, 16), (17, 64), (65, None))
QUANTILES = (0.25, 0.5, 0.75)
NEURAL_FOLLOW_UP = ("deviation analysis runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def lam_bin_names():
    return [str(a) if a == b else ("%d-%d" % (a, b) if b is not None else ">%d" % (a - 1)) for a, b in LAM_BINS]


def default_horizon(n_actions):
    """H = min(prod_i n_actions_i + 1, 65536): after the first step the state is a function of the action tuple, so
    with H >= prod + 1 a cycle always lies within the horizon."""
    h = 1
    for a in n_actions:
        h *= int(a)
        if h >= MAX_DEFAULT_HORIZON:
            return MAX_DEFAULT_HORIZON
    return min(h + 1, MAX_DEFAULT_HORIZON)


def check_config(config):
    """ValueError for a config with neural agents (the analysis needs every agent's greedy table)."""
    an.check_qtable_only(config, "deviation", NEURAL_FOLLOW_UP)


def action_index(action):
    """'best_response' -> -1, an int -> that action index."""
    if action == "best_response":
        return -1
    if isinstance(action, bool) or not isinstance(action, (int, np.integer)) or int(action) < 0:
        raise ValueError("deviation action must be 'best_response' or an action index >= 0, got %r" % (action,))
    return int(action)


def parse_options(opt, config):
    """training.deviation (true or a dict) -> the dict with every key filled in: agents (the deviators, default all),
    steps K, dev_len L, action ('best_response' or an index), horizon (None = default_horizon)."""
    check_config(config)
    n = len(config["agents"])
    out = an.options("deviation", opt, dict(DEFAULTS, agents=list(range(n))), tables=True)
    out["agents"] = [int(d) for d in out["agents"]]
    if not out["agents"] or any(not 0 <= d < n for d in out["agents"]):
        raise ValueError("training.deviation.agents %r: deviators must lie in [0, %d)" % (out["agents"], n))
    out["steps"], out["dev_len"] = int(out["steps"]), int(out["dev_len"])
    if not 1 <= out["dev_len"] <= out["steps"] <= _lib.DEV_MAX_STEPS:
        raise ValueError("training.deviation: needs 1 <= dev_len <= steps <= %d, got dev_len=%d steps=%d"
                         % (_lib.DEV_MAX_STEPS, out["dev_len"], out["steps"]))
    idx = action_index(out["action"])
    if idx >= 0:
        acts = [int(dict(_lib.QTABLE_DEFAULTS, **config["agents"][d])["actions"]) for d in out["agents"]]
        if idx >= min(acts):
            raise ValueError("training.deviation.action=%d is not an action of every deviator (%s)" % (idx, acts))
    if out["horizon"] is not None:
        out["horizon"] = int(out["horizon"])
        if not 1 <= out["horizon"] <= _lib.DEV_MAX_HORIZON:
            raise ValueError("training.deviation.horizon=%d out of [1, %d]" % (out["horizon"], _lib.DEV_MAX_HORIZON))
    return out


# ---------------------------------------------------------------------------------------------- the device call
def run(batch, deviator=0, steps=32, dev_len=1, action="best_response", horizon=None, state0=None, rows=False,
        group_stats=None, budget=ROW_BUDGET, q=None):
    """thrl_deviation for every game of `batch` (a GameBatch or an all-QTable MixedGameBatch; see
    GameBatch.deviation).  The rows are produced in tau-chunks of at most `budget` bytes per device buffer.
    q: a device tensor shaped and typed like batch.q analysed in place of the batch's tables (e.g. the tables at
    convergence, convergence.Tracker.tables_at_convergence)."""
    import torch
    G, N = batch.G, batch.N
    K, L = int(steps), int(dev_len)
    n_actions = [int(batch.cfg.n_actions[i]) for i in range(N)]
    H = default_horizon(n_actions) if horizon is None else int(horizon)
    if not 0 <= int(deviator) < N:
        raise ThrlError("deviator %d out of [0, %d)" % (int(deviator), N))
    if group_stats is not None and group_stats.G != G:
        raise ThrlError("group_stats spec is for %d games, this batch has %d" % (group_stats.G, G))
    dev = batch.device
    q = an.tables_tensor(batch, q, "deviation")
    a = _lib.DeviationArgs()
    a.n_games, a.deviator, a.dev_len, a.n_steps, a.horizon = G, int(deviator), L, K, H
    a.dev_action = action_index(action)
    with torch.cuda.device(dev):
        s0 = an.state0_tensor(batch, state0, G, "deviation")
        out = {f: torch.zeros((G,), dtype=torch.int32, device=dev) for f in INT_FIELDS}
        out.update(cycle_reward=torch.zeros((N, G), dtype=torch.float64, device=dev),
                   cycle_action=torch.zeros((N, G), dtype=torch.float64, device=dev),
                   gain=torch.zeros((G,), dtype=torch.float64, device=dev))
        a.state0 = s0.data_ptr()
        gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
        a.sweep_gamma = gam.data_ptr() if gam is not None else None
        an.bind(a, out)
        want = bool(rows) or group_stats is not None
        chunk = max(1, min(K, int(budget) // (8 * N * G))) if want else K
        st = group_stats.zeros(K, dev) if group_stats is not None else None
        host_r, host_a = [], []
        b0 = 0
        while True:
            k = min(chunk, K - b0) if want else 0
            rr = ra = None
            if k:
                rr = torch.empty((k, N, G), dtype=torch.float64, device=dev)
                ra = torch.empty((k, N, G), dtype=torch.float64, device=dev)
            a.row_begin, a.row_count = b0, k
            a.reward_rows = rr.data_ptr() if rr is not None else None
            a.action_rows = ra.data_ptr() if ra is not None else None
            _lib.check(batch.L.thrl_deviation(ctypes.byref(batch.cfg), q.data_ptr(), ctypes.byref(a),
                                              batch._stream()), "thrl_deviation")
            if st is not None and k:
                group_stats.reduce(batch.L, rr, ra, k, st, batch._stream(), at=b0)
            if rows and k:
                host_r.append(rr.cpu().numpy())
                host_a.append(ra.cpu().numpy())
            b0 += k
            if b0 >= K or not want:
                break
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["horizon"] = H
        if rows:
            res["reward_rows"] = np.concatenate(host_r, axis=0)
            res["action_rows"] = np.concatenate(host_a, axis=0)
        if st is not None:
            from .group_stats import to_numpy
            res["group_stats"] = to_numpy(st)
    return res


# ---------------------------------------------------------------------------------------------- host side
def optimal(config):
    """(Nash, Cartel) total rewards: environment.get_optimal() of the config's environment (without constructing
    one, which would draw from numpy's global stream)."""
    from .environments import NoisyPriceState
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    n = int(env.get("nplayers", len(config["agents"])))
    nash, cartel = NoisyPriceState.get_optimal(types.SimpleNamespace(nplayers=n, a=env["a"], b=env["b"]))
    return float(nash), float(cartel)


def profit_gain(cycle_reward, nash, cartel):
    """delta [G] = (sum_i cycle_reward[i] - nash) / (cartel - nash), the sum in agent order in float64."""
    cr = np.asarray(cycle_reward, np.float64)
    tot = cr[0].copy()
    for i in range(1, cr.shape[0]):
        tot = tot + cr[i]
    return (tot - float(nash)) / (float(cartel) - float(nash))


def summarize(games, ids, n_groups, nash, cartel, deviator):
    """One dict per group for one deviator: games = dict of per-game arrays (INT_FIELDS, gain [G], cycle_reward
    [N, G]) in global game order, ids = group id per game."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    lam = np.asarray(games["lam"])
    ret = np.asarray(games["ret_step"])
    gain = np.asarray(games["gain"], np.float64)
    delta = profit_gain(games["cycle_reward"], nash, cartel)
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        lk, rk, gk = lam[m], ret[m], gain[m]
        dk = delta[m][lk > 0]
        hist = [int(np.sum((lk >= lo) & (lk <= hi))) if hi is not None else int(np.sum(lk >= lo))
                for lo, hi in LAM_BINS]
        qs = np.quantile(dk, QUANTILES) if dk.size else [None] * len(QUANTILES)
        out.append({"group": k, "deviator": int(deviator), "games": int(m.sum()), "cycles": int(np.sum(lk > 0)),
                    "fixed_points": int(np.sum(lk == 1)), "returned": int(np.sum(rk >= 0)),
                    "unprofitable": int(np.sum(gk < 0)), "lam_hist": hist,
                    "ret_step_mean": an.num(rk[rk >= 0].mean()) if np.any(rk >= 0) else None,
                    "delta_mean": an.num(dk.mean()) if dk.size else None,
                    "delta_q25": an.num(qs[0]), "delta_q50": an.num(qs[1]), "delta_q75": an.num(qs[2]),
                    "gain_mean": an.num(gk.mean()) if gk.size else None})
    return out


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis."""
    return an.combine(parts)


def describe(options, nash, cartel, summary):
    """deviation.json's content."""
    return {"options": options, "nash": nash, "cartel": cartel, "lam_bins": lam_bin_names(),
            "quantiles": list(QUANTILES), "summary": summary}


# ---------------------------------------------------------------------------------------------- artefacts
def load_games(d, deviator):
    """The per-game arrays one run directory (or shard) holds for `deviator`."""
    cyc = np.load(os.path.join(d, "dev_cycle.npy"))
    post = np.load(os.path.join(d, "dev%d_post.npy" % deviator))
    return {"mu": cyc[0], "lam": cyc[1], "mu_post": post[0], "lam_post": post[1], "ret_step": post[2],
            "act_dev": post[3], "gain": np.load(os.path.join(d, "dev%d_gain.npy" % deviator)),
            "cycle_reward": np.load(os.path.join(d, "dev_cycle_reward.npy")),
            "cycle_action": np.load(os.path.join(d, "dev_cycle_action.npy"))}


def merged(shards, out, config, opt, ids, n_groups, first):
    """deviation.json of a sharded run (launch.merge_analysis): per deviator the shards' arrays concatenated in global
    game order and summarised as one run."""
    nash, cartel = optimal(config)
    summary = []
    for d in opt["agents"]:
        summary += summarize(combine(load_games(s, d) for s in shards), ids, n_groups, nash, cartel, d)
    return describe(opt, nash, cartel, summary)


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, spec=None, histograms=False, budget=ROW_BUDGET,
                    q=None, state0=None):
    """train_one's training.deviation outputs: the per-game .npy files, dev<d>_*.npy group statistics with a spec,
    and deviation.json.  q / state0 (device tensors): the tables and start prices analysed in place of the batch's
    (opt["tables"] == "converged")."""
    from . import trainer
    nash, cartel = optimal(config)
    summary = []
    for d in opt["agents"]:
        r = run(batch, deviator=d, steps=opt["steps"], dev_len=opt["dev_len"], action=opt["action"],
                horizon=opt["horizon"], group_stats=spec, budget=budget, q=q, state0=state0)
        if d == opt["agents"][0]:
            np.save(os.path.join(exp_path, "dev_cycle.npy"), np.stack([r["mu"], r["lam"]]).astype(np.int32))
            np.save(os.path.join(exp_path, "dev_cycle_reward.npy"), r["cycle_reward"])
            np.save(os.path.join(exp_path, "dev_cycle_action.npy"), r["cycle_action"])
        np.save(os.path.join(exp_path, "dev%d_post.npy" % d),
                np.stack([r["mu_post"], r["lam_post"], r["ret_step"], r["act_dev"]]).astype(np.int32))
        np.save(os.path.join(exp_path, "dev%d_gain.npy" % d), r["gain"])
        if spec is not None:
            trainer.save_group_stats(exp_path, "dev%d" % d, r["group_stats"], spec, histograms)
        summary += summarize(r, ids, n_groups, nash, cartel, d)
    opt = dict(opt, horizon_used=int(r["horizon"]))
    save_json(os.path.join(exp_path, "deviation.json"), describe(opt, nash, cartel, summary))
