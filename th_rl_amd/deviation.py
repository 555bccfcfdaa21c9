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

Under demand noise (thrl_deviation_noise; the option "noise" of training.deviation) a game follows no single path, and
the test becomes the propagation of a distribution over the price cells of stationary.py: run_noise() starts from the
long-run distribution of noisy greedy play (stationary.run's pi from the reset start) or from weights of the caller's,
replaces the deviator's action in every cell for dev_len periods and returns the expected response: base_reward,
base_action [N, G], dev_share, gain, gain_dev, low, dist, mass [G], low_step, ret_step [G] and, when asked, the rows
E_i(tau), A_i(tau) [steps, N, G] and dist_rows [steps, G].  summarize_noise() gives per (group, deviator) games, solved,
deviates, dev_share_mean, unprofitable, gain_mean and its quantiles, gain_dev_mean, low_mean, returned, ret_step_mean
and dist_mean.  The noise-free artefacts are what they were; the noisy ones are devn_*.npy, devn<d>_*.npy and
deviation_noise.json.
"""
import ctypes
import json
import os
import types

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .analysis import save_json  # noqa: F401  (dv.save_json stays a public name)

DEFAULTS = dict(steps=32, dev_len=1, action="best_response", horizon=None)
NOISE_DEFAULTS = dict(noise_prob=None, ret_tol=1e-6, tol=1e-12, max_iters=8192)
NOISE_FLOAT = ("dev_share", "gain", "gain_dev", "low", "dist", "mass")
NOISE_INT = ("low_step", "ret_step")
NOISE_AGENT = ("base_reward", "base_action")
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
    steps K, dev_len L, action ('best_response' or an index), horizon (None = default_horizon).  The optional key
    "noise" (true or {"noise_prob": a number in (0, 1] or None = the run's own noise, refused for a noise-free run as
    training.stationary does; "ret_tol": the distance at which play counts as returned; "tol", "max_iters": the
    stopping rule of the stationary iteration the weights come from}) asks for the test under demand noise as well;
    it stays in the result, filled in, only when given."""
    check_config(config)
    noise = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        noise = opt.pop("noise")
        noise = None if noise is None or noise is False else parse_noise(noise, config)
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
    if noise is not None:
        out["noise"] = noise
    return out


def parse_noise(noise, config):
    """training.deviation.noise (true or a dict) -> the dict with every key filled in."""
    from . import stationary as sn
    name = "training.deviation.noise"
    out = an.options("deviation.noise", noise, NOISE_DEFAULTS)
    if out["noise_prob"] is None:       # the run's own noise: refuse a noise-free run before training
        an.check_own_noise(config, name)
    else:
        out["noise_prob"] = sn.check_prob(out["noise_prob"], name + ".noise_prob")
    for f in ("ret_tol", "tol"):
        t = out[f]
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0.0:
            raise ValueError("%s.%s must be a number >= 0, got %r" % (name, f, t))
        out[f] = float(t)
    m = out["max_iters"]
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= _lib.STAT_MAX_ITERS:
        raise ValueError("%s.max_iters must be an integer in [1, %d], got %r" % (name, _lib.STAT_MAX_ITERS, m))
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


def run_noise(batch, deviator=0, steps=32, dev_len=1, action="best_response", noise_prob=None, ret_tol=1e-6,
              weights="stationary", rows=False, group_stats=None, budget=ROW_BUDGET, q=None, policy=None, n_games=None,
              tabs=None, tol=1e-12, max_iters=8192):
    """thrl_deviation_noise for the first n_games (default all) games of `batch` (a GameBatch or an all-QTable
    MixedGameBatch; see AnalysisMethods.deviation_noise).  tabs: stationary.tables(batch.config), or a dict that
    replaces some of them.  weights="stationary": the policies are extracted once (crossplay.extract) and handed to
    stationary.run (start="reset", tol, max_iters) and to this call alike; a game whose stationary iteration stopped at
    its step limit starts from its last iterate all the same, and a game that iteration did not solve is not solved
    here.  The rows are produced in tau-chunks of at most `budget` bytes per device buffer.  Returns a dict of numpy
    arrays."""
    import torch
    from . import stationary as sn
    from .attractors import policy_entries
    N = batch.N
    G = an.games(batch, n_games, "deviation_noise")
    K, L = int(steps), int(dev_len)
    if not 0 <= int(deviator) < N:
        raise ThrlError("deviator %d out of [0, %d)" % (int(deviator), N))
    if group_stats is not None and group_stats.G != G:
        raise ThrlError("group_stats spec is for %d games, this call has %d" % (group_stats.G, G))
    dev = batch.device
    given = policy is not None
    P = policy_entries(batch)
    if given:
        an.check_policy(batch, policy, (G, P), "deviation_noise", more_games=True)
    else:
        q = an.tables_tensor(batch, q, "deviation_noise")
    if tabs is None:
        tabs = sn.tables(batch.config)
    J, T, W = int(tabs["n_cells"]), int(tabs["n_tuples"]), int(tabs["band_w"])
    a = _lib.DeviationNoiseArgs()
    a.n_games, a.n_cells, a.band_w = G, J, W
    a.deviator, a.dev_len, a.n_steps, a.dev_action = int(deviator), L, K, action_index(action)
    a.ret_tol = float(ret_tol)
    nt = ctypes.c_int32(-1)
    a.n_tuples = ctypes.pointer(nt)
    with torch.cuda.device(dev):
        p, p_g = sn.resolve_noise(batch, noise_prob, G)
        stat_iters = np.zeros(G, np.int32)
        if isinstance(weights, str):
            if weights != "stationary":
                raise ThrlError("deviation_noise: weights must be 'stationary' or a [G, J] array, got %r" % (weights,))
            if not given:       # one extraction serves both calls, which then read the same policies
                from .crossplay import extract
                policy, given = extract(batch, q), True
            st = sn.run(batch, noise_prob=noise_prob, start="reset", tol=tol, max_iters=max_iters, pi=True, policy=policy,
                        n_games=G, tabs=tabs)
            m0 = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
            stat_iters = np.asarray(st["iters"], np.int32)
        else:
            if weights is None:
                raise ThrlError("deviation_noise: weights must be 'stationary' or a [G, J] array, got None")
            if isinstance(weights, torch.Tensor):
                m0 = weights.to(device=dev, dtype=torch.float64).contiguous()
            else:
                m0 = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, np.float64))).to(dev)
            if tuple(m0.shape) != (G, J):
                raise ThrlError("deviation_noise: weights must be shaped %s, got %s" % ((G, J), tuple(m0.shape)))
        a.flags = _lib.STAT_POLICY_GIVEN if given else 0
        if not given:
            policy = torch.empty((G, P), dtype=torch.int16, device=dev)
        keep = an.bind_tables(a, tabs, [("cell_rows", (N, J), np.int32), ("det_cell", (T,), np.int32),
                                        ("band_lo", (T,), np.int32), ("band", (T, W), np.float64),
                                        ("noise_reward", (N, T), np.float64)], dev, "deviation_noise")
        if p_g is not None:
            a.noise_prob_g = p_g.data_ptr()
        else:
            a.noise_prob = p
        gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
        if gam is not None:
            gam = gam[:, :G].contiguous()
            a.sweep_gamma = gam.data_ptr()
        a.policy = policy.data_ptr()
        a.weights = m0.data_ptr()
        out = an.outputs(dev, (NOISE_AGENT, (N, G), "float64"), (NOISE_FLOAT, (G,), "float64"), (NOISE_INT, (G,), "int32"))
        an.bind(a, out)
        want = bool(rows) or group_stats is not None
        chunk = max(1, min(K, int(budget) // (8 * N * G))) if want else K
        st = group_stats.zeros(K, dev) if group_stats is not None else None
        host_r, host_a, host_d = [], [], []
        b0 = 0
        while True:
            k = min(chunk, K - b0) if want else 0
            rr = ra = rd = None
            if k:
                rr = torch.empty((k, N, G), dtype=torch.float64, device=dev)
                ra = torch.empty((k, N, G), dtype=torch.float64, device=dev)
                rd = torch.empty((k, G), dtype=torch.float64, device=dev) if rows else None
            a.row_begin, a.row_count = b0, k
            a.reward_rows = rr.data_ptr() if rr is not None else None
            a.action_rows = ra.data_ptr() if ra is not None else None
            a.dist_rows = rd.data_ptr() if rd is not None else None
            rc = batch.L.thrl_deviation_noise(ctypes.byref(batch.cfg), None if given else q.data_ptr(), ctypes.byref(a),
                                              batch._stream())
            if nt.value >= 0 and nt.value != T:
                raise ThrlError("deviation_noise: the tables hold %d action tuples, the batch's config has %d" % (T, nt.value))
            _lib.check(rc, "thrl_deviation_noise")
            a.flags, given = _lib.STAT_POLICY_GIVEN, True       # later chunks work from the policies of the first
            if st is not None and k:
                group_stats.reduce(batch.L, rr, ra, k, st, batch._stream(), at=b0)
            if rows and k:
                host_r.append(rr.cpu().numpy())
                host_a.append(ra.cpu().numpy())
                host_d.append(rd.cpu().numpy())
            b0 += k
            if b0 >= K or not want:
                break
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["noise_prob"] = np.full(G, p, np.float64) if p_g is None else p_g.cpu().numpy()
        if rows:
            res["reward_rows"] = np.concatenate(host_r, axis=0)
            res["action_rows"] = np.concatenate(host_a, axis=0)
            res["dist_rows"] = np.concatenate(host_d, axis=0)
        if st is not None:
            from .group_stats import to_numpy
            res["group_stats"] = to_numpy(st)
    res["stat_iters"], res["n_cells"], res["ret_tol"] = stat_iters, J, float(ret_tol)
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


def solved_noise(games):
    """bool [G]: the games thrl_deviation_noise solved, those with a noise probability in (0, 1]."""
    p = np.asarray(games["noise_prob"], np.float64)
    with np.errstate(invalid="ignore"):
        return (p > 0.0) & (p <= 1.0)


def summarize_noise(games, ids, n_groups, deviators):
    """The summary rows of the test under noise, one per (group, deviator): games[d] = the dict of per-game arrays of
    deviator d (run_noise / load_noise_games) in global game order, ids = group id per game.  Every statistic but
    `games` is over the solved games (solved_noise): solved (their number), deviates (the share with dev_share > 0),
    dev_share_mean, unprofitable (the share with gain < 0), gain_mean, gain_q25 / q50 / q75, gain_dev_mean, low_mean,
    returned (the share with ret_step >= 0), ret_step_mean over those, dist_mean."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    out = []
    for k in range(int(n_groups)):
        for d in deviators:
            g = games[d]
            m = (ids == k) & solved_noise(g)
            f = {name: np.asarray(g[name], np.float64)[m] for name in NOISE_FLOAT}
            ret = np.asarray(g["ret_step"])[m]
            row = {"group": k, "deviator": int(d), "games": int(np.sum(ids == k)), "solved": int(m.sum()),
                   "deviates": an.frac(f["dev_share"] > 0), "dev_share_mean": an.mean(f["dev_share"]),
                   "unprofitable": an.frac(f["gain"] < 0), "gain_mean": an.mean(f["gain"])}
            an.quantiles(row, "gain", f["gain"])
            row.update(gain_dev_mean=an.mean(f["gain_dev"]), low_mean=an.mean(f["low"]), returned=an.frac(ret >= 0),
                       ret_step_mean=an.mean(ret[ret >= 0]), dist_mean=an.mean(f["dist"]))
            out.append(row)
    return out


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis."""
    return an.combine(parts)


def describe(options, nash, cartel, summary):
    """deviation.json's content (without the option "noise": the file is what it is without that option)."""
    options = {k: v for k, v in options.items() if k != "noise"}
    return {"options": options, "nash": nash, "cartel": cartel, "lam_bins": lam_bin_names(),
            "quantiles": list(QUANTILES), "summary": summary}


def describe_noise(options, n_cells, summary):
    """deviation_noise.json's content."""
    return {"options": options, "n_cells": int(n_cells), "quantiles": list(QUANTILES), "summary": summary}


# ---------------------------------------------------------------------------------------------- artefacts
def load_games(d, deviator):
    """The per-game arrays one run directory (or shard) holds for `deviator`."""
    cyc = np.load(os.path.join(d, "dev_cycle.npy"))
    post = np.load(os.path.join(d, "dev%d_post.npy" % deviator))
    return {"mu": cyc[0], "lam": cyc[1], "mu_post": post[0], "lam_post": post[1], "ret_step": post[2],
            "act_dev": post[3], "gain": np.load(os.path.join(d, "dev%d_gain.npy" % deviator)),
            "cycle_reward": np.load(os.path.join(d, "dev_cycle_reward.npy")),
            "cycle_action": np.load(os.path.join(d, "dev_cycle_action.npy"))}


def save_noise_games(d, deviator, r):
    """devn<d>_games float64 [6, G] (dev_share, gain, gain_dev, low, dist, mass), devn<d>_steps int32 [2, G] (low_step,
    ret_step), devn<d>_base float64 [2, N, G] (base_reward, base_action); devn_prob [G] (the noise probabilities
    analysed) and devn_stat_iters int32 [G] (the stationary iteration behind the weights) are the same for every
    deviator."""
    np.save(os.path.join(d, "devn%d_games.npy" % deviator), np.stack([r[f] for f in NOISE_FLOAT]).astype(np.float64))
    np.save(os.path.join(d, "devn%d_steps.npy" % deviator), np.stack([r[f] for f in NOISE_INT]).astype(np.int32))
    np.save(os.path.join(d, "devn%d_base.npy" % deviator), np.stack([r[f] for f in NOISE_AGENT]).astype(np.float64))
    np.save(os.path.join(d, "devn_prob.npy"), np.asarray(r["noise_prob"], np.float64))
    np.save(os.path.join(d, "devn_stat_iters.npy"), np.asarray(r["stat_iters"], np.int32))


def load_noise_games(d, deviator):
    """The per-game arrays of the test under noise one run directory (or shard) holds for `deviator`."""
    gm = np.load(os.path.join(d, "devn%d_games.npy" % deviator))
    st = np.load(os.path.join(d, "devn%d_steps.npy" % deviator))
    base = np.load(os.path.join(d, "devn%d_base.npy" % deviator))
    g = {f: gm[k] for k, f in enumerate(NOISE_FLOAT)}
    g.update({f: st[k] for k, f in enumerate(NOISE_INT)})
    g.update({f: base[k] for k, f in enumerate(NOISE_AGENT)})
    g["noise_prob"] = np.load(os.path.join(d, "devn_prob.npy"))
    g["stat_iters"] = np.load(os.path.join(d, "devn_stat_iters.npy"))
    return g


def merged(shards, out, config, opt, ids, n_groups, first):
    """deviation.json of a sharded run (launch.merge_analysis): per deviator the shards' arrays concatenated in global
    game order and summarised as one run; with the option "noise" devn_*.npy and deviation_noise.json the same way."""
    nash, cartel = optimal(config)
    summary = []
    for d in opt["agents"]:
        summary += summarize(combine(load_games(s, d) for s in shards), ids, n_groups, nash, cartel, d)
    if opt.get("noise"):
        games = {d: combine(load_noise_games(s, d) for s in shards) for d in opt["agents"]}
        for d in opt["agents"]:
            save_noise_games(out, d, games[d])
        with open(os.path.join(shards[0], "deviation_noise.json")) as f:
            n_cells = json.load(f)["n_cells"]
        save_json(os.path.join(out, "deviation_noise.json"),
                  describe_noise(opt, n_cells, summarize_noise(games, ids, n_groups, opt["agents"])))
    return describe(opt, nash, cartel, summary)


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, spec=None, histograms=False, budget=ROW_BUDGET,
                    q=None, state0=None):
    """train_one's training.deviation outputs: the per-game .npy files, dev<d>_*.npy group statistics with a spec,
    and deviation.json, and with the option "noise" the test under demand noise after them (devn_*.npy, devn<d>_*.npy
    with the response curves' group statistics under the same prefix, deviation_noise.json).  q / state0 (device
    tensors): the tables and start prices analysed in place of the batch's (opt["tables"] == "converged")."""
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
    if opt.get("noise"):
        nz = opt["noise"]
        games = {}
        for d in opt["agents"]:
            games[d] = run_noise(batch, deviator=d, steps=opt["steps"], dev_len=opt["dev_len"], action=opt["action"],
                                 noise_prob=nz["noise_prob"], ret_tol=nz["ret_tol"], group_stats=spec, budget=budget, q=q,
                                 tol=nz["tol"], max_iters=nz["max_iters"])
            save_noise_games(exp_path, d, games[d])
            if spec is not None:
                trainer.save_group_stats(exp_path, "devn%d" % d, games[d]["group_stats"], spec, histograms)
        save_json(os.path.join(exp_path, "deviation_noise.json"),
                  describe_noise(opt, games[opt["agents"][0]]["n_cells"], summarize_noise(games, ids, n_groups, opt["agents"])))
