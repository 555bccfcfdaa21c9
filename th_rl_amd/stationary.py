"""Greedy play under demand noise (thrl_stationary, include/thrl.h): the exact long-run profit of trained QTable games
in the environment the reference ships.  NoisyPriceState(noise_prob=0.05) redraws the demand intercept from
U(0.7 a, a) with that probability at every step, and the reference's evaluation plots (utils.play_game) step through
that environment.  The deviation, equilibrium, cross-play and attractor analyses describe the noise-free greedy map,
which usually has several limit cycles; a demand shock moves a game from one to another, so what greedy play sustains
in the long run belongs to no single cycle.  With the price axis cut at the agents' encode breakpoints (attractors.
starts) noisy greedy play is a finite Markov chain per game, and the kernel iterates it in its lazy form from the
environment's reset distribution (or from the training state); no sampling, no transient, no sampling error.

Per game (definitions in include/thrl.h): iters, change, mass [G], stat_reward, stat_action [N, G], stat_price [G],
optionally pi [G, J].  tables() derives the per-config tables in numpy; the device only reads them.  summarize() gives,
per group:

    games, converged (share of games with 0 <= iters < max_iters), iters_q25 / q50 / q75 / max
    delta_noise_mean, delta_noise_q25 / q50 / q75   deviation.profit_gain of stat_reward against deviation.optimal(config),
                         the NOISE-FREE Nash and Cartel rewards (the benchmark of every other analysis here)
    price_mean           mean stat_price
    delta_reset_mean     the attractor analysis's noise-free reset-expected gain, and
    noise_cost_mean      mean of (delta_reset - delta_noise): both only when the attractor analysis's reset_reward is given

Games that were not solved (iters = -1) count as games and enter no other statistic.  Statistics that have no games
are None.  Shards combine exactly: their per-game arrays are concatenated in global game order (combine) and
summarised as one run.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from . import tuple_play as tp
from ._lib import ThrlError
from .analysis import QUANTILES, save_json  # noqa: F401  (sn.save_json stays a public name)
from .attractors import encode64, policy_entries, starts
from .deviation import optimal, profit_gain

DEFAULTS = dict(noise_prob=None, start="reset", tol=1e-12, max_iters=8192, pi=False)
STARTS = ("reset", "state")
GAME_FLOAT = ("change", "mass", "stat_price")
AGENT_FLOAT = ("stat_reward", "stat_action")
NEURAL_FOLLOW_UP = ("the stationary analysis runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def check_config(config):
    """ValueError for a config with neural agents (the analysis needs every agent's greedy table)."""
    an.check_qtable_only(config, "stationary", NEURAL_FOLLOW_UP)


def check_prob(p, what):
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 < float(p) <= 1.0:
        raise ValueError("%s must be a number in (0, 1], got %r" % (what, p))
    return float(p)


def parse_options(opt, config):
    """training.stationary (true or a dict) -> the dict with every key filled in: noise_prob (None = the run's own),
    start ('reset' or 'state'), tol, max_iters, pi (store the distributions), and tables when given."""
    check_config(config)
    out = an.options("stationary", opt, DEFAULTS, tables=True)
    if out["noise_prob"] is not None:
        out["noise_prob"] = check_prob(out["noise_prob"], "training.stationary.noise_prob")
    else:
        an.check_own_noise(config, "training.stationary")
    an.chain_options(out, "training.stationary", STARTS)
    return out


# ---------------------------------------------------------------------------------------------- the per-config tables
def breakpoints(config):
    """The arrays the price axis is cut at: [0, a] and, per QTable agent, its encode breakpoints inside (0, a)."""
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    a = float(env["a"])
    parts = [np.array([0.0, a])]
    for ag in config["agents"]:
        if ag.get("name", "QTable") != "QTable":
            continue
        p = dict(_lib.QTABLE_DEFAULTS, **ag)
        n, ms = int(p["states"]), float(p["max_state"])
        b = (np.arange(n, dtype=np.float64) + 0.5) * ms / float(n)
        parts.append(b[(b > 0.0) & (b < a)])
    return parts


def cuts(config):
    """c float64 [J + 1]: the ends of the cells of attractors.starts(config), cell k = [c[k], c[k + 1])."""
    return np.unique(np.concatenate(breakpoints(config)))


def tuple_steps(config, t=None):
    """The env step of every action tuple (agent 0 slowest), operation for operation the device's scale_action and
    env_step, from tuple_play.tables(config) (t): (quantity [N, T] = ratio * scaled action, u [T] = the amount subtracted
    from the intercept, price [T] = the noise-free price, scaled [N, T])."""
    t = tp.tables(config) if t is None else t
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    a, b = float(env["a"]), float(env["b"])
    quantity = (a / b) * t["scaled"]
    total = np.zeros(t["T"], np.float64)
    for qn in quantity:
        total = total + qn
    return quantity, b * total, t["price"], t["scaled"]


def noise_geometry(config, t, c):
    """What the redrawn price of every tuple covers of the cells with the ends c: dict(length [T, J], the length of
    [0.7 a - u(t), a - u(t)) inside each cell; z [T], the length clipped to price 0; width = 0.3 a; noise_price [T];
    quantity [N, T]; cell_w and cell_x [J]).  tables() and tuple_stationary.tables() lump z into cell 0;
    sampled_play.noise_tables gives it a node of its own."""
    quantity, u, _, _ = tuple_steps(config, t)
    a = float(dict(_lib.ENV_DEFAULTS, **config["environment"])["a"])
    w = (c[1:] - c[:-1]) / a
    x = 0.5 * (c[:-1] + c[1:])
    noise_lo = a * 0.7
    lo, hi, width = noise_lo - u, a - u, a - noise_lo
    length = np.maximum(0.0, np.minimum(c[None, 1:], hi[:, None]) - np.maximum(c[None, :-1], lo[:, None]))
    z = np.maximum(0.0, -lo) - np.maximum(0.0, -hi)
    nprice = np.where(lo >= 0.0, (lo + hi) / 2.0, np.where(hi <= 0.0, 0.0, hi * hi / (2.0 * width)))
    return dict(length=length, z=z, width=width, noise_price=nprice, quantity=quantity, cell_w=w, cell_x=x, u=u, a=a)


def band_of(n):
    """(band_lo int32 [T], band [T, W]) of the weights n [T, J]: every row from its first to its last non-zero entry,
    padded with zeros to the widest."""
    T, J = n.shape
    nz = n > 0.0
    first = np.where(nz.any(axis=1), nz.argmax(axis=1), 0)
    last = np.where(nz.any(axis=1), J - 1 - nz[:, ::-1].argmax(axis=1), 0)
    W = int((last - first + 1).max())
    pad = np.concatenate([n, np.zeros((T, W))], axis=1)
    band = pad[np.arange(T)[:, None], first[:, None] + np.arange(W)[None, :]]
    return first.astype(np.int32), np.ascontiguousarray(band, np.float64)


def tables(config):
    """The per-config tables of thrl_stationary (include/thrl.h "Per-config tables") as a dict of numpy arrays:
    cell_rows int32 [N, J] and cell_w [J] (attractors.starts), det_cell int32 [T], band_lo int32 [T], band [T, W],
    noise_reward [N, T], noise_price [T], and n_cells, n_intervals, n_tuples, band_w.

    The first n_intervals cells are the intervals of attractors.starts.  A noise-free price that sits exactly on a
    breakpoint where the agents' half-even ties disagree (agent 0 rounds down, agent 1 up) has a row tuple that no
    interval has; the deterministic map still goes there, so every such row tuple is appended as a POINT CELL: its
    rows, weight 0 in the reset distribution, and no band entry, since a redrawn intercept lands on a single price
    with probability 0.  That keeps the chain's noise-free part identical to thrl_deviation's F on every config (the
    headline config has no point cell; three agents with grids of 30, 60 and 40 states have some)."""
    check_config(config)
    rows, w = starts(config)
    c = cuts(config)
    Ji = int(w.size)
    if c.size != Ji + 1:
        raise ValueError("stationary: %d cell ends for %d cells" % (c.size, Ji))
    ps = [dict(_lib.QTABLE_DEFAULTS, **ag) for ag in config["agents"]]
    t = tp.tables(config)
    price, T = t["price"], int(t["T"])
    # det_cell: the cell with the row tuple of the noise-free price; a row tuple that no interval has becomes a point cell
    cell_of = {tuple(int(v) for v in rows[:, k]): k for k in range(Ji)}
    prow = np.stack([encode64(price, int(p["states"]), float(p["max_state"])) for p in ps])
    det = np.zeros(T, np.int32)
    points = []
    for k in range(T):
        key = tuple(int(v) for v in prow[:, k])
        if key not in cell_of:
            cell_of[key] = Ji + len(points)
            points.append(key)
        det[k] = cell_of[key]
    J = Ji + len(points)
    if points:
        rows = np.concatenate([rows, np.array(points, np.int32).T], axis=1)
        w = np.concatenate([w, np.zeros(len(points))])
    if J > _lib.STAT_MAX_CELLS:
        raise ValueError("stationary: %d cells, at most %d" % (J, _lib.STAT_MAX_CELLS))
    # band: where a redrawn intercept puts the price; no intercept lands on a point cell
    geo = noise_geometry(config, t, c)
    length, nprice = geo["length"], geo["noise_price"]
    length[:, 0] = length[:, 0] + geo["z"]
    first, band = band_of(np.concatenate([length / geo["width"], np.zeros((T, J - Ji))], axis=1))
    return dict(cell_rows=np.ascontiguousarray(rows, np.int32), cell_w=np.ascontiguousarray(w, np.float64),
                det_cell=det, band_lo=first, band=band,
                noise_reward=np.ascontiguousarray(nprice[None, :] * geo["quantity"]), noise_price=np.ascontiguousarray(nprice),
                n_cells=J, n_intervals=Ji, n_tuples=T, band_w=int(band.shape[1]))


# ---------------------------------------------------------------------------------------------- the device call
def resolve_noise(batch, noise_prob, G):
    """analysis.resolve_noise for GameBatch.stationary's noise_prob argument: a number lies in (0, 1]."""
    return an.resolve_noise(batch, noise_prob, G, "stationary")


def run(batch, noise_prob=None, start="reset", state0=None, tol=1e-12, max_iters=8192, pi=False, q=None, policy=None,
        n_games=None, tabs=None):
    """thrl_stationary for the first n_games (default all) games of `batch` (a GameBatch or an all-QTable
    MixedGameBatch; see GameBatch.stationary).  tabs: tables(batch.config), or a dict that replaces some of them.
    Returns a dict of numpy arrays."""
    import torch
    N = batch.N
    G = an.games(batch, n_games, "stationary")
    if start not in STARTS:
        raise ThrlError("stationary: start must be one of %s, got %r" % (STARTS, start))
    dev = batch.device
    given = policy is not None
    P = policy_entries(batch)
    if given:
        an.check_policy(batch, policy, (G, P), "stationary", more_games=True)
    else:
        q = an.tables_tensor(batch, q, "stationary")
    if tabs is None:
        tabs = tables(batch.config)
    J, T, W = int(tabs["n_cells"]), int(tabs["n_tuples"]), int(tabs["band_w"])
    a = _lib.StationaryArgs()
    a.n_games, a.n_cells, a.band_w, a.max_iters, a.tol = G, J, W, int(max_iters), float(tol)
    a.flags = (_lib.STAT_POLICY_GIVEN if given else 0) | (_lib.STAT_START_STATE if start == "state" else 0)
    nt = ctypes.c_int32(-1)
    a.n_tuples = ctypes.pointer(nt)
    with torch.cuda.device(dev):
        p, p_g = resolve_noise(batch, noise_prob, G)
        keep = an.bind_tables(a, tabs, [("cell_rows", (N, J), np.int32), ("cell_w", (J,), np.float64),
                                        ("det_cell", (T,), np.int32), ("band_lo", (T,), np.int32),
                                        ("band", (T, W), np.float64), ("noise_reward", (N, T), np.float64),
                                        ("noise_price", (T,), np.float64)], dev, "stationary")
        if p_g is not None:
            a.noise_prob_g = p_g.data_ptr()
        else:
            a.noise_prob = p
        if start == "state":
            s0 = an.state0_tensor(batch, state0, G, "stationary")
            a.state0 = s0.data_ptr()
        if not given:
            policy = torch.empty((G, P), dtype=torch.int16, device=dev)
        a.policy = policy.data_ptr()
        out = an.outputs(dev, (("iters",), (G,), "int32"), (GAME_FLOAT, (G,), "float64"), (AGENT_FLOAT, (N, G), "float64"),
                         (("pi",) if pi else (), (G, J), "float64"))
        an.bind(a, out)
        rc = batch.L.thrl_stationary(ctypes.byref(batch.cfg), None if given else q.data_ptr(), ctypes.byref(a),
                                     batch._stream())
        if nt.value >= 0 and nt.value != T:
            raise ThrlError("stationary: the tables hold %d action tuples, the batch's config has %d" % (T, nt.value))
        _lib.check(rc, "thrl_stationary")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["noise_prob"] = np.full(G, p, np.float64) if p_g is None else p_g.cpu().numpy()
    res["n_cells"], res["max_iters"] = J, int(max_iters)
    return res


# ---------------------------------------------------------------------------------------------- host side
def summarize(games, ids, n_groups, nash, cartel, max_iters, reset_reward=None):
    """The summary rows, one per group.  games = dict of per-game arrays in global game order, ids = group id per
    game, reset_reward [N, G] = the attractor analysis's, when the run has one."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    iters = np.asarray(games["iters"], np.int64)
    solved = iters >= 0
    delta = profit_gain(np.asarray(games["stat_reward"], np.float64), nash, cartel)
    price = np.asarray(games["stat_price"], np.float64)
    dreset = None if reset_reward is None else profit_gain(np.asarray(reset_reward, np.float64), nash, cartel)
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        ms = m & solved
        row = {"group": k, "games": int(m.sum()),
               "converged": an.mean(solved[m] & (iters[m] < int(max_iters))) if m.any() else None}
        an.quantiles(row, "iters", iters[ms])
        row["iters_max"] = int(iters[ms].max()) if ms.any() else None
        row["delta_noise_mean"] = an.mean(delta[ms])
        an.quantiles(row, "delta_noise", delta[ms])
        row["price_mean"] = an.mean(price[ms])
        if dreset is not None:
            row["delta_reset_mean"] = an.mean(dreset[ms])
            row["noise_cost_mean"] = an.mean(dreset[ms] - delta[ms])
        out.append(row)
    return out


PER_GAME = ("iters", "noise_prob") + GAME_FLOAT + AGENT_FLOAT + ("pi",)


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis (axis
    0 of pi [G, J], the last axis of the others)."""
    return an.combine(parts, other={"pi": 0}, only=PER_GAME)


def describe(options, n_cells, nash, cartel, summary):
    """stationary.json's content."""
    return {"options": options, "n_cells": int(n_cells), "nash": nash, "cartel": cartel, "quantiles": list(QUANTILES),
            "benchmark": "noise-free Nash and Cartel rewards (environment.get_optimal)", "summary": summary}


# ---------------------------------------------------------------------------------------------- artefacts
def save_games(d, r):
    """stat_iters int32 [G], stat_games float64 [4, G] (change, mass, stat_price, noise_prob), stat_reward and
    stat_action float64 [N, G]; with the distributions stat_pi float64 [G, J]."""
    np.save(os.path.join(d, "stat_iters.npy"), np.asarray(r["iters"], np.int32))
    np.save(os.path.join(d, "stat_games.npy"),
            np.stack([np.asarray(r[f], np.float64) for f in GAME_FLOAT + ("noise_prob",)]))
    for f in AGENT_FLOAT:
        np.save(os.path.join(d, "%s.npy" % f), np.asarray(r[f], np.float64))
    if "pi" in r:
        np.save(os.path.join(d, "stat_pi.npy"), np.asarray(r["pi"], np.float64))


def load_games(d):
    """The per-game arrays one run directory (or shard) holds."""
    gm = np.load(os.path.join(d, "stat_games.npy"))
    g = {"iters": np.load(os.path.join(d, "stat_iters.npy"))}
    g.update({f: gm[k] for k, f in enumerate(GAME_FLOAT + ("noise_prob",))})
    g.update({f: np.load(os.path.join(d, "%s.npy" % f)) for f in AGENT_FLOAT})
    if os.path.isfile(os.path.join(d, "stat_pi.npy")):
        g["pi"] = np.load(os.path.join(d, "stat_pi.npy"))
    return g


def reset_reward_of(d, n_games=None):
    """The attractor analysis's reset_reward [N, G] of the same directory, or None when there is none or (n_games
    given) it holds another number of games: a file left by an earlier run."""
    path = os.path.join(d, "attr_reset_reward.npy")
    if not os.path.isfile(path):
        return None
    rr = np.load(path)
    return rr if n_games is None or (rr.ndim == 2 and rr.shape[1] == int(n_games)) else None


def merged(shards, out, config, opt, ids, n_groups, first):
    """stationary.json and stat_*.npy of a sharded run (launch.merge_analysis); delta_reset_mean and noise_cost_mean
    from the attractor analysis's merged reset_reward in `out`, which that key's merge wrote before."""
    games = combine(load_games(s) for s in shards)
    save_games(out, games)
    nash, cartel = optimal(config)
    rr = reset_reward_of(out, len(ids)) if an.enabled(config.get("training", {}), "attractors") else None
    summary = summarize(games, ids, n_groups, nash, cartel, opt["max_iters"], reset_reward=rr)
    return describe(opt, first["n_cells"], nash, cartel, summary)


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, q=None, state0=None, with_attractors=False):
    """train_one's training.stationary outputs: the per-game stat_*.npy files and stationary.json.  q / state0 (device
    tensors): the tables and training states analysed in place of the batch's (opt["tables"] == "converged").
    with_attractors: this run wrote attr_reset_reward.npy (training.attractors) just before; only then does the
    summary carry delta_reset_mean and noise_cost_mean."""
    r = run(batch, noise_prob=opt["noise_prob"], start=opt["start"], state0=state0, tol=opt["tol"],
            max_iters=opt["max_iters"], pi=opt["pi"], q=q)
    save_games(exp_path, r)
    nash, cartel = optimal(config)
    rr = reset_reward_of(exp_path, np.asarray(r["iters"]).size) if with_attractors else None
    summary = summarize(r, ids, n_groups, nash, cartel, opt["max_iters"], reset_reward=rr)
    save_json(os.path.join(exp_path, "stationary.json"), describe(opt, r["n_cells"], nash, cartel, summary))
