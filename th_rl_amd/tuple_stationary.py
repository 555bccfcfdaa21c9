"""Greedy play under demand noise for games whose agents may be networks (thrl_price_policy, thrl_tuple_stationary,
include/thrl.h): stationary.py for any mix of QTable, Reinforce and ActorCritic agents: the exact long-run profit of
greedy play in the environment the reference ships, NoisyPriceState(noise_prob=0.05).

Under noise the next price is no tuple's price, but its distribution depends only on the tuple just played: with
probability 1 - p the tuple's noise-free price, with probability p uniform on [0.7 a - u(t), a - u(t)], clipped at 0.  So
the distribution over the tuple played at a step is a Markov chain on the game's T action tuples (tuple_play.py).  Beyond
the strategies in tuple form it needs every agent's greedy action as a function of the price on [0, a): a QTable's is
piecewise constant with known cuts; a network's is piecewise constant with unknown cuts and is sampled at the midpoints
of a per-config grid of cells (`resolution` uniform cuts beside the QTable agents' breakpoints).  The share of the price
axis on which that sampling may be wrong is reported per game: n_switch, the pairs of adjacent cells between which a
network's action changes, and unresolved, their share of the axis.  A strategy that switches twice between two adjacent
midpoints is not seen; a higher resolution is the remedy.

tables(config, resolution) derives the per-config tables in numpy; the device only reads them.  extract_cells() samples
the strategies at the cell midpoints, run() iterates the chain and returns per game (definitions in include/thrl.h)
iters, change, mass, stat_price, n_switch, unresolved [G], stat_reward, stat_action [N, G], optionally pi [G, T].
summarize() gives stationary.summarize's rows per group plus n_switch_max, unresolved_mean and unresolved_max.  Sharded
runs (th_rl_amd.launch) are refused.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from . import stationary as sn
from . import tuple_play as tp
from ._lib import ThrlError
from .deviation import optimal

DEFAULTS = dict(noise_prob=None, start="reset", tol=1e-12, max_iters=8192, pi=False, resolution=1024)
STARTS = sn.STARTS
MAX_CELLS = _lib.STAT_MAX_CELLS
GAME_FLOAT = sn.GAME_FLOAT + ("unresolved",)
AGENT_FLOAT = sn.AGENT_FLOAT
PER_GAME = ("iters", "n_switch", "noise_prob", "start") + GAME_FLOAT + AGENT_FLOAT + ("pi",)


def _check_resolution(r, what):
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) <= MAX_CELLS:
        raise ValueError("%s must be an integer in [0, %d], got %r" % (what, MAX_CELLS, r))
    return int(r)


def parse_options(opt, config):
    """training.greedy_stationary (true or a dict) -> the dict with every key filled in: noise_prob (None = the run's
    own), start ('reset' or 'state'), tol, max_iters, pi (store the distributions), resolution (uniform cuts of the price
    axis).  Refuses a CAC agent, more than tuple_play.MAX_TUPLES tuples and more than MAX_CELLS cells."""
    name = "training.greedy_stationary"
    tp.check_config(config)
    out = an.options("greedy_stationary", opt, DEFAULTS)
    if out["noise_prob"] is not None:
        out["noise_prob"] = sn.check_prob(out["noise_prob"], name + ".noise_prob")
    else:
        an.check_own_noise(config, name)
    an.chain_options(out, name, STARTS)
    out["resolution"] = _check_resolution(out["resolution"], name + ".resolution")
    try:
        cuts(config, out["resolution"])          # more than MAX_CELLS cells: refused before training
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e))
    return out


# ---------------------------------------------------------------------------------------------- the per-config tables
def cuts(config, resolution):
    """c float64 [J + 1]: the ends of the cells, cell k = [c[k], c[k + 1]): [0, a) cut at the encode breakpoints of the
    QTable agents (the construction of stationary.cuts) and at a * m / resolution, m = 1..resolution-1 (0 = none).  Two
    cuts so close that the midpoint between them rounds onto one of them (the same number reached by two roundings) are
    one cut: every midpoint lies strictly inside its cell."""
    resolution = _check_resolution(resolution, "resolution")
    parts = sn.breakpoints(config)
    a = float(parts[0][1])
    if resolution > 1:
        u = a * np.arange(1, resolution, dtype=np.float64) / float(resolution)
        parts.append(u[(u > 0.0) & (u < a)])
    c = np.unique(np.concatenate(parts))
    while True:
        x = 0.5 * (c[:-1] + c[1:])
        bad = np.flatnonzero(~((c[:-1] < x) & (x < c[1:])))
        if not bad.size:
            break
        k = int(bad[0])
        c = np.delete(c, k + 1 if k + 2 < c.size else k)
    if c.size - 1 > MAX_CELLS:
        raise ValueError("tuple_stationary: resolution=%d gives %d cells, at most %d" % (resolution, c.size - 1, MAX_CELLS))
    return c


noise_geometry, band_of = sn.noise_geometry, sn.band_of     # stationary.py holds the one copy; the names stay here


def tables(config, resolution=DEFAULTS["resolution"]):
    """The per-config tables of thrl_tuple_stationary (include/thrl.h) as a dict of numpy arrays: cuts [J + 1], cell_w
    [J] (length / a), cell_x [J] (the midpoints the strategies are sampled at); tuple_play.tables' T, n_actions, kinds,
    price [T], reward and scaled [N, T]; band_lo int32 [T], band [T, W], noise_price [T], noise_reward [N, T] by the
    formulas of thrl_stationary's tables over these cells; n_cells, n_tuples, band_w, resolution.  More than MAX_CELLS
    cells is a ValueError that names the resolution."""
    t = tp.tables(config)
    c = cuts(config, resolution)
    J = int(c.size - 1)
    geo = noise_geometry(config, t, c)
    length, width, w, x, nprice, quantity = (geo[f] for f in ("length", "width", "cell_w", "cell_x", "noise_price", "quantity"))
    length[:, 0] = length[:, 0] + geo["z"]
    n = length / width
    first, band = band_of(n)
    W = int(band.shape[1])
    out = dict(t)
    out.update(cuts=c, cell_w=np.ascontiguousarray(w), cell_x=np.ascontiguousarray(x), band_lo=first,
               band=band, noise_price=np.ascontiguousarray(nprice),
               noise_reward=np.ascontiguousarray(nprice[None, :] * quantity), n_cells=J, n_tuples=int(t["T"]), band_w=W,
               resolution=int(resolution))
    return out


# ---------------------------------------------------------------------------------------------- the device calls
def price_policy(batch, price, per_game=False, n_games=None):
    """thrl_price_policy: what every agent of the first n_games (default all) games of `batch` plays at the prices
    `price` (J numbers shared by the games, or with per_game [G, J]: each game its own), as a device int16 tensor
    [G, N, J] holding uint16 entries.  Nothing of the batch is written."""
    import torch
    kinds = tp._kinds(batch)
    if not getattr(batch, "initialized", True):
        raise ThrlError("tuple_stationary: call init_tables() or set_tables() first")
    G = an.games(batch, n_games, "tuple_stationary")
    dev = batch.device
    with torch.cuda.device(dev):
        if isinstance(price, torch.Tensor):
            x = price.to(device=dev, dtype=torch.float64).contiguous()
        else:
            x = torch.from_numpy(np.ascontiguousarray(price, np.float64)).to(dev)
        if per_game:
            x = x.reshape(x.shape[0], -1)[:G].contiguous()
            if x.shape[0] != G:
                raise ThrlError("tuple_stationary: per-game prices must hold %d rows" % G)
        else:
            x = x.reshape(-1)
        J = int(x.shape[-1])
        pol = torch.empty((G, batch.N, J), dtype=torch.int16, device=dev)
        a = _lib.PricePolicyArgs()
        a.n_games, a.n_prices, a.flags = G, J, _lib.PP_PER_GAME if per_game else 0
        for i, k in enumerate(kinds):
            a.kind[i] = tp.KINDS[k]
            if k != "QTable":
                a.nn_params[i] = batch.nn[i].params.data_ptr()
        a.price, a.price_policy = x.data_ptr(), pol.data_ptr()
        q = batch.q.data_ptr() if "QTable" in kinds else None
        _lib.check(batch.L.thrl_price_policy(ctypes.byref(batch.cfg), q, ctypes.byref(a), batch._stream()),
                   "thrl_price_policy")
        torch.cuda.synchronize(dev)
    return pol


def extract_cells(batch, tabs, n_games=None):
    """The strategies of `batch` sampled at the cell midpoints of `tabs`: device int16 [G, N, J] (thrl_price_policy)."""
    return price_policy(batch, tabs["cell_x"], n_games=n_games)


def state_tuples(batch, tabs, n_games=None):
    """int32 [G] (device): the tuple every game plays at the state it holds: the strategies evaluated at batch.state
    through thrl_price_policy's per-game mode."""
    import torch
    G = batch.G if n_games is None else int(n_games)
    pol = price_policy(batch, batch.state[:G].reshape(G, 1), per_game=True, n_games=G)
    e = (pol.reshape(G, batch.N).to(torch.int32) & 0xffff)
    nact = torch.from_numpy(np.asarray(tabs["n_actions"], np.int32)).to(e.device)
    stride = np.concatenate([np.cumprod(np.asarray(tabs["n_actions"], np.int64)[::-1])[::-1][1:], [1]]).astype(np.int32)
    t = (torch.minimum(e, nact[None, :] - 1) * torch.from_numpy(stride).to(e.device)[None, :]).sum(dim=1)
    return t.to(torch.int32).contiguous()


def run(batch, noise_prob=None, start="reset", resolution=DEFAULTS["resolution"], tol=1e-12, max_iters=8192, pi=False,
        tuple_policy=None, cell_policy=None, n_games=None, tabs=None):
    """thrl_tuple_stationary for the first n_games (default all) games of `batch` (a MixedGameBatch of QTable / Reinforce
    / ActorCritic agents, or a GameBatch).  noise_prob: stationary.resolve_noise's rules (None = the batch's per-game
    sweep array, else the config's value; 0 asks for an explicit one).  start: "reset" (a uniform price on [0, a)),
    "state" (the tuple played at batch.state), or int [G] start tuples (outside [0, T): that game is refused with
    iters = -1).  tuple_policy / cell_policy: the strategies of tuple_play.extract() / extract_cells() (default:
    extracted here).  tabs: tables(batch.config, resolution).  Returns a dict of numpy arrays."""
    import torch
    N = batch.N
    G = an.games(batch, n_games, "tuple_stationary")
    given_start = not isinstance(start, str)
    if not given_start and start not in STARTS:
        raise ThrlError("tuple_stationary: start must be one of %s or an array of tuples, got %r" % (STARTS, start))
    if tabs is None:
        tabs = tables(batch.config, resolution)
    tp._batch_tables(batch, tabs)
    dev = batch.device
    J, T, W = int(tabs["n_cells"]), int(tabs["n_tuples"]), int(tabs["band_w"])
    sdev = batch.state.device
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    if not an.is_policy(tuple_policy, (batch.G, N, T), sdev):
        an.check_policy(batch, tuple_policy, (G, N, T), "tuple_stationary", "tuple_policy")
    if cell_policy is None:
        cell_policy = extract_cells(batch, tabs, n_games=G)
    an.check_policy(batch, cell_policy, (G, N, J), "tuple_stationary", "cell_policy")
    a = _lib.TupleStationaryArgs()
    a.n_games, a.n_tuples, a.n_cells, a.band_w, a.max_iters, a.tol = G, T, J, W, int(max_iters), float(tol)
    for i, k in enumerate(tp._kinds(batch)):
        a.kind[i] = tp.KINDS[k]
    with torch.cuda.device(dev):
        p, p_g = sn.resolve_noise(batch, noise_prob, G)
        keep = an.bind_tables(a, tabs, [("cell_w", (J,), np.float64), ("reward", (N, T), np.float64),
                                        ("scaled", (N, T), np.float64), ("price", (T,), np.float64),
                                        ("band_lo", (T,), np.int32), ("band", (T, W), np.float64),
                                        ("noise_reward", (N, T), np.float64), ("noise_price", (T,), np.float64)],
                              dev, "tuple_stationary")
        if p_g is not None:
            a.noise_prob_g = p_g.data_ptr()
        else:
            a.noise_prob = p
        t0 = None
        if given_start:
            t0 = an.start_tensor(start, G, dev, "tuple_stationary")
        elif start == "state":
            t0 = state_tuples(batch, tabs, n_games=G)
        if t0 is not None:
            a.flags = _lib.TS_START_TUPLE
            a.start = t0.data_ptr()
        a.tuple_policy, a.cell_policy = tuple_policy.data_ptr(), cell_policy.data_ptr()
        out = an.outputs(dev, (("iters", "n_switch"), (G,), "int32"), (GAME_FLOAT, (G,), "float64"),
                         (AGENT_FLOAT, (N, G), "float64"), (("pi",) if pi else (), (G, T), "float64"))
        an.bind(a, out)
        _lib.check(batch.L.thrl_tuple_stationary(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                   "thrl_tuple_stationary")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["noise_prob"] = np.full(G, p, np.float64) if p_g is None else p_g.cpu().numpy()
        if t0 is not None:
            res["start"] = t0.cpu().numpy()
    res["n_cells"], res["T"], res["max_iters"], res["resolution"] = J, T, int(max_iters), int(tabs.get("resolution", resolution))
    return res


# ---------------------------------------------------------------------------------------------- host side
def summarize(games, ids, n_groups, nash, cartel, max_iters):
    """stationary.summarize's rows, one per group, plus n_switch_max, unresolved_mean and unresolved_max over the
    group's games (solved or not: they describe the sampling of the strategies, not the chain)."""
    rows = sn.summarize(games, ids, n_groups, nash, cartel, max_iters)
    ids = np.asarray(ids, np.int64).reshape(-1)
    ns = np.asarray(games["n_switch"], np.int64)
    un = np.asarray(games["unresolved"], np.float64)
    for r in rows:
        m = ids == r["group"]
        r["n_switch_max"] = int(ns[m].max()) if m.any() else None
        r["unresolved_mean"] = an.mean(un[m])
        r["unresolved_max"] = an.num(un[m].max()) if m.any() else None
    return rows


def combine(parts):
    """Per-game arrays of disjoint sets of games (in global game order) as one run's: concatenated along the game axis
    (axis 0 of pi [G, T], the last axis of the others)."""
    return an.combine(parts, other={"pi": 0}, only=PER_GAME)


def describe(options, n_cells, T, nash, cartel, summary):
    """greedy_stationary.json's content."""
    return {"options": options, "n_cells": int(n_cells), "T": int(T), "nash": nash, "cartel": cartel,
            "quantiles": list(sn.QUANTILES), "benchmark": "noise-free Nash and Cartel rewards (environment.get_optimal)",
            "summary": summary}


def save_games(d, r):
    """gstat_iters int32 [2, G] (iters, n_switch), gstat_games float64 [5, G] (change, mass, stat_price, unresolved,
    noise_prob), gstat_reward and gstat_action float64 [N, G]; from given start tuples gstat_start int32 [G]; with the
    distributions gstat_pi float64 [G, T]."""
    np.save(os.path.join(d, "gstat_iters.npy"), np.stack([r["iters"], r["n_switch"]]).astype(np.int32))
    np.save(os.path.join(d, "gstat_games.npy"),
            np.stack([np.asarray(r[f], np.float64) for f in GAME_FLOAT + ("noise_prob",)]))
    np.save(os.path.join(d, "gstat_reward.npy"), np.asarray(r["stat_reward"], np.float64))
    np.save(os.path.join(d, "gstat_action.npy"), np.asarray(r["stat_action"], np.float64))
    for f, name in (("start", "gstat_start.npy"), ("pi", "gstat_pi.npy")):
        path = os.path.join(d, name)
        if f in r:
            np.save(path, np.asarray(r[f], np.int32 if f == "start" else np.float64))
        elif os.path.isfile(path):               # a file left by an earlier run with other options
            os.remove(path)


def load_games(d):
    """The per-game arrays one run directory holds (training.greedy_stationary)."""
    it = np.load(os.path.join(d, "gstat_iters.npy"))
    gm = np.load(os.path.join(d, "gstat_games.npy"))
    g = {"iters": it[0], "n_switch": it[1]}
    g.update({f: gm[k] for k, f in enumerate(GAME_FLOAT + ("noise_prob",))})
    g.update(stat_reward=np.load(os.path.join(d, "gstat_reward.npy")), stat_action=np.load(os.path.join(d, "gstat_action.npy")))
    for f, name in (("start", "gstat_start.npy"), ("pi", "gstat_pi.npy")):
        if os.path.isfile(os.path.join(d, name)):
            g[f] = np.load(os.path.join(d, name))
    return g


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, tuple_policy=None):
    """train_one's training.greedy_stationary outputs: the per-game gstat_*.npy files and greedy_stationary.json."""
    tabs = tables(config, opt["resolution"])
    r = run(batch, noise_prob=opt["noise_prob"], start=opt["start"], tol=opt["tol"], max_iters=opt["max_iters"],
            pi=opt["pi"], tuple_policy=tuple_policy, tabs=tabs)
    save_games(exp_path, r)
    nash, cartel = optimal(config)
    summary = summarize(r, ids, n_groups, nash, cartel, opt["max_iters"])
    an.save_json(os.path.join(exp_path, "greedy_stationary.json"), describe(opt, r["n_cells"], r["T"], nash, cartel, summary))
    return r
