"""Attractor analysis of trained QTable games (thrl_attractors, include/thrl.h): ALL limit cycles of a game's greedy
play and their basins.  The deviation test, the equilibrium check and cross-play follow the one path that starts at
the price the game happened to hold when training stopped; a trained pair of tables defines a map on states, and that
map usually has several limit cycles (two or more in most fresh headline games).  This analysis answers whether the
cycle a run reports is the only outcome of the learned strategies, whether it is the outcome from most starting prices,
and what greedy play earns in expectation over the environment's reset distribution -- the exact value of what the
reference's averaged greedy plots (utils.plot_mean_conf / plot_sweep_conf: play_game from environment.reset(), a
uniform draw on [0, a)) estimate by sampling.

Per game (definitions in include/thrl.h): n_attr, mu_max, n_cycle_states [G]; the KEEP = 8 attractors with the largest
basins as rep, lam, basin [KEEP, G] and cycle_reward, cycle_action [KEEP, N, G]; the training state's attractor rep_x0,
mu_x0, slot_x0 [G]; with the reset starts (starts()) reset_mass [KEEP, G], reset_mass_other [G] and reset_reward [N, G];
optionally state_rep, state_mu [G, S].  summarize() gives, per group (profit gains are deviation.profit_gain, against
Nash / Cartel):

    games, single (share of games with one attractor), n_attr_q25 / q50 / q75 / max, mu_max_q25 / q50 / q75
    delta_train_mean     profit gain of the training state's attractor (games where it is among the kept)
    delta_largest_mean   profit gain of the attractor with the largest basin (slot 0)
    delta_reset_mean     the reset-expected profit gain, from reset_reward
    train_is_largest     share of games whose training attractor has the largest basin
    train_mass_q25 / q50 / q75   the training attractor's share of the reset distribution
    luck_mean            mean of (training gain - reset-expected gain): what the stopping point added

Statistics that have no games are None.  Shards combine exactly: their per-game arrays are concatenated in global game
order (combine) and summarised as one run.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .analysis import QUANTILES, save_json  # noqa: F401  (at.save_json stays a public name)
from .deviation import optimal, profit_gain

KEEP = _lib.ATTR_KEEP
DEFAULTS = dict(policies=False)
GAME_INT = ("n_attr", "mu_max", "n_cycle_states", "rep_x0", "mu_x0", "slot_x0")
SLOT_INT = ("rep", "lam", "basin")
SLOT_FLOAT = ("cycle_reward", "cycle_action")
RESET_FIELDS = ("reset_mass", "reset_mass_other", "reset_reward")
STATE_FIELDS = ("state_rep", "state_mu")
NEURAL_FOLLOW_UP = ("the attractor analysis runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def check_config(config):
    """ValueError for a config with neural agents (the analysis needs every agent's greedy table)."""
    an.check_qtable_only(config, "attractors", NEURAL_FOLLOW_UP)


def parse_options(opt, config):
    """training.attractors (true or a dict) -> the dict with every key filled in: policies (store the per-state
    arrays), and tables when given."""
    check_config(config)
    out = an.options("attractors", opt, DEFAULTS, tables=True)
    if not isinstance(out["policies"], bool):
        raise ValueError("training.attractors.policies must be true or false, got %r" % (out["policies"],))
    return out


# ---------------------------------------------------------------------------------------------- the reset starts
def encode64(price, states, max_state):
    """QTable.encode on float64 prices, clipped to the table as the device clamps it."""
    x = np.asarray(price, np.float64) / float(max_state)
    x = x * float(states)
    return np.clip(np.rint(x), 0, int(states)).astype(np.int64)


def starts(config):
    """(rows int32 [N, J], w float64 [J]): the reset distribution of the environment, a uniform price on [0, a), cut
    at every agent's encode breakpoints (k + 0.5) * max_state / states inside (0, a).  Interval j = [c_j, c_{j+1}):
    rows[i][j] = encode64_i at its midpoint, w[j] = (c_{j+1} - c_j) / a."""
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    a = float(env["a"])
    cuts = [np.array([0.0, a])]
    params = []
    for ag in config["agents"]:
        p = dict(_lib.QTABLE_DEFAULTS, **ag)
        n, ms = int(p["states"]), float(p["max_state"])
        params.append((n, ms))
        b = (np.arange(n, dtype=np.float64) + 0.5) * ms / float(n)
        cuts.append(b[(b > 0.0) & (b < a)])
    c = np.unique(np.concatenate(cuts))
    mid = (c[:-1] + c[1:]) / 2.0
    rows = np.stack([encode64(mid, n, ms) for n, ms in params]).astype(np.int32)
    w = (c[1:] - c[:-1]) / a
    if rows.shape[1] > _lib.ATTR_MAX_STARTS:
        raise ValueError("attractors: %d reset starts, at most %d" % (rows.shape[1], _lib.ATTR_MAX_STARTS))
    return rows, w


# ---------------------------------------------------------------------------------------------- the device call
def policy_entries(batch):
    return sum(int(batch.cfg.n_states[i]) + 1 for i in range(batch.N))


def n_states(batch):
    """S of the batch's config (include/thrl.h "States"), from the library's own plan."""
    a = _lib.AttractorsArgs()
    a.n_games = 1
    return an.n_states(batch, "thrl_attractors", a)


def run(batch, state0=None, policies=False, q=None, policy=None, reset=True, n_games=None):
    """thrl_attractors for the first n_games (default all) games of `batch` (a GameBatch or an all-QTable
    MixedGameBatch; see GameBatch.attractors).  q: a device tensor shaped and typed like batch.q analysed in place of
    the batch's tables; policy (a device int16 / uint16-bits tensor [G, P], e.g. convergence.Tracker.policy or
    crossplay.extract()): analysed as it is, no table is read.  reset: True = the environment's reset distribution
    (starts(batch.config)), False = none, or a (rows [N, J], w [J]) pair.  Returns a dict of numpy arrays."""
    import torch
    N = batch.N
    G = batch.G if n_games is None else int(n_games)
    if not 1 <= G <= batch.G:
        raise ThrlError("attractors: n_games=%r out of [1, %d]" % (n_games, batch.G))
    dev = batch.device
    given = policy is not None
    P = policy_entries(batch)
    if given:
        an.check_policy(batch, policy, (G, P), "attractors", more_games=True)
    else:
        q = an.tables_tensor(batch, q, "attractors")
    if reset is True:
        reset = starts(batch.config)
    S = n_states(batch)
    a = _lib.AttractorsArgs()
    a.n_games, a.flags = G, _lib.ATTR_POLICY_GIVEN if given else 0
    with torch.cuda.device(dev):
        s0 = an.state0_tensor(batch, state0, G, "attractors")
        if not given:
            policy = torch.empty((G, P), dtype=torch.int16, device=dev)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        out = {f: i32(G) for f in GAME_INT}
        out.update({f: i32(KEEP, G) for f in SLOT_INT})
        out.update({f: f64(KEEP, N, G) for f in SLOT_FLOAT})
        keep = []
        if reset:
            rows = np.ascontiguousarray(np.asarray(reset[0], np.int32))
            w = np.ascontiguousarray(np.asarray(reset[1], np.float64).reshape(-1))
            if rows.ndim != 2 or rows.shape != (N, w.size) or w.size < 1:
                raise ThrlError("attractors: reset must be (rows [N=%d, J], w [J]) with J >= 1" % N)
            keep = [torch.from_numpy(rows).to(dev), torch.from_numpy(w).to(dev)]
            a.n_starts, a.start_rows, a.start_w = int(w.size), keep[0].data_ptr(), keep[1].data_ptr()
            out.update(reset_mass=f64(KEEP, G), reset_mass_other=f64(G), reset_reward=f64(N, G))
        if policies:
            out["state_rep"] = torch.zeros((G, S), dtype=torch.int16, device=dev)
            out["state_mu"] = torch.zeros((G, S), dtype=torch.int16, device=dev)
        a.state0, a.policy = s0.data_ptr(), policy.data_ptr()
        an.bind(a, out)
        _lib.check(batch.L.thrl_attractors(ctypes.byref(batch.cfg), None if given else q.data_ptr(), ctypes.byref(a),
                                           batch._stream()), "thrl_attractors")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
    for f in STATE_FIELDS:
        if f in res:
            res[f] = res[f].view(np.uint16)
    res["n_states"] = S
    res["n_starts"] = int(a.n_starts)
    return res


# ---------------------------------------------------------------------------------------------- host side
def train_slot_values(games, field):
    """field [KEEP, ..., G] at every game's training slot -> [..., G]; NaN where the training attractor is not kept."""
    x = np.asarray(games[field], np.float64)
    slot = np.asarray(games["slot_x0"], np.int64)
    G = slot.size
    out = np.moveaxis(x, 0, -1)[..., np.arange(G), np.clip(slot, 0, x.shape[0] - 1)]
    return np.where(slot >= 0, out, np.nan)


def gains(games, nash, cartel):
    """Per-game profit gains [G]: train (NaN where the training attractor is not kept), largest, and reset (None
    without the reset outputs)."""
    cr = np.asarray(games["cycle_reward"], np.float64)
    out = {"train": profit_gain(train_slot_values(games, "cycle_reward"), nash, cartel),
           "largest": profit_gain(cr[0], nash, cartel), "reset": None}
    if "reset_reward" in games:
        out["reset"] = profit_gain(np.asarray(games["reset_reward"], np.float64), nash, cartel)
    return out


def summarize(games, ids, n_groups, nash, cartel):
    """The summary rows, one per group.  games = dict of per-game arrays in global game order, ids = group id per
    game."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    n_attr, mu_max = np.asarray(games["n_attr"]), np.asarray(games["mu_max"])
    slot = np.asarray(games["slot_x0"])
    gn = gains(games, nash, cartel)
    mass = train_slot_values(games, "reset_mass") if "reset_mass" in games else None
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        kept = m & (slot >= 0)
        row = {"group": k, "games": int(m.sum()), "single": an.mean(n_attr[m] == 1) if m.any() else None}
        an.quantiles(row, "n_attr", n_attr[m])
        row["n_attr_max"] = int(n_attr[m].max()) if m.any() else None
        an.quantiles(row, "mu_max", mu_max[m])
        row["delta_train_mean"] = an.mean(gn["train"][kept])
        row["delta_largest_mean"] = an.mean(gn["largest"][m])
        row["delta_reset_mean"] = an.mean(gn["reset"][m]) if gn["reset"] is not None else None
        row["train_is_largest"] = an.mean(slot[m] == 0) if m.any() else None
        an.quantiles(row, "train_mass", mass[kept] if mass is not None else [])
        row["luck_mean"] = an.mean(gn["train"][kept] - gn["reset"][kept]) if gn["reset"] is not None else None
        out.append(row)
    return out


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis (axis
    0 of the per-state [G, S] arrays, the last axis of the others)."""
    return an.combine(parts, other=dict.fromkeys(STATE_FIELDS, 0))


def describe(options, n_states, n_starts, nash, cartel, summary):
    """attractors.json's content."""
    return {"options": options, "n_states": int(n_states), "n_starts": int(n_starts), "keep": KEEP, "nash": nash,
            "cartel": cartel, "quantiles": list(QUANTILES), "summary": summary}


# ---------------------------------------------------------------------------------------------- artefacts
def save_games(d, r):
    """attr_games int32 [6, G] (n_attr, mu_max, n_cycle_states, rep_x0, mu_x0, slot_x0), attr_slots int32 [3, KEEP, G]
    (rep, lam, basin), attr_cycle float64 [2, KEEP, N, G] (cycle_reward, cycle_action); with the reset starts
    attr_reset_mass [KEEP + 1, G] (the slots, then the attractors not kept) and attr_reset_reward [N, G]; with
    per-state arrays attr_state uint16 [2, G, S] (rep, mu)."""
    np.save(os.path.join(d, "attr_games.npy"), np.stack([r[f] for f in GAME_INT]).astype(np.int32))
    np.save(os.path.join(d, "attr_slots.npy"), np.stack([r[f] for f in SLOT_INT]).astype(np.int32))
    np.save(os.path.join(d, "attr_cycle.npy"), np.stack([r[f] for f in SLOT_FLOAT]).astype(np.float64))
    if "reset_mass" in r:
        np.save(os.path.join(d, "attr_reset_mass.npy"),
                np.concatenate([r["reset_mass"], np.asarray(r["reset_mass_other"])[None]]).astype(np.float64))
        np.save(os.path.join(d, "attr_reset_reward.npy"), np.asarray(r["reset_reward"], np.float64))
    if "state_rep" in r:
        np.save(os.path.join(d, "attr_state.npy"), np.stack([r["state_rep"], r["state_mu"]]).astype(np.uint16))


def load_games(d):
    """The per-game arrays one run directory (or shard) holds."""
    gm, sl, cy = (np.load(os.path.join(d, "attr_%s.npy" % f)) for f in ("games", "slots", "cycle"))
    g = {f: gm[k] for k, f in enumerate(GAME_INT)}
    g.update({f: sl[k] for k, f in enumerate(SLOT_INT)})
    g.update({f: cy[k] for k, f in enumerate(SLOT_FLOAT)})
    if os.path.isfile(os.path.join(d, "attr_reset_mass.npy")):
        rm = np.load(os.path.join(d, "attr_reset_mass.npy"))
        g.update(reset_mass=rm[:-1], reset_mass_other=rm[-1], reset_reward=np.load(os.path.join(d, "attr_reset_reward.npy")))
    if os.path.isfile(os.path.join(d, "attr_state.npy")):
        st = np.load(os.path.join(d, "attr_state.npy"))
        g.update(state_rep=st[0], state_mu=st[1])
    return g


def merged(shards, out, config, opt, ids, n_groups, first):
    """attractors.json and attr_*.npy of a sharded run (launch.merge_analysis)."""
    games = combine(load_games(s) for s in shards)
    save_games(out, games)
    nash, cartel = optimal(config)
    return describe(opt, first["n_states"], first["n_starts"], nash, cartel, summarize(games, ids, n_groups, nash, cartel))


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, q=None, state0=None):
    """train_one's training.attractors outputs: the per-game attr_*.npy files and attractors.json.  q / state0 (device
    tensors): the tables and training states analysed in place of the batch's (opt["tables"] == "converged")."""
    reset = starts(config)
    r = run(batch, state0=state0, policies=opt["policies"], q=q, reset=reset)
    save_games(exp_path, r)
    nash, cartel = optimal(config)
    summary = summarize(r, ids, n_groups, nash, cartel)
    save_json(os.path.join(exp_path, "attractors.json"),
              describe(opt, r["n_states"], r["n_starts"], nash, cartel, summary))
