"""Equilibrium check of trained QTable games (thrl_equilibrium, include/thrl.h): the step of the algorithmic-collusion
protocol (Calvano, Calzolari, Denicolo, Pastorello, AER 2020) that says whether what the agents learned is an
equilibrium.  Hold the rivals' greedy strategies fixed, solve each agent's dynamic problem exactly (policy iteration
from its own greedy strategy), and ask whether that strategy is a best response on the path greedy play follows
(Nash) and in every state (subgame perfect) -- and if not, which share of the attainable value it gives up (the
paper's Q-loss).  training.deviation's "best_response" is the ONE-period best response; this is the patient one.

The per-game outputs (mu, lam [G]; iters, n_diff_all, n_diff_on, loss_all, loss_on, loss_all_mean, loss_on_mean, v_on
[N, G]) come from one kernel; the definitions are in include/thrl.h.  mu and lam are the pre-shock cycle of the
deviation analysis (deviation.py) with its default horizon, bit for bit.  This module parses training.equilibrium,
runs the kernel for a GameBatch or an all-QTable MixedGameBatch, and derives on the host, with a tolerance `tol`
(default 0.0: exact, which the kernel's keep-the-incumbent rule makes meaningful):

    br_on  [N, G] = loss_on  <= tol      agent i's strategy is a best response on the path
    br_all [N, G] = loss_all <= tol      ... in every state
    nash [G] = every solved agent br_on, perfect [G] = every solved agent br_all

and the summary, per (group, agent): games, br_on / br_all (fractions), loss_on_q25 / q50 / q75 and loss_all_q25 / q50
/ q75 over the games where the loss is positive, capped (games with iters == -1); per group (agent = None): nash,
perfect (fractions) and, when the cycle rewards of the deviation analysis are at hand, collusive (games whose profit
gain deviation.profit_gain exceeds COLLUSIVE_GAIN), nash_collusive and perfect_collusive (the two fractions among
those games).  Statistics that have no games are None.  Shards combine exactly: their per-game arrays are concatenated
in global game order (combine) and summarised as one run.
"""
import ctypes
import json
import os

import numpy as np

from . import _lib
from ._lib import ThrlError

DEFAULTS = dict(tol=0.0, policies=False)
INT_FIELDS = ("iters", "n_diff_all", "n_diff_on")
FLOAT_FIELDS = ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on")
QUANTILES = (0.25, 0.5, 0.75)
COLLUSIVE_GAIN = 0.5
NEURAL_FOLLOW_UP = ("the equilibrium check runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def check_config(config):
    """ValueError for a config with neural agents (the check needs every agent's greedy table)."""
    kinds = [a.get("name", "QTable") for a in config["agents"]]
    if any(k != "QTable" for k in kinds):
        raise ValueError("training.equilibrium: agents %s: %s" % (kinds, NEURAL_FOLLOW_UP))


def check_gamma(gammas, what="gamma"):
    """ValueError unless every gamma lies in [0, 1): the discounted values need it."""
    g = np.asarray(gammas, np.float64)
    if g.size and not bool(np.all((g >= 0.0) & (g < 1.0))):
        bad = g.ravel()[~((g.ravel() >= 0.0) & (g.ravel() < 1.0))][0]
        raise ValueError("training.equilibrium: %s=%r: the equilibrium check needs gamma in [0, 1)" % (what, float(bad)))


def parse_options(opt, config):
    """training.equilibrium (true or a dict) -> the dict with every key filled in: agents (those solved, default all),
    tol, policies (store the per-state arrays), and tables when given.  Refuses neural agents and, for the solved
    agents, a gamma outside [0, 1) in the config or in training.sweep.gamma."""
    check_config(config)
    n = len(config["agents"])
    if opt is True:
        opt = {}
    if not isinstance(opt, dict):
        raise ValueError("training.equilibrium must be true or a dict, got %r" % (opt,))
    known = {"agents", "tol", "policies", "tables"}
    bad = set(opt) - known
    if bad:
        raise ValueError("training.equilibrium: unknown keys %s (known: %s)" % (sorted(bad), ", ".join(sorted(known))))
    out = dict(DEFAULTS, agents=list(range(n)))
    out.update(opt)
    out["agents"] = sorted(set(int(d) for d in out["agents"]))
    if not out["agents"] or any(not 0 <= d < n for d in out["agents"]):
        raise ValueError("training.equilibrium.agents %r: agents must lie in [0, %d)" % (out["agents"], n))
    out["tol"] = float(out["tol"])
    if not out["tol"] >= 0.0:
        raise ValueError("training.equilibrium.tol=%r must be >= 0" % (out["tol"],))
    out["policies"] = bool(out["policies"])
    if "tables" in out and out["tables"] not in ("final", "converged"):
        raise ValueError("training.equilibrium.tables must be 'final' or 'converged', got %r" % (out["tables"],))
    sweep = (config.get("training") or {}).get("sweep") or {}
    for d in out["agents"]:
        if "gamma" in sweep:
            sg = np.asarray(sweep["gamma"], np.float64)
            check_gamma(sg[d] if sg.ndim == 2 else sg, "sweep.gamma")
        else:
            check_gamma([float(dict(_lib.QTABLE_DEFAULTS, **config["agents"][d])["gamma"])], "agents[%d].gamma" % d)
    return out


def agents_mask(agents, n):
    if agents is None:
        return list(range(n)), (1 << n) - 1
    ag = sorted(set(int(d) for d in agents))
    if not ag or any(not 0 <= d < n for d in ag):
        raise ThrlError("equilibrium: agents %r must be a non-empty subset of [0, %d)" % (list(agents), n))
    return ag, sum(1 << d for d in ag)


# ---------------------------------------------------------------------------------------------- the device call
def n_states(batch):
    """S of the batch's config (include/thrl.h "States"), from the library's own plan; no device work."""
    s = ctypes.c_int32(-1)
    a = _lib.EquilibriumArgs()
    a.n_games, a.agents = 1, 1
    a.n_states = ctypes.pointer(s)
    rc = batch.L.thrl_equilibrium(ctypes.byref(batch.cfg), None, ctypes.byref(a), None)
    if s.value < 0:
        _lib.check(rc, "thrl_equilibrium")
    return int(s.value)


def run(batch, agents=None, state0=None, policies=False, tol=0.0, q=None):
    """thrl_equilibrium for every game of `batch` (a GameBatch or an all-QTable MixedGameBatch; see
    GameBatch.equilibrium).  q: a device tensor shaped and typed like batch.q analysed in place of the batch's tables
    (e.g. convergence.Tracker.tables_at_convergence)."""
    import torch
    G, N = batch.G, batch.N
    ag, mask = agents_mask(agents, N)
    dev = batch.device
    if q is None:
        q = batch.q
    elif tuple(q.shape) != tuple(batch.q.shape) or q.dtype != batch.q.dtype or q.device != batch.q.device \
            or not q.is_contiguous():
        raise ThrlError("equilibrium: q must be a contiguous %s tensor %s on %s" % (batch.q.dtype, tuple(batch.q.shape), dev))
    S = n_states(batch)
    a = _lib.EquilibriumArgs()
    a.n_games, a.agents = G, mask
    with torch.cuda.device(dev):
        if state0 is None:
            s0 = batch.state
        elif isinstance(state0, torch.Tensor):
            s0 = state0.to(device=dev, dtype=torch.float64).reshape(G).contiguous()
        else:
            s0 = torch.from_numpy(np.ascontiguousarray(np.asarray(state0, np.float64).reshape(G))).to(dev)
        gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
        if gam is not None:
            sel = gam[ag]
            if not bool(((sel >= 0.0) & (sel < 1.0)).all()):
                raise ThrlError("equilibrium: the per-game sweep gamma must lie in [0, 1)")
        out = {"mu": torch.zeros((G,), dtype=torch.int32, device=dev),
               "lam": torch.zeros((G,), dtype=torch.int32, device=dev)}
        out.update({f: torch.zeros((N, G), dtype=torch.int32, device=dev) for f in INT_FIELDS})
        out.update({f: torch.zeros((N, G), dtype=torch.float64, device=dev) for f in FLOAT_FIELDS})
        if policies:
            out["br_policy"] = torch.zeros((N, G, S), dtype=torch.int16, device=dev)
            out["v_opt"] = torch.zeros((N, G, S), dtype=torch.float64, device=dev)
            out["v_pi"] = torch.zeros((N, G, S), dtype=torch.float64, device=dev)
        a.state0 = s0.data_ptr()
        a.sweep_gamma = gam.data_ptr() if gam is not None else None
        for f, t in out.items():
            setattr(a, f, t.data_ptr())
        _lib.check(batch.L.thrl_equilibrium(ctypes.byref(batch.cfg), q.data_ptr(), ctypes.byref(a), batch._stream()),
                   "thrl_equilibrium")
        torch.cuda.synchronize(dev)
        res = {f: t.cpu().numpy() for f, t in out.items()}
    if policies:
        res["br_policy"] = res["br_policy"].view(np.uint16)
    res["agents"] = ag
    res["n_states"] = S
    res["tol"] = float(tol)
    res.update(flags(res, ag, tol))
    return res


# ---------------------------------------------------------------------------------------------- host side
def flags(games, agents, tol=0.0):
    """br_on, br_all [N, G] (False for agents not solved) and nash, perfect [G] over the solved agents."""
    lon, lall = np.asarray(games["loss_on"], np.float64), np.asarray(games["loss_all"], np.float64)
    solved = np.zeros(lon.shape[0], bool)
    solved[list(agents)] = True
    br_on = (lon <= float(tol)) & solved[:, None]
    br_all = (lall <= float(tol)) & solved[:, None]
    return {"br_on": br_on, "br_all": br_all, "nash": br_on[solved].all(axis=0), "perfect": br_all[solved].all(axis=0)}


def _num(x):
    return None if x is None or not np.isfinite(x) else float(x)


def _frac(mask):
    return _num(mask.mean()) if mask.size else None


def summarize(games, ids, n_groups, agents, tol=0.0, delta=None):
    """The summary rows: for every group one row per solved agent, then one row with agent None.  games = dict of
    per-game arrays in global game order, ids = group id per game, delta [G] = the profit gain per game or None."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    fl = flags(games, agents, tol)
    iters = np.asarray(games["iters"])
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        for i in agents:
            row = {"group": k, "agent": int(i), "games": int(m.sum()), "br_on": _frac(fl["br_on"][i][m]),
                   "br_all": _frac(fl["br_all"][i][m]), "capped": int(np.sum(iters[i][m] == -1))}
            for name in ("loss_on", "loss_all"):
                x = np.asarray(games[name], np.float64)[i][m]
                x = x[x > 0]
                qs = np.quantile(x, QUANTILES) if x.size else [None] * len(QUANTILES)
                for qq, v in zip(QUANTILES, qs):
                    row["%s_q%d" % (name, int(round(qq * 100)))] = _num(v)
            out.append(row)
        row = {"group": k, "agent": None, "games": int(m.sum()), "nash": _frac(fl["nash"][m]),
               "perfect": _frac(fl["perfect"][m]), "collusive": None, "nash_collusive": None, "perfect_collusive": None}
        if delta is not None:
            c = m & (np.asarray(delta, np.float64) > COLLUSIVE_GAIN)
            row.update(collusive=int(c.sum()), nash_collusive=_frac(fl["nash"][c]), perfect_collusive=_frac(fl["perfect"][c]))
        out.append(row)
    return out


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis
    (axis 1 of the per-state [N, G, S] arrays, the last axis of the others)."""
    parts = list(parts)
    return {f: np.concatenate([np.asarray(p[f]) for p in parts], axis=1 if np.asarray(parts[0][f]).ndim == 3 else -1)
            for f in parts[0]}


def describe(options, n_states, summary):
    """equilibrium.json's content."""
    return {"options": options, "n_states": int(n_states), "quantiles": list(QUANTILES),
            "collusive_gain": COLLUSIVE_GAIN, "summary": summary}


def save_json(path, content):
    with open(path, "w") as f:
        json.dump(content, f, indent=2)


# ---------------------------------------------------------------------------------------------- artefacts
FILES = {"eq_cycle.npy": None, "eq_iters.npy": "iters", "eq_diff.npy": None, "eq_loss.npy": None, "eq_value.npy": "v_on"}


def save_games(d, r):
    """eq_cycle [2, G] (mu, lam), eq_iters [N, G], eq_diff [2, N, G] (n_diff_all, n_diff_on), eq_loss [4, N, G]
    (loss_all, loss_on, loss_all_mean, loss_on_mean), eq_value [N, G] (v_on); with per-state arrays eq_policy,
    eq_v_opt, eq_v_pi [N, G, S]."""
    np.save(os.path.join(d, "eq_cycle.npy"), np.stack([r["mu"], r["lam"]]).astype(np.int32))
    np.save(os.path.join(d, "eq_iters.npy"), np.asarray(r["iters"], np.int32))
    np.save(os.path.join(d, "eq_diff.npy"), np.stack([r["n_diff_all"], r["n_diff_on"]]).astype(np.int32))
    np.save(os.path.join(d, "eq_loss.npy"),
            np.stack([r["loss_all"], r["loss_on"], r["loss_all_mean"], r["loss_on_mean"]]).astype(np.float64))
    np.save(os.path.join(d, "eq_value.npy"), np.asarray(r["v_on"], np.float64))
    if "br_policy" in r:
        np.save(os.path.join(d, "eq_policy.npy"), np.asarray(r["br_policy"], np.uint16))
        np.save(os.path.join(d, "eq_v_opt.npy"), np.asarray(r["v_opt"], np.float64))
        np.save(os.path.join(d, "eq_v_pi.npy"), np.asarray(r["v_pi"], np.float64))


def load_games(d):
    """The per-game arrays one run directory (or shard) holds."""
    cyc, diff, loss = (np.load(os.path.join(d, "eq_%s.npy" % f)) for f in ("cycle", "diff", "loss"))
    g = {"mu": cyc[0], "lam": cyc[1], "iters": np.load(os.path.join(d, "eq_iters.npy")), "n_diff_all": diff[0],
         "n_diff_on": diff[1], "loss_all": loss[0], "loss_on": loss[1], "loss_all_mean": loss[2],
         "loss_on_mean": loss[3], "v_on": np.load(os.path.join(d, "eq_value.npy"))}
    if os.path.isfile(os.path.join(d, "eq_policy.npy")):
        g.update(br_policy=np.load(os.path.join(d, "eq_policy.npy")), v_opt=np.load(os.path.join(d, "eq_v_opt.npy")),
                 v_pi=np.load(os.path.join(d, "eq_v_pi.npy")))
    return g


def load_delta(d, config):
    """The profit gain per game from the deviation analysis' cycle rewards in `d`, or None without them."""
    path = os.path.join(d, "dev_cycle_reward.npy")
    if not os.path.isfile(path):
        return None
    from . import deviation as dv
    nash, cartel = dv.optimal(config)
    return dv.profit_gain(np.load(path), nash, cartel)


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, q=None, state0=None):
    """train_one's training.equilibrium outputs: the per-game eq_*.npy files and equilibrium.json.  q / state0 (device
    tensors): the tables and start prices analysed in place of the batch's (opt["tables"] == "converged").  The
    collusive fractions use dev_cycle_reward.npy when training.deviation wrote it for the same tables and start."""
    r = run(batch, agents=opt["agents"], state0=state0, policies=opt["policies"], tol=opt["tol"], q=q)
    save_games(exp_path, r)
    delta = None
    dv = (config.get("training") or {}).get("deviation")
    if dv is not None and dv is not False:
        same = not isinstance(dv, dict) or dv.get("tables", "final") == opt.get("tables", "final")
        delta = load_delta(exp_path, config) if same else None
    summary = summarize(r, ids, n_groups, opt["agents"], opt["tol"], delta)
    save_json(os.path.join(exp_path, "equilibrium.json"), describe(opt, r["n_states"], summary))
