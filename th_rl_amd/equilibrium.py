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

Under demand noise (thrl_equilibrium_noise; the option "noise" of training.equilibrium) the same question is asked in
the environment of stationary.py, where every price cell is reachable and there is no path: run_noise() gives iters,
sweeps, n_diff_all, loss_all, loss_all_mean [N, G] and, weighted by the long-run distribution over the cells
(stationary.run's pi) or by weights of the caller's, loss_w, diff_w, v_w [N, G]; br_all = loss_all <= tol and br_w =
loss_w <= tol.  summarize_noise() gives per (group, agent) games, capped, br_all, br_w, the quantiles of loss_all and
loss_w over the games where they are positive, diff_w_mean and sweeps_max, and per group perfect.  The noise-free
artefacts are what they were; the noisy ones are eqn_*.npy and equilibrium_noise.json.
"""
import ctypes
import json
import os

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .analysis import QUANTILES, save_json  # noqa: F401  (eq.save_json stays a public name)

DEFAULTS = dict(tol=0.0, policies=False)
NOISE_DEFAULTS = dict(noise_prob=None, eval_tol=1e-12, max_sweeps=8192)
NOISE_INT = ("iters", "sweeps", "n_diff_all")
NOISE_FLOAT = ("loss_all", "loss_all_mean")
NOISE_WEIGHTED = ("loss_w", "diff_w", "v_w")
INT_FIELDS = ("iters", "n_diff_all", "n_diff_on")
FLOAT_FIELDS = ("loss_all", "loss_on", "loss_all_mean", "loss_on_mean", "v_on")
COLLUSIVE_GAIN = 0.5
NEURAL_FOLLOW_UP = ("the equilibrium check runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def check_config(config):
    """ValueError for a config with neural agents (the check needs every agent's greedy table)."""
    an.check_qtable_only(config, "equilibrium", NEURAL_FOLLOW_UP)


def check_gamma(gammas, what="gamma"):
    """ValueError unless every gamma lies in [0, 1): the discounted values need it."""
    g = np.asarray(gammas, np.float64)
    if g.size and not bool(np.all((g >= 0.0) & (g < 1.0))):
        bad = g.ravel()[~((g.ravel() >= 0.0) & (g.ravel() < 1.0))][0]
        raise ValueError("training.equilibrium: %s=%r: the equilibrium check needs gamma in [0, 1)" % (what, float(bad)))


def parse_options(opt, config):
    """training.equilibrium (true or a dict) -> the dict with every key filled in: agents (those solved, default all),
    tol, policies (store the per-state arrays), and tables when given.  Refuses neural agents and, for the solved
    agents, a gamma outside [0, 1) in the config or in training.sweep.gamma.  The optional key "noise" (true or
    {"noise_prob": a number in (0, 1] or None = the run's own noise, refused for a noise-free run as
    training.stationary does; "eval_tol", "max_sweeps": the stopping rule of an evaluation}) asks for the check under
    demand noise as well; it stays in the result, filled in, only when given."""
    check_config(config)
    noise = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        noise = opt.pop("noise")
        noise = None if noise is None or noise is False else parse_noise(noise, config)
    n = len(config["agents"])
    out = an.options("equilibrium", opt, dict(DEFAULTS, agents=list(range(n))), tables=True)
    out["agents"] = sorted(set(int(d) for d in out["agents"]))
    if not out["agents"] or any(not 0 <= d < n for d in out["agents"]):
        raise ValueError("training.equilibrium.agents %r: agents must lie in [0, %d)" % (out["agents"], n))
    out["tol"] = float(out["tol"])
    if not out["tol"] >= 0.0:
        raise ValueError("training.equilibrium.tol=%r must be >= 0" % (out["tol"],))
    out["policies"] = bool(out["policies"])
    sweep = (config.get("training") or {}).get("sweep") or {}
    for d in out["agents"]:
        if "gamma" in sweep:
            sg = np.asarray(sweep["gamma"], np.float64)
            check_gamma(sg[d] if sg.ndim == 2 else sg, "sweep.gamma")
        else:
            check_gamma([float(dict(_lib.QTABLE_DEFAULTS, **config["agents"][d])["gamma"])], "agents[%d].gamma" % d)
    if noise is not None:
        out["noise"] = noise
    return out


def parse_noise(noise, config):
    """training.equilibrium.noise (true or a dict) -> the dict with every key filled in."""
    name = "training.equilibrium.noise"
    out = an.options("equilibrium.noise", noise, NOISE_DEFAULTS)
    if out["noise_prob"] is None:       # the run's own noise: refuse a noise-free run before training
        env = dict(_lib.ENV_DEFAULTS, **config["environment"])
        sweep = (config.get("training") or {}).get("sweep") or {}
        if float(env["noise_prob"]) == 0.0 and "noise_prob" not in sweep:
            raise ValueError("%s: the environment has noise_prob = 0: give the noise_prob to analyse" % name)
    else:
        from . import stationary as sn
        out["noise_prob"] = sn.check_prob(out["noise_prob"], name + ".noise_prob")
    t = out["eval_tol"]
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0.0:
        raise ValueError("%s.eval_tol must be a number >= 0, got %r" % (name, t))
    out["eval_tol"] = float(t)
    m = out["max_sweeps"]
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= _lib.STAT_MAX_ITERS:
        raise ValueError("%s.max_sweeps must be an integer in [1, %d], got %r" % (name, _lib.STAT_MAX_ITERS, m))
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
    a = _lib.EquilibriumArgs()
    a.n_games, a.agents = 1, 1
    return an.n_states(batch, "thrl_equilibrium", a)


def run(batch, agents=None, state0=None, policies=False, tol=0.0, q=None):
    """thrl_equilibrium for every game of `batch` (a GameBatch or an all-QTable MixedGameBatch; see
    GameBatch.equilibrium).  q: a device tensor shaped and typed like batch.q analysed in place of the batch's tables
    (e.g. convergence.Tracker.tables_at_convergence)."""
    import torch
    G, N = batch.G, batch.N
    ag, mask = agents_mask(agents, N)
    dev = batch.device
    q = an.tables_tensor(batch, q, "equilibrium")
    S = n_states(batch)
    a = _lib.EquilibriumArgs()
    a.n_games, a.agents = G, mask
    with torch.cuda.device(dev):
        s0 = an.state0_tensor(batch, state0, G, "equilibrium")
        gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
        if gam is not None:
            sel = gam[ag]
            if not bool(((sel >= 0.0) & (sel < 1.0)).all()):
                raise ThrlError("equilibrium: the per-game sweep gamma must lie in [0, 1)")
        out = an.outputs(dev, (("mu", "lam"), (G,), "int32"), (INT_FIELDS, (N, G), "int32"), (FLOAT_FIELDS, (N, G), "float64"),
                         (("br_policy",) if policies else (), (N, G, S), "int16"),
                         (("v_opt", "v_pi") if policies else (), (N, G, S), "float64"))
        a.state0 = s0.data_ptr()
        a.sweep_gamma = gam.data_ptr() if gam is not None else None
        an.bind(a, out)
        _lib.check(batch.L.thrl_equilibrium(ctypes.byref(batch.cfg), q.data_ptr(), ctypes.byref(a), batch._stream()),
                   "thrl_equilibrium")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
    if policies:
        res["br_policy"] = res["br_policy"].view(np.uint16)
    res["agents"] = ag
    res["n_states"] = S
    res["tol"] = float(tol)
    res.update(flags(res, ag, tol))
    return res


def run_noise(batch, agents=None, noise_prob=None, eval_tol=1e-12, max_sweeps=8192, policies=False, tol=0.0, q=None,
              policy=None, weights="stationary", n_games=None, tabs=None):
    """thrl_equilibrium_noise for the first n_games (default all) games of `batch` (a GameBatch or an all-QTable
    MixedGameBatch; see AnalysisMethods.equilibrium_noise).  tabs: stationary.tables(batch.config), or a dict that
    replaces some of them.  weights="stationary": the policies are extracted once (crossplay.extract) and handed to
    stationary.run (tol 1e-12, at most 8192 steps) and to this call alike; a game whose stationary iteration stopped at
    its step limit is weighted by its last iterate all the same, and a game that iteration did not solve by zeros.
    Returns a dict of numpy arrays."""
    import torch
    from . import stationary as sn
    from .attractors import policy_entries
    N = batch.N
    G = an.games(batch, n_games, "equilibrium_noise")
    ag, mask = agents_mask(agents, N)
    dev = batch.device
    given = policy is not None
    P = policy_entries(batch)
    if given:
        an.check_policy(batch, policy, (G, P), "equilibrium_noise", more_games=True)
    else:
        q = an.tables_tensor(batch, q, "equilibrium_noise")
    if tabs is None:
        tabs = sn.tables(batch.config)
    J, T, W = int(tabs["n_cells"]), int(tabs["n_tuples"]), int(tabs["band_w"])
    a = _lib.EquilibriumNoiseArgs()
    a.n_games, a.agents, a.n_cells, a.band_w = G, mask, J, W
    a.max_sweeps, a.eval_tol = int(max_sweeps), float(eval_tol)
    a.flags = _lib.EQN_POLICY_GIVEN if given else 0
    nt = ctypes.c_int32(-1)
    a.n_tuples = ctypes.pointer(nt)
    with torch.cuda.device(dev):
        p, p_g = sn.resolve_noise(batch, noise_prob, G)
        pi = None
        if isinstance(weights, str):
            if weights != "stationary":
                raise ThrlError("equilibrium_noise: weights must be 'stationary', None or a [G, J] array, got %r"
                                % (weights,))
            if not given:       # one extraction serves both calls, which then read the same policies
                from .crossplay import extract
                policy, given = extract(batch, q), True
            st = sn.run(batch, noise_prob=noise_prob, start="reset", pi=True, policy=policy, n_games=G, tabs=tabs)
            pi = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
            a.flags = _lib.EQN_POLICY_GIVEN
        elif weights is not None:
            if isinstance(weights, torch.Tensor):
                pi = weights.to(device=dev, dtype=torch.float64).contiguous()
            else:
                pi = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, np.float64))).to(dev)
            if tuple(pi.shape) != (G, J):
                raise ThrlError("equilibrium_noise: weights must be shaped %s, got %s" % ((G, J), tuple(pi.shape)))
        if not given:
            policy = torch.empty((G, P), dtype=torch.int16, device=dev)
        keep = an.bind_tables(a, tabs, [("cell_rows", (N, J), np.int32), ("det_cell", (T,), np.int32),
                                        ("band_lo", (T,), np.int32), ("band", (T, W), np.float64),
                                        ("noise_reward", (N, T), np.float64)], dev, "equilibrium_noise")
        if p_g is not None:
            a.noise_prob_g = p_g.data_ptr()
        else:
            a.noise_prob = p
        gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
        if gam is not None:
            gam = gam[:, :G].contiguous()
            a.sweep_gamma = gam.data_ptr()
        a.policy = policy.data_ptr()
        if pi is not None:
            a.weights = pi.data_ptr()
        out = an.outputs(dev, (NOISE_INT, (N, G), "int32"), (NOISE_FLOAT, (N, G), "float64"),
                         (NOISE_WEIGHTED if pi is not None else (), (N, G), "float64"),
                         (("br_policy",) if policies else (), (N, G, J), "int16"),
                         (("v_opt", "v_pi") if policies else (), (N, G, J), "float64"))
        an.bind(a, out)
        rc = batch.L.thrl_equilibrium_noise(ctypes.byref(batch.cfg), None if given else q.data_ptr(), ctypes.byref(a),
                                            batch._stream())
        if nt.value >= 0 and nt.value != T:
            raise ThrlError("equilibrium_noise: the tables hold %d action tuples, the batch's config has %d" % (T, nt.value))
        _lib.check(rc, "thrl_equilibrium_noise")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["noise_prob"] = np.full(G, p, np.float64) if p_g is None else p_g.cpu().numpy()
    if policies:
        res["br_policy"] = res["br_policy"].view(np.uint16)
    res["agents"], res["n_cells"], res["tol"] = ag, J, float(tol)
    res["eval_tol"], res["max_sweeps"] = float(eval_tol), int(max_sweeps)
    res.update(flags_noise(res, ag, tol))
    return res


# ---------------------------------------------------------------------------------------------- host side
def flags_noise(games, agents, tol=0.0):
    """br_all [N, G] and, with weights, br_w [N, G] (False for agents not solved and for games with iters = -1), and
    perfect [G] over the solved agents."""
    lall = np.asarray(games["loss_all"], np.float64)
    solved = np.zeros(lall.shape[0], bool)
    solved[list(agents)] = True
    done = solved[:, None] & (np.asarray(games["iters"]) >= 0)
    with np.errstate(invalid="ignore"):
        out = {"br_all": (lall <= float(tol)) & done}
        if "loss_w" in games:
            out["br_w"] = (np.asarray(games["loss_w"], np.float64) <= float(tol)) & done
    out["perfect"] = out["br_all"][solved].all(axis=0)
    return out


def summarize_noise(games, ids, n_groups, agents, tol=0.0):
    """The summary rows of the check under noise: for every group one row per solved agent (games, capped = games with
    iters == -1, br_all, br_w, loss_all_q*, loss_w_q* over the games where they are positive, diff_w_mean over the
    solved games, sweeps_max), then one row with agent None (perfect = every solved agent br_all).  Without weights
    br_w, the loss_w quantiles and diff_w_mean are None."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    fl = flags_noise(games, agents, tol)
    iters, sweeps = np.asarray(games["iters"]), np.asarray(games["sweeps"])
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        for i in agents:
            ok = m & (iters[i] >= 0)
            row = {"group": k, "agent": int(i), "games": int(m.sum()), "capped": int(np.sum(iters[i][m] == -1)),
                   "br_all": an.frac(fl["br_all"][i][m]), "br_w": an.frac(fl["br_w"][i][m]) if "br_w" in fl else None}
            for name in ("loss_all", "loss_w"):
                x = np.asarray(games[name], np.float64)[i][ok] if name in games else np.zeros(0)
                an.quantiles(row, name, x[x > 0])
            row["diff_w_mean"] = an.mean(np.asarray(games["diff_w"], np.float64)[i][ok]) if "diff_w" in games else None
            row["sweeps_max"] = int(sweeps[i][m].max()) if m.any() else None
            out.append(row)
        out.append({"group": k, "agent": None, "games": int(m.sum()), "perfect": an.frac(fl["perfect"][m])})
    return out


NOISE_CELL = ("br_policy", "v_opt", "v_pi")


def combine_noise(parts):
    """combine() for the arrays of run_noise / load_noise_games."""
    return an.combine(parts, other={f: 1 for f in NOISE_CELL},
                      only=NOISE_INT + NOISE_FLOAT + NOISE_WEIGHTED + NOISE_CELL + ("noise_prob",))


def describe_noise(options, n_cells, summary):
    """equilibrium_noise.json's content."""
    return {"options": options, "n_cells": int(n_cells), "quantiles": list(QUANTILES), "summary": summary}


def save_noise_games(d, r):
    """eqn_iters int32 [3, N, G] (iters, sweeps, n_diff_all), eqn_loss [2, N, G] (loss_all, loss_all_mean), eqn_prob [G]
    (the noise probabilities analysed); with weights eqn_weighted [3, N, G] (loss_w, diff_w, v_w); with per-cell arrays
    eqn_policy, eqn_v_opt, eqn_v_pi [N, G, J]."""
    np.save(os.path.join(d, "eqn_iters.npy"), np.stack([r[f] for f in NOISE_INT]).astype(np.int32))
    np.save(os.path.join(d, "eqn_loss.npy"), np.stack([r[f] for f in NOISE_FLOAT]).astype(np.float64))
    np.save(os.path.join(d, "eqn_prob.npy"), np.asarray(r["noise_prob"], np.float64))
    if "loss_w" in r:
        np.save(os.path.join(d, "eqn_weighted.npy"), np.stack([r[f] for f in NOISE_WEIGHTED]).astype(np.float64))
    if "br_policy" in r:
        np.save(os.path.join(d, "eqn_policy.npy"), np.asarray(r["br_policy"], np.uint16))
        np.save(os.path.join(d, "eqn_v_opt.npy"), np.asarray(r["v_opt"], np.float64))
        np.save(os.path.join(d, "eqn_v_pi.npy"), np.asarray(r["v_pi"], np.float64))


def load_noise_games(d):
    """The per-game arrays of the check under noise one run directory (or shard) holds."""
    it, loss = np.load(os.path.join(d, "eqn_iters.npy")), np.load(os.path.join(d, "eqn_loss.npy"))
    g = {f: it[k] for k, f in enumerate(NOISE_INT)}
    g.update({f: loss[k] for k, f in enumerate(NOISE_FLOAT)})
    g["noise_prob"] = np.load(os.path.join(d, "eqn_prob.npy"))
    if os.path.isfile(os.path.join(d, "eqn_weighted.npy")):
        w = np.load(os.path.join(d, "eqn_weighted.npy"))
        g.update({f: w[k] for k, f in enumerate(NOISE_WEIGHTED)})
    if os.path.isfile(os.path.join(d, "eqn_policy.npy")):
        g.update(br_policy=np.load(os.path.join(d, "eqn_policy.npy")), v_opt=np.load(os.path.join(d, "eqn_v_opt.npy")),
                 v_pi=np.load(os.path.join(d, "eqn_v_pi.npy")))
    return g


def flags(games, agents, tol=0.0):
    """br_on, br_all [N, G] (False for agents not solved) and nash, perfect [G] over the solved agents."""
    lon, lall = np.asarray(games["loss_on"], np.float64), np.asarray(games["loss_all"], np.float64)
    solved = np.zeros(lon.shape[0], bool)
    solved[list(agents)] = True
    br_on = (lon <= float(tol)) & solved[:, None]
    br_all = (lall <= float(tol)) & solved[:, None]
    return {"br_on": br_on, "br_all": br_all, "nash": br_on[solved].all(axis=0), "perfect": br_all[solved].all(axis=0)}


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
            row = {"group": k, "agent": int(i), "games": int(m.sum()), "br_on": an.frac(fl["br_on"][i][m]),
                   "br_all": an.frac(fl["br_all"][i][m]), "capped": int(np.sum(iters[i][m] == -1))}
            for name in ("loss_on", "loss_all"):
                x = np.asarray(games[name], np.float64)[i][m]
                an.quantiles(row, name, x[x > 0])
            out.append(row)
        row = {"group": k, "agent": None, "games": int(m.sum()), "nash": an.frac(fl["nash"][m]),
               "perfect": an.frac(fl["perfect"][m]), "collusive": None, "nash_collusive": None, "perfect_collusive": None}
        if delta is not None:
            c = m & (np.asarray(delta, np.float64) > COLLUSIVE_GAIN)
            row.update(collusive=int(c.sum()), nash_collusive=an.frac(fl["nash"][c]), perfect_collusive=an.frac(fl["perfect"][c]))
        out.append(row)
    return out


def combine(parts):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis
    (axis 1 of the per-state [N, G, S] arrays, the last axis of the others)."""
    return an.combine(parts, other={"br_policy": 1, "v_opt": 1, "v_pi": 1})


def describe(options, n_states, summary):
    """equilibrium.json's content (without the option "noise": the file is what it is without that option)."""
    options = {k: v for k, v in options.items() if k != "noise"}
    return {"options": options, "n_states": int(n_states), "quantiles": list(QUANTILES),
            "collusive_gain": COLLUSIVE_GAIN, "summary": summary}


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


def merged(shards, out, config, opt, ids, n_groups, first):
    """equilibrium.json and eq_*.npy of a sharded run (launch.merge_analysis); the collusive fractions where the shards
    had the deviation analysis's cycle rewards."""
    games = combine(load_games(s) for s in shards)
    save_games(out, games)
    delta = None
    if first["summary"] and first["summary"][-1]["collusive"] is not None:
        delta = np.concatenate([load_delta(s, config) for s in shards])
    if opt.get("noise"):        # the check under noise: its arrays concatenated, summarised as one run
        ng = combine_noise(load_noise_games(s) for s in shards)
        save_noise_games(out, ng)
        with open(os.path.join(shards[0], "equilibrium_noise.json")) as f:
            n_cells = json.load(f)["n_cells"]
        save_json(os.path.join(out, "equilibrium_noise.json"),
                  describe_noise(opt, n_cells, summarize_noise(ng, ids, n_groups, opt["agents"], opt["tol"])))
    return describe(opt, first["n_states"], summarize(games, ids, n_groups, opt["agents"], opt["tol"], delta))


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, q=None, state0=None):
    """train_one's training.equilibrium outputs: the per-game eq_*.npy files and equilibrium.json, and with the option
    "noise" the check under demand noise after them (eqn_*.npy, equilibrium_noise.json).  q / state0 (device
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
    if opt.get("noise"):
        nz = opt["noise"]
        rn = run_noise(batch, agents=opt["agents"], noise_prob=nz["noise_prob"], eval_tol=nz["eval_tol"],
                       max_sweeps=nz["max_sweeps"], policies=opt["policies"], tol=opt["tol"], q=q)
        save_noise_games(exp_path, rn)
        save_json(os.path.join(exp_path, "equilibrium_noise.json"),
                  describe_noise(opt, rn["n_cells"], summarize_noise(rn, ids, n_groups, opt["agents"], opt["tol"])))
