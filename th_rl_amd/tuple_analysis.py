"""Deviation test, equilibrium check and attractor analysis of trained games whose agents may be networks
(thrl_tuple_deviation, thrl_tuple_equilibrium, thrl_tuple_attractors, include/thrl.h): deviation.py, equilibrium.py and
attractors.py for any mix of QTable, Reinforce and ActorCritic agents, on the strategies in tuple form that
tuple_play.extract() fills.

A strategy of any discrete agent is a table over the game's T = prod_i A_i action tuples (tuple_play.py), so "is a
deviation punished" and "is the strategy a best response" are questions about a map on tuple indices: the state set
of the equilibrium check is the T tuples (n_states = T), and the paths of both analyses start at a tuple, by default
the one whose price is the state training stopped at (tuple_play.start_tuples; a game whose state is no tuple's price
has none: -1, refused by the deviation test, without on-path outputs in the equilibrium check, counted under no_start).

deviation() and equilibrium() return the dict fields of deviation.run / equilibrium.run plus "start"; the summaries
are deviation.summarize's and equilibrium.summarize's rows with no_start added.  The discount factor of agent i is the
per-game sweep gamma when the batch has one, else the agent's own gamma (a network's is its class default or the
config's, not the placeholder table slot's).  Sharded runs (th_rl_amd.launch) are refused.

attractors() returns attractors.run's dict fields with the T tuples as the state set (n_states = T) and start_mass,
start_mass_other, start_reward in place of the reset_* fields: the environment's reset distribution, a uniform price on
[0, a), would need a network's action at a continuum of prices, so its place is taken by a weight per start tuple,
by default 1 / T: a start drawn uniformly over action profiles, NOT the environment's reset.  The stationary analysis
in tuple form is tuple_stationary.py.

Under demand noise (thrl_tuple_equilibrium_noise; the option "noise" of training.greedy_equilibrium) the equilibrium
check is asked in the environment of tuple_stationary.py, on the S = T + J states "the price is exactly tuple t's" and
"the price lies in cell k": equilibrium_noise() gives iters, sweeps, n_diff_tuples, n_diff_cells, loss_all,
loss_tuples_mean, loss_cells_mean [N, G] and, weighted by where decisions are made in the long run (from
tuple_stationary.run's pi, or a pi of the caller's), loss_w, diff_w, v_w [N, G], with equilibrium.flags_noise's br_all,
br_w and perfect.  The noise-free artefacts are what they were; the noisy ones are geqn_*.npy and
greedy_equilibrium_noise.json.

The deviation test under demand noise (thrl_tuple_deviation_noise; the option "noise" of training.greedy_deviation) is
deviation.run_noise on the tuples: deviation_noise() starts from the long-run distribution over the tuple played
(tuple_stationary.run's pi from the reset start, or weights of the caller's), replaces the deviator's action in the tuple
played for dev_len periods and returns deviation.run_noise's fields plus n_switch, unresolved, T.  The noise-free
artefacts are what they were; the noisy ones are gdevn_*.npy, gdevn<d>_*.npy and greedy_deviation_noise.json.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from . import attractors as at
from . import deviation as dv
from . import equilibrium as eq
from . import tuple_play as tp
from ._lib import ThrlError

DEV_DEFAULTS = dict(dv.DEFAULTS)
EQ_DEFAULTS = dict(eq.DEFAULTS)
NOISE_DEFAULTS = dict(eq.NOISE_DEFAULTS, resolution=1024)
DEV_NOISE_DEFAULTS = dict(dv.NOISE_DEFAULTS, resolution=1024)
NOISE_INT = ("iters", "sweeps", "n_diff_tuples", "n_diff_cells")
NOISE_FLOAT = ("loss_all", "loss_tuples_mean", "loss_cells_mean")
NOISE_WEIGHTED = eq.NOISE_WEIGHTED
ATTR_DEFAULTS = dict(policies=False, weights="uniform")
KEEP = at.KEEP
START_FIELDS = ("start_mass", "start_mass_other", "start_reward")
TUPLE_FIELDS = ("tuple_rep", "tuple_mu")
UNIFORM_LABEL = "a start drawn uniformly over action profiles (1 / T per tuple), not the environment's reset distribution"


def _agent_gammas(config):
    from .mixed import NN_DEFAULTS
    return [float(dict(_lib.QTABLE_DEFAULTS if a.get("name", "QTable") == "QTable" else NN_DEFAULTS, **a)["gamma"])
            for a in config["agents"]]


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    return int(v)


def _agents(name, opt, n):
    try:
        ag = [_int(name + ".agents[]", d) for d in opt]
    except TypeError:
        raise ValueError("%s.agents must be a list of agent indices, got %r" % (name, opt))
    if not ag or any(not 0 <= d < n for d in ag):
        raise ValueError("%s.agents %r: agents must lie in [0, %d)" % (name, ag, n))
    return ag


def parse_deviation_options(opt, config):
    """training.greedy_deviation (true or a dict) -> the dict with every key filled in: agents (the deviators, default
    all), steps K, dev_len L, action ('best_response' or an index), horizon (None = deviation.default_horizon).
    Refuses a CAC agent and more than tuple_play.MAX_TUPLES tuples."""
    name = "training.greedy_deviation"
    ps, _ = tp.check_config(config)
    n = len(ps)
    noise = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        noise = opt.pop("noise")
        noise = None if noise is None or noise is False else parse_deviation_noise(noise, config)
    out = an.options("greedy_deviation", opt, dict(DEV_DEFAULTS, agents=list(range(n))))
    out["agents"] = _agents(name, out["agents"], n)
    out["steps"], out["dev_len"] = _int(name + ".steps", out["steps"]), _int(name + ".dev_len", out["dev_len"])
    if not 1 <= out["dev_len"] <= out["steps"] <= _lib.DEV_MAX_STEPS:
        raise ValueError("%s: needs 1 <= dev_len <= steps <= %d, got dev_len=%d steps=%d"
                         % (name, _lib.DEV_MAX_STEPS, out["dev_len"], out["steps"]))
    idx = dv.action_index(out["action"])
    if idx >= 0:
        acts = [ps[d][1] for d in out["agents"]]
        if idx >= min(acts):
            raise ValueError("%s.action=%d is not an action of every deviator (%s)" % (name, idx, acts))
    if out["horizon"] is not None:
        out["horizon"] = _int(name + ".horizon", out["horizon"])
        if not 1 <= out["horizon"] <= _lib.DEV_MAX_HORIZON:
            raise ValueError("%s.horizon=%d out of [1, %d]" % (name, out["horizon"], _lib.DEV_MAX_HORIZON))
    if noise is not None:
        out["noise"] = noise
    return out


def parse_deviation_noise(noise, config):
    """training.greedy_deviation.noise (true or a dict) -> the dict with every key filled in: deviation.parse_noise's
    noise_prob (None = the run's own noise, refused for a noise-free run), ret_tol, tol and max_iters, and resolution
    (tuple_stationary's uniform cuts of the price axis; more than its MAX_CELLS cells is refused before training)."""
    from . import tuple_stationary as ts
    name = "training.greedy_deviation.noise"
    out = an.options("greedy_deviation.noise", noise, DEV_NOISE_DEFAULTS)
    resolution = out.pop("resolution")
    try:
        out = dv.parse_noise(out, config)
    except ValueError as e:
        raise ValueError(str(e).replace("training.deviation.noise", name))
    out["resolution"] = ts._check_resolution(resolution, name + ".resolution")
    try:
        ts.cuts(config, out["resolution"])
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e))
    return out


def parse_equilibrium_options(opt, config):
    """training.greedy_equilibrium (true or a dict) -> the dict with every key filled in: agents (those solved, default
    all), tol, policies (store the per-state arrays).  Refuses a CAC agent, more than tuple_play.MAX_TUPLES tuples and,
    for the solved agents, a gamma outside [0, 1) in the config or in training.sweep.gamma."""
    name = "training.greedy_equilibrium"
    ps, _ = tp.check_config(config)
    n = len(ps)
    noise = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        noise = opt.pop("noise")
        noise = None if noise is None or noise is False else parse_equilibrium_noise(noise, config)
    out = an.options("greedy_equilibrium", opt, dict(EQ_DEFAULTS, agents=list(range(n))))
    out["agents"] = sorted(set(_agents(name, out["agents"], n)))
    if isinstance(out["tol"], bool) or not isinstance(out["tol"], (int, float, np.integer, np.floating)) \
            or not float(out["tol"]) >= 0.0:
        raise ValueError("%s.tol=%r must be a number >= 0" % (name, out["tol"]))
    out["tol"] = float(out["tol"])
    if not isinstance(out["policies"], (bool, np.bool_)):
        raise ValueError("%s.policies must be true or false, got %r" % (name, out["policies"]))
    out["policies"] = bool(out["policies"])
    sweep = (config.get("training") or {}).get("sweep") or {}
    gammas = _agent_gammas(config)
    for d in out["agents"]:
        try:
            if "gamma" in sweep:
                sg = np.asarray(sweep["gamma"], np.float64)
                eq.check_gamma(sg[d] if sg.ndim == 2 else sg, "sweep.gamma")
            else:
                eq.check_gamma([gammas[d]], "agents[%d].gamma" % d)
        except ValueError as e:
            raise ValueError(str(e).replace("training.equilibrium", name))
    if noise is not None:
        out["noise"] = noise
    return out


def parse_equilibrium_noise(noise, config):
    """training.greedy_equilibrium.noise (true or a dict) -> the dict with every key filled in: equilibrium.parse_noise's
    noise_prob (None = the run's own noise, refused for a noise-free run), eval_tol and max_sweeps, and resolution
    (tuple_stationary's uniform cuts of the price axis; more than its MAX_CELLS cells is refused before training)."""
    from . import tuple_stationary as ts
    name = "training.greedy_equilibrium.noise"
    out = an.options("greedy_equilibrium.noise", noise, NOISE_DEFAULTS)
    resolution = out.pop("resolution")
    try:
        out = eq.parse_noise(out, config)
    except ValueError as e:
        raise ValueError(str(e).replace("training.equilibrium.noise", name))
    out["resolution"] = ts._check_resolution(resolution, name + ".resolution")
    try:
        ts.cuts(config, out["resolution"])
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e))
    return out


def start_weights(weights, T, name="weights"):
    """float64 [T] or None: "uniform" = 1 / T per tuple, None = no start weights, else T finite numbers >= 0."""
    if weights is None:
        return None
    if isinstance(weights, str):
        if weights != "uniform":
            raise ValueError("%s must be 'uniform', null or %d numbers, got %r" % (name, T, weights))
        return np.full(T, 1.0 / float(T), np.float64)
    try:
        w = np.array(weights, np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be 'uniform', null or %d numbers, got %r" % (name, T, weights))
    if w.shape != (T,) or not np.isfinite(w).all() or (w < 0.0).any():
        raise ValueError("%s must hold %d finite numbers >= 0 (one per action tuple), got shape %s" % (name, T, w.shape))
    return np.ascontiguousarray(w)


def parse_attractor_options(opt, config):
    """training.greedy_attractors (true or a dict) -> the dict with every key filled in: policies (store the per-tuple
    arrays), weights ("uniform" = 1 / T per start tuple, null = none, or a list of T numbers >= 0).  Refuses a CAC agent
    and more than tuple_play.MAX_TUPLES tuples."""
    name = "training.greedy_attractors"
    _, T = tp.check_config(config)
    out = an.options("greedy_attractors", opt, ATTR_DEFAULTS)
    if not isinstance(out["policies"], (bool, np.bool_)):
        raise ValueError("%s.policies must be true or false, got %r" % (name, out["policies"]))
    out["policies"] = bool(out["policies"])
    w = start_weights(out["weights"], T, name + ".weights")
    if w is not None and not isinstance(out["weights"], str):
        out["weights"] = [float(x) for x in w]
    return out


# ---------------------------------------------------------------------------------------------- the device calls
def _gamma(batch):
    """The discount factors as a device tensor [N, G], or None when cfg.gamma is every agent's own: the per-game sweep
    when there is one, else (with a network in the game, whose table slot is a placeholder) the agents' own gammas."""
    import torch
    gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
    if gam is not None:
        return gam
    nn = getattr(batch, "nn", None)
    if not nn:
        return None
    g = np.array([float(nn[i].gamma) if i in nn else float(batch.cfg.gamma[i]) for i in range(batch.N)], np.float64)
    return torch.from_numpy(np.ascontiguousarray(np.repeat(g[:, None], batch.G, axis=1))).to(batch.device)


def _inputs(batch, tuple_policy, start, tabs):
    """(tabs, T, tuple_policy, start int32 [G], reward, scaled) on the batch's device."""
    import torch
    G, N = batch.G, batch.N
    tabs = tp._batch_tables(batch, tabs)
    T = int(tabs["T"])
    dev = batch.device
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    else:
        an.check_policy(batch, tuple_policy, (G, N, T), "tuple_analysis", "tuple_policy")
    with torch.cuda.device(dev):
        if start is None:
            t0 = tp.start_tuples(batch.state, tabs).contiguous()
        elif isinstance(start, torch.Tensor):
            t0 = start.to(device=dev, dtype=torch.int32).reshape(G).contiguous()
        else:
            t0 = torch.from_numpy(np.ascontiguousarray(np.asarray(start).reshape(G).astype(np.int32))).to(dev)
        d_rew = torch.from_numpy(np.ascontiguousarray(tabs["reward"], np.float64)).to(dev)
        d_sca = torch.from_numpy(np.ascontiguousarray(tabs["scaled"], np.float64)).to(dev)
    return tabs, T, tuple_policy, t0, d_rew, d_sca


def deviation(batch, deviator=0, steps=32, dev_len=1, action="best_response", horizon=None, start=None, rows=False,
              group_stats=None, tuple_policy=None, budget=dv.ROW_BUDGET, tabs=None):
    """thrl_tuple_deviation for every game of `batch` (a GameBatch, or a MixedGameBatch of QTable / Reinforce /
    ActorCritic agents): deviation.run's dict fields, from the strategies tuple_policy (a device int16 tensor [G, N, T] of
    tuple_play.extract(), default: extracted here) and the start tuples `start` int [G] (default: the tuple whose
    price is the game's state, -1 when there is none: that game is refused).  "start" [G] is returned too.  The rows
    are produced in tau-chunks of at most `budget` bytes per device buffer."""
    import torch
    G, N = batch.G, batch.N
    K, L = int(steps), int(dev_len)
    if not 0 <= int(deviator) < N:
        raise ThrlError("deviator %d out of [0, %d)" % (int(deviator), N))
    if group_stats is not None and group_stats.G != G:
        raise ThrlError("group_stats spec is for %d games, this batch has %d" % (group_stats.G, G))
    tabs, T, tuple_policy, t0, d_rew, d_sca = _inputs(batch, tuple_policy, start, tabs)
    H = dv.default_horizon([int(x) for x in tabs["n_actions"]]) if horizon is None else int(horizon)
    dev = batch.device
    a = _lib.TupleDeviationArgs()
    a.n_games, a.n_tuples, a.deviator, a.dev_len, a.n_steps, a.horizon = G, T, int(deviator), L, K, H
    a.dev_action = dv.action_index(action)
    with torch.cuda.device(dev):
        out = {f: torch.zeros((G,), dtype=torch.int32, device=dev) for f in dv.INT_FIELDS}
        out.update(cycle_reward=torch.zeros((N, G), dtype=torch.float64, device=dev),
                   cycle_action=torch.zeros((N, G), dtype=torch.float64, device=dev),
                   gain=torch.zeros((G,), dtype=torch.float64, device=dev))
        a.start, a.tuple_policy, a.reward, a.scaled = t0.data_ptr(), tuple_policy.data_ptr(), d_rew.data_ptr(), d_sca.data_ptr()
        gam = _gamma(batch)
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
            a.row_begin, a.row_count = (b0, k) if k else (0, 0)
            a.reward_rows = rr.data_ptr() if rr is not None else None
            a.action_rows = ra.data_ptr() if ra is not None else None
            _lib.check(batch.L.thrl_tuple_deviation(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                       "thrl_tuple_deviation")
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
        res["start"] = t0.cpu().numpy()
        res["horizon"] = H
        if rows:
            res["reward_rows"] = np.concatenate(host_r, axis=0) if host_r else np.zeros((0, N, G))
            res["action_rows"] = np.concatenate(host_a, axis=0) if host_a else np.zeros((0, N, G))
        if st is not None:
            from .group_stats import to_numpy
            res["group_stats"] = to_numpy(st)
    return res


def equilibrium(batch, agents=None, start=None, policies=False, tol=0.0, tuple_policy=None, tabs=None):
    """thrl_tuple_equilibrium for every game of `batch`: equilibrium.run's dict fields with n_states = T, plus "start"
    [G].  tuple_policy and start as in deviation(); a game without a start tuple gets mu = -1, lam = 0 and NaN in its
    on-path outputs (its flags br_on and nash are False).  policies=True adds br_policy (uint16), v_opt, v_pi [N, G, T]."""
    import torch
    G, N = batch.G, batch.N
    ag, mask = eq.agents_mask(agents, N)
    tabs, T, tuple_policy, t0, d_rew, _ = _inputs(batch, tuple_policy, start, tabs)
    dev = batch.device
    a = _lib.TupleEquilibriumArgs()
    a.n_games, a.n_tuples, a.agents = G, T, mask
    with torch.cuda.device(dev):
        gam = _gamma(batch)
        if gam is not None:
            sel = gam[ag]
            if not bool(((sel >= 0.0) & (sel < 1.0)).all()):
                raise ThrlError("equilibrium: every solved agent's gamma must lie in [0, 1)")
        out = an.outputs(dev, (("mu", "lam"), (G,), "int32"), (eq.INT_FIELDS, (N, G), "int32"),
                         (eq.FLOAT_FIELDS, (N, G), "float64"), (("br_policy",) if policies else (), (N, G, T), "int16"),
                         (("v_opt", "v_pi") if policies else (), (N, G, T), "float64"))
        a.start, a.tuple_policy, a.reward = t0.data_ptr(), tuple_policy.data_ptr(), d_rew.data_ptr()
        a.sweep_gamma = gam.data_ptr() if gam is not None else None
        an.bind(a, out)
        _lib.check(batch.L.thrl_tuple_equilibrium(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                   "thrl_tuple_equilibrium")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["start"] = t0.cpu().numpy()
    if policies:
        res["br_policy"] = res["br_policy"].view(np.uint16)
    res["agents"] = ag
    res["n_states"] = T
    res["tol"] = float(tol)
    res.update(eq.flags(res, ag, tol))
    return res


def attractors(batch, start=None, weights="uniform", policies=False, tuple_policy=None, tabs=None):
    """thrl_tuple_attractors for every game of `batch`: attractors.run's dict fields with the T tuples as the state set
    (n_states = T), start_mass [KEEP, G], start_mass_other [G] and start_reward [N, G] in place of the reset_* fields,
    plus "start" [G].  tuple_policy and start as in deviation(); a game without a start tuple has rep_x0 = mu_x0 =
    slot_x0 = -1.  weights: "uniform" (1 / T per start tuple), None (no start_* fields) or T numbers >= 0.
    policies=True adds tuple_rep, tuple_mu (uint16) [G, T]."""
    import torch
    G, N = batch.G, batch.N
    tabs, T, tuple_policy, t0, d_rew, d_sca = _inputs(batch, tuple_policy, start, tabs)
    w = start_weights(weights, T)
    dev = batch.device
    a = _lib.TupleAttractorsArgs()
    a.n_games, a.n_tuples = G, T
    with torch.cuda.device(dev):
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        out = {f: i32(G) for f in at.GAME_INT}
        out.update({f: i32(KEEP, G) for f in at.SLOT_INT})
        out.update({f: f64(KEEP, N, G) for f in at.SLOT_FLOAT})
        d_w = None
        if w is not None:
            d_w = torch.from_numpy(w).to(dev)
            a.start_w = d_w.data_ptr()
            out.update(start_mass=f64(KEEP, G), start_mass_other=f64(G), start_reward=f64(N, G))
        if policies:
            out["tuple_rep"] = torch.zeros((G, T), dtype=torch.int16, device=dev)
            out["tuple_mu"] = torch.zeros((G, T), dtype=torch.int16, device=dev)
        a.start, a.tuple_policy, a.reward, a.scaled = t0.data_ptr(), tuple_policy.data_ptr(), d_rew.data_ptr(), d_sca.data_ptr()
        an.bind(a, out)
        _lib.check(batch.L.thrl_tuple_attractors(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                   "thrl_tuple_attractors")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["start"] = t0.cpu().numpy()
    for f in TUPLE_FIELDS:
        if f in res:
            res[f] = res[f].view(np.uint16)
    res["n_states"] = T
    return res


def equilibrium_noise(batch, agents=None, noise_prob=None, resolution=NOISE_DEFAULTS["resolution"], eval_tol=1e-12,
                      max_sweeps=8192, policies=False, tol=0.0, tuple_policy=None, cell_policy=None, weights="stationary",
                      n_games=None, tabs=None):
    """thrl_tuple_equilibrium_noise for the first n_games (default all) games of `batch` (see
    AnalysisMethods.greedy_equilibrium_noise).  tabs: tuple_stationary.tables(batch.config, resolution).  tuple_policy /
    cell_policy: the strategies of tuple_play.extract() / tuple_stationary.extract_cells() (default: extracted here, once,
    for this call and for the stationary one).  weights="stationary": tuple_stationary.run(pi=True, start="reset", tol
    1e-12, at most 8192 steps) on the same tables and strategies gives pi [G, T]; a game whose iteration stopped at its
    step limit is weighted by its last iterate all the same, and a game that iteration did not solve by zeros.  Returns
    a dict of numpy arrays."""
    import torch
    from . import stationary as sn
    from . import tuple_stationary as ts
    N = batch.N
    G = an.games(batch, n_games, "greedy_equilibrium_noise")
    ag, mask = eq.agents_mask(agents, N)
    if tabs is None:
        tabs = ts.tables(batch.config, resolution)
    tp._batch_tables(batch, tabs)
    dev = batch.device
    J, T, W = int(tabs["n_cells"]), int(tabs["n_tuples"]), int(tabs["band_w"])
    S = T + J
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    if not an.is_policy(tuple_policy, (batch.G, N, T), batch.state.device):
        an.check_policy(batch, tuple_policy, (G, N, T), "greedy_equilibrium_noise", "tuple_policy")
    if cell_policy is None:
        cell_policy = ts.extract_cells(batch, tabs, n_games=G)
    an.check_policy(batch, cell_policy, (G, N, J), "greedy_equilibrium_noise", "cell_policy")
    a = _lib.TupleEquilibriumNoiseArgs()
    a.n_games, a.n_tuples, a.n_cells, a.band_w, a.agents = G, T, J, W, mask
    a.max_sweeps, a.eval_tol = int(max_sweeps), float(eval_tol)
    nn = getattr(batch, "nn", None) or {}
    for i, k in enumerate(tp._kinds(batch)):
        a.kind[i] = tp.KINDS[k]
        a.gamma[i] = float(nn[i].gamma) if i in nn else float(batch.cfg.gamma[i])
    with torch.cuda.device(dev):
        p, p_g = sn.resolve_noise(batch, noise_prob, G)
        pi = None
        if isinstance(weights, str):
            if weights != "stationary":
                raise ThrlError("greedy_equilibrium_noise: weights must be 'stationary', None or a [G, T] array, got %r"
                                % (weights,))
            st = ts.run(batch, noise_prob=noise_prob, start="reset", pi=True, tuple_policy=tuple_policy,
                        cell_policy=cell_policy, n_games=G, tabs=tabs)
            pi = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
        elif weights is not None:
            if isinstance(weights, torch.Tensor):
                pi = weights.to(device=dev, dtype=torch.float64).contiguous()
            else:
                pi = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, np.float64))).to(dev)
            if tuple(pi.shape) != (G, T):
                raise ThrlError("greedy_equilibrium_noise: weights must be shaped %s, got %s" % ((G, T), tuple(pi.shape)))
        keep = an.bind_tables(a, tabs, [("reward", (N, T), np.float64), ("band_lo", (T,), np.int32),
                                        ("band", (T, W), np.float64), ("noise_reward", (N, T), np.float64)],
                              dev, "greedy_equilibrium_noise")
        if p_g is not None:
            a.noise_prob_g = p_g.data_ptr()
        else:
            a.noise_prob = p
        gam = batch.sweep.get("gamma") if getattr(batch, "sweep", None) else None
        if gam is not None:
            gam = gam[:, :G].contiguous()
            a.sweep_gamma = gam.data_ptr()
        a.tuple_policy, a.cell_policy = tuple_policy.data_ptr(), cell_policy.data_ptr()
        if pi is not None:
            a.pi = pi.data_ptr()
        out = an.outputs(dev, (NOISE_INT, (N, G), "int32"), (NOISE_FLOAT, (N, G), "float64"),
                         (NOISE_WEIGHTED if pi is not None else (), (N, G), "float64"),
                         (("br_policy",) if policies else (), (N, G, S), "int16"),
                         (("v_opt", "v_pi") if policies else (), (N, G, S), "float64"))
        an.bind(a, out)
        _lib.check(batch.L.thrl_tuple_equilibrium_noise(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                   "thrl_tuple_equilibrium_noise")
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        res["noise_prob"] = np.full(G, p, np.float64) if p_g is None else p_g.cpu().numpy()
        if pi is not None:
            res["pi"] = pi.cpu().numpy()
    if policies:
        res["br_policy"] = res["br_policy"].view(np.uint16)
    res["agents"], res["n_cells"], res["T"], res["n_states"], res["tol"] = ag, J, T, S, float(tol)
    res["eval_tol"], res["max_sweeps"] = float(eval_tol), int(max_sweeps)
    res["resolution"] = int(tabs.get("resolution", resolution))
    res.update(eq.flags_noise(res, ag, tol))
    return res


def deviation_noise(batch, deviator=0, steps=32, dev_len=1, action="best_response", noise_prob=None,
                    resolution=DEV_NOISE_DEFAULTS["resolution"], ret_tol=1e-6, weights="stationary", rows=False,
                    group_stats=None, budget=dv.ROW_BUDGET, tuple_policy=None, cell_policy=None, n_games=None, tabs=None,
                    tol=1e-12, max_iters=8192):
    """thrl_tuple_deviation_noise for the first n_games (default all) games of `batch` (see
    AnalysisMethods.greedy_deviation_noise).  tabs: tuple_stationary.tables(batch.config, resolution).  tuple_policy /
    cell_policy: the strategies of tuple_play.extract() / tuple_stationary.extract_cells() (default: extracted here, once,
    for this call and for the stationary one).  weights="stationary": tuple_stationary.run(pi=True, start="reset", tol,
    max_iters) on the same tables and strategies gives m_0 [G, T]; a game whose iteration stopped at its step limit starts
    from its last iterate all the same, and a game that iteration did not solve is not solved here.  The rows are
    produced in tau-chunks of at most `budget` bytes per device buffer.  Returns a dict of numpy arrays."""
    import torch
    from . import stationary as sn
    from . import tuple_stationary as ts
    N = batch.N
    G = an.games(batch, n_games, "greedy_deviation_noise")
    K, L = int(steps), int(dev_len)
    if not 0 <= int(deviator) < N:
        raise ThrlError("deviator %d out of [0, %d)" % (int(deviator), N))
    if group_stats is not None and group_stats.G != G:
        raise ThrlError("group_stats spec is for %d games, this call has %d" % (group_stats.G, G))
    if tabs is None:
        tabs = ts.tables(batch.config, resolution)
    tp._batch_tables(batch, tabs)
    dev = batch.device
    J, T, W = int(tabs["n_cells"]), int(tabs["n_tuples"]), int(tabs["band_w"])
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    if not an.is_policy(tuple_policy, (batch.G, N, T), batch.state.device):
        an.check_policy(batch, tuple_policy, (G, N, T), "greedy_deviation_noise", "tuple_policy")
    if cell_policy is None:
        cell_policy = ts.extract_cells(batch, tabs, n_games=G)
    an.check_policy(batch, cell_policy, (G, N, J), "greedy_deviation_noise", "cell_policy")
    a = _lib.TupleDeviationNoiseArgs()
    a.n_games, a.n_tuples, a.n_cells, a.band_w = G, T, J, W
    a.deviator, a.dev_len, a.n_steps, a.dev_action = int(deviator), L, K, dv.action_index(action)
    a.ret_tol = float(ret_tol)
    for i, k in enumerate(tp._kinds(batch)):
        a.kind[i] = tp.KINDS[k]
    with torch.cuda.device(dev):
        p, p_g = sn.resolve_noise(batch, noise_prob, G)
        stat_iters = np.zeros(G, np.int32)
        if isinstance(weights, str):
            if weights != "stationary":
                raise ThrlError("greedy_deviation_noise: weights must be 'stationary' or a [G, T] array, got %r" % (weights,))
            st = ts.run(batch, noise_prob=noise_prob, start="reset", tol=tol, max_iters=max_iters, pi=True,
                        tuple_policy=tuple_policy, cell_policy=cell_policy, n_games=G, tabs=tabs)
            m0 = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
            stat_iters = np.asarray(st["iters"], np.int32)
            n_switch, unresolved = st["n_switch"], st["unresolved"]
        else:
            if weights is None:
                raise ThrlError("greedy_deviation_noise: weights must be 'stationary' or a [G, T] array, got None")
            if isinstance(weights, torch.Tensor):
                m0 = weights.to(device=dev, dtype=torch.float64).contiguous()
            else:
                m0 = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, np.float64))).to(dev)
            if tuple(m0.shape) != (G, T):
                raise ThrlError("greedy_deviation_noise: weights must be shaped %s, got %s" % ((G, T), tuple(m0.shape)))
            n_switch, unresolved = _switches(batch, tabs, cell_policy, G)
        keep = an.bind_tables(a, tabs, [("reward", (N, T), np.float64), ("scaled", (N, T), np.float64),
                                        ("band_lo", (T,), np.int32), ("band", (T, W), np.float64),
                                        ("noise_reward", (N, T), np.float64)], dev, "greedy_deviation_noise")
        if p_g is not None:
            a.noise_prob_g = p_g.data_ptr()
        else:
            a.noise_prob = p
        gam = _gamma(batch)
        if gam is not None:
            gam = gam[:, :G].contiguous()
            a.sweep_gamma = gam.data_ptr()
        a.tuple_policy, a.cell_policy, a.weights = tuple_policy.data_ptr(), cell_policy.data_ptr(), m0.data_ptr()
        out = an.outputs(dev, (dv.NOISE_AGENT, (N, G), "float64"), (dv.NOISE_FLOAT, (G,), "float64"),
                         (dv.NOISE_INT, (G,), "int32"))
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
            _lib.check(batch.L.thrl_tuple_deviation_noise(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                       "thrl_tuple_deviation_noise")
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
        del keep
    res["stat_iters"], res["n_switch"], res["unresolved"] = stat_iters, np.asarray(n_switch, np.int32), np.asarray(unresolved)
    res["n_cells"], res["T"], res["ret_tol"] = J, T, float(ret_tol)
    res["resolution"] = int(tabs.get("resolution", resolution))
    return res


def _switches(batch, tabs, cell_policy, G):
    """(n_switch int32 [G], unresolved [G]) of thrl_tuple_stationary's sampling diagnostics, on the host: the pairs of
    adjacent cells on which the clamped entry of some neural agent differs, and their share of the price axis, the
    widths added in ascending k from 0.0."""
    cp = cell_policy[:G].cpu().numpy().view(np.uint16).astype(np.int64)
    J = cp.shape[2]
    w = np.asarray(tabs["cell_w"], np.float64)
    flag = np.zeros((G, max(J - 1, 0)), bool)
    for i, k in enumerate(tp._kinds(batch)):
        if k != "QTable":
            e = np.minimum(cp[:, i], int(tabs["n_actions"][i]) - 1)
            flag |= e[:, :-1] != e[:, 1:]
    un = np.zeros(G)
    for k in range(J - 1):
        un = np.where(flag[:, k], un + 0.5 * (w[k] + w[k + 1]), un)
    return flag.sum(axis=1).astype(np.int32), un


# ---------------------------------------------------------------------------------------------- host side
def summarize_equilibrium_noise(games, ids, n_groups, agents, tol=0.0):
    """equilibrium.summarize_noise's rows (per (group, agent): games, capped, br_all, br_w, the quantiles of loss_all and
    loss_w over the games where they are positive, diff_w_mean, sweeps_max; per group: perfect) with, per agent,
    diff_tuples_mean and diff_cells_mean (the mean counts of differing tuple-states and cell-states over the solved
    games) added."""
    rows = eq.summarize_noise(games, ids, n_groups, agents, tol)
    ids = np.asarray(ids, np.int64).reshape(-1)
    iters = np.asarray(games["iters"])
    for r in rows:
        if r["agent"] is not None:
            ok = (ids == r["group"]) & (iters[r["agent"]] >= 0)
            r["diff_tuples_mean"] = an.mean(np.asarray(games["n_diff_tuples"])[r["agent"]][ok])
            r["diff_cells_mean"] = an.mean(np.asarray(games["n_diff_cells"])[r["agent"]][ok])
    return rows


def save_equilibrium_noise_games(d, r):
    """geqn_iters int32 [4, N, G] (iters, sweeps, n_diff_tuples, n_diff_cells), geqn_loss float64 [3, N, G] (loss_all,
    loss_tuples_mean, loss_cells_mean), geqn_prob float64 [G] (the noise probabilities analysed); with weights
    geqn_weighted float64 [3, N, G] (loss_w, diff_w, v_w); with per-state arrays geqn_policy uint16, geqn_v_opt and
    geqn_v_pi float64 [N, G, T + J], tuple-states first."""
    np.save(os.path.join(d, "geqn_iters.npy"), np.stack([r[f] for f in NOISE_INT]).astype(np.int32))
    np.save(os.path.join(d, "geqn_loss.npy"), np.stack([r[f] for f in NOISE_FLOAT]).astype(np.float64))
    np.save(os.path.join(d, "geqn_prob.npy"), np.asarray(r["noise_prob"], np.float64))
    if "loss_w" in r:
        np.save(os.path.join(d, "geqn_weighted.npy"), np.stack([r[f] for f in NOISE_WEIGHTED]).astype(np.float64))
    if "br_policy" in r:
        np.save(os.path.join(d, "geqn_policy.npy"), np.asarray(r["br_policy"], np.uint16))
        np.save(os.path.join(d, "geqn_v_opt.npy"), np.asarray(r["v_opt"], np.float64))
        np.save(os.path.join(d, "geqn_v_pi.npy"), np.asarray(r["v_pi"], np.float64))


def load_equilibrium_noise_games(d):
    """The per-game arrays of the check under noise a run directory holds (training.greedy_equilibrium.noise)."""
    it, loss = np.load(os.path.join(d, "geqn_iters.npy")), np.load(os.path.join(d, "geqn_loss.npy"))
    g = {f: it[k] for k, f in enumerate(NOISE_INT)}
    g.update({f: loss[k] for k, f in enumerate(NOISE_FLOAT)})
    g["noise_prob"] = np.load(os.path.join(d, "geqn_prob.npy"))
    if os.path.isfile(os.path.join(d, "geqn_weighted.npy")):
        w = np.load(os.path.join(d, "geqn_weighted.npy"))
        g.update({f: w[k] for k, f in enumerate(NOISE_WEIGHTED)})
    if os.path.isfile(os.path.join(d, "geqn_policy.npy")):
        g.update(br_policy=np.load(os.path.join(d, "geqn_policy.npy")), v_opt=np.load(os.path.join(d, "geqn_v_opt.npy")),
                 v_pi=np.load(os.path.join(d, "geqn_v_pi.npy")))
    return g


def summarize_deviation_noise(games, ids, n_groups, deviators):
    """deviation.summarize_noise's rows (one per (group, deviator)) with n_switch_max and unresolved_mean over the
    group's games (solved or not: they describe the sampling of the strategies, not the chain) added."""
    rows = dv.summarize_noise(games, ids, n_groups, deviators)
    ids = np.asarray(ids, np.int64).reshape(-1)
    for r in rows:
        g = games[r["deviator"]]
        m = ids == r["group"]
        r["n_switch_max"] = int(np.asarray(g["n_switch"])[m].max()) if m.any() else None
        r["unresolved_mean"] = an.mean(np.asarray(g["unresolved"], np.float64)[m])
    return rows


def save_deviation_noise_games(d, deviator, r):
    """gdevn<d>_games float64 [6, G] (dev_share, gain, gain_dev, low, dist, mass), gdevn<d>_steps int32 [2, G] (low_step,
    ret_step), gdevn<d>_base float64 [2, N, G] (base_reward, base_action); gdevn_prob [G] (the noise probabilities
    analysed), gdevn_stat int32 [2, G] (the stationary iteration behind the weights: iters, n_switch) and
    gdevn_unresolved [G] are the same for every deviator."""
    np.save(os.path.join(d, "gdevn%d_games.npy" % deviator), np.stack([r[f] for f in dv.NOISE_FLOAT]).astype(np.float64))
    np.save(os.path.join(d, "gdevn%d_steps.npy" % deviator), np.stack([r[f] for f in dv.NOISE_INT]).astype(np.int32))
    np.save(os.path.join(d, "gdevn%d_base.npy" % deviator), np.stack([r[f] for f in dv.NOISE_AGENT]).astype(np.float64))
    np.save(os.path.join(d, "gdevn_prob.npy"), np.asarray(r["noise_prob"], np.float64))
    np.save(os.path.join(d, "gdevn_stat.npy"), np.stack([r["stat_iters"], r["n_switch"]]).astype(np.int32))
    np.save(os.path.join(d, "gdevn_unresolved.npy"), np.asarray(r["unresolved"], np.float64))


def load_deviation_noise_games(d, deviator):
    """The per-game arrays of the test under noise a run directory holds for `deviator` (training.greedy_deviation.noise)."""
    gm = np.load(os.path.join(d, "gdevn%d_games.npy" % deviator))
    st = np.load(os.path.join(d, "gdevn%d_steps.npy" % deviator))
    base = np.load(os.path.join(d, "gdevn%d_base.npy" % deviator))
    g = {f: gm[k] for k, f in enumerate(dv.NOISE_FLOAT)}
    g.update({f: st[k] for k, f in enumerate(dv.NOISE_INT)})
    g.update({f: base[k] for k, f in enumerate(dv.NOISE_AGENT)})
    g["noise_prob"] = np.load(os.path.join(d, "gdevn_prob.npy"))
    stat = np.load(os.path.join(d, "gdevn_stat.npy"))
    g["stat_iters"], g["n_switch"] = stat[0], stat[1]
    g["unresolved"] = np.load(os.path.join(d, "gdevn_unresolved.npy"))
    return g


def write_deviation_noise(exp_path, batch, config, opt, ids, n_groups, spec=None, histograms=False, budget=dv.ROW_BUDGET,
                          tuple_policy=None):
    """The outputs of the option "noise" of training.greedy_deviation: per deviator gdevn<d>_games / _steps / _base.npy,
    gdevn_prob / gdevn_stat / gdevn_unresolved.npy (save_deviation_noise_games), gdevn<d>_*.npy group statistics of the
    response curves with a spec, and greedy_deviation_noise.json.  The cells' strategies and the long-run distribution
    are computed once for all deviators."""
    from . import trainer
    from . import tuple_stationary as ts
    nz = opt["noise"]
    tabs = ts.tables(config, nz["resolution"])
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    cell_policy = ts.extract_cells(batch, tabs)
    st = ts.run(batch, noise_prob=nz["noise_prob"], start="reset", tol=nz["tol"], max_iters=nz["max_iters"], pi=True,
                tuple_policy=tuple_policy, cell_policy=cell_policy, tabs=tabs)
    games = {}
    for d in opt["agents"]:
        r = deviation_noise(batch, deviator=d, steps=opt["steps"], dev_len=opt["dev_len"], action=opt["action"],
                            noise_prob=nz["noise_prob"], ret_tol=nz["ret_tol"], weights=st["pi"], group_stats=spec,
                            budget=budget, tuple_policy=tuple_policy, cell_policy=cell_policy, tabs=tabs)
        r.update(stat_iters=np.asarray(st["iters"], np.int32), n_switch=st["n_switch"], unresolved=st["unresolved"])
        games[d] = r
        save_deviation_noise_games(exp_path, d, r)
        if spec is not None:
            trainer.save_group_stats(exp_path, "gdevn%d" % d, r["group_stats"], spec, histograms)
    first = games[opt["agents"][0]]
    an.save_json(os.path.join(exp_path, "greedy_deviation_noise.json"),
                 {"options": opt, "n_cells": int(first["n_cells"]), "T": int(first["T"]), "quantiles": list(dv.QUANTILES),
                  "summary": summarize_deviation_noise(games, ids, n_groups, opt["agents"])})
    return games


def _no_start(rows, start, ids):
    ids = np.asarray(ids, np.int64).reshape(-1)
    start = np.asarray(start).reshape(-1)
    for r in rows:
        r["no_start"] = int(np.sum((ids == r["group"]) & (start < 0)))
    return rows


def summarize_deviation(games, ids, n_groups, nash, cartel, deviator):
    """deviation.summarize's rows for one deviator with no_start (the group's refused games; they count under games
    with lam = 0 and gain = 0) added.  games also holds start [G]."""
    return _no_start(dv.summarize(games, ids, n_groups, nash, cartel, deviator), games["start"], ids)


def summarize_equilibrium(games, ids, n_groups, agents, tol=0.0, delta=None):
    """equilibrium.summarize's rows with no_start added (those games have NaN on-path losses: not a best response on a
    path they do not have).  games also holds start [G]."""
    return _no_start(eq.summarize(games, ids, n_groups, agents, tol, delta), games["start"], ids)


def _as_reset(games):
    """games with the start_* fields under attractors.py's reset_* names (its gains() and summarize() read those)."""
    g = dict(games)
    for f in START_FIELDS:
        if f in g:
            g["reset" + f[5:]] = g[f]
    return g


def attractor_gains(games, nash, cartel):
    """attractors.gains on the tuple form's arrays: per-game profit gains train, largest and start (None without the
    start weights)."""
    gn = at.gains(_as_reset(games), nash, cartel)
    return {"train": gn["train"], "largest": gn["largest"], "start": gn["reset"]}


def summarize_attractors(games, ids, n_groups, nash, cartel):
    """attractors.summarize's rows with delta_reset_mean named delta_start_mean (the gain in expectation over the start
    weights), train_mass_* the training attractor's share of the start weights, luck_mean against the start-expected
    gain, and no_start added (those games have no training attractor: they count under games only).  games also holds
    start [G]."""
    rows = []
    for r in at.summarize(_as_reset(games), ids, n_groups, nash, cartel):
        rows.append({("delta_start_mean" if k == "delta_reset_mean" else k): v for k, v in r.items()})
    return _no_start(rows, games["start"], ids)


def load_deviation_games(d, deviator):
    """The per-game arrays a run directory holds for `deviator` (training.greedy_deviation)."""
    cyc = np.load(os.path.join(d, "gdev_cycle.npy"))
    post = np.load(os.path.join(d, "gdev%d_post.npy" % deviator))
    return {"mu": cyc[0], "lam": cyc[1], "start": cyc[2], "mu_post": post[0], "lam_post": post[1], "ret_step": post[2],
            "act_dev": post[3], "gain": np.load(os.path.join(d, "gdev%d_gain.npy" % deviator)),
            "cycle_reward": np.load(os.path.join(d, "gdev_cycle_reward.npy")),
            "cycle_action": np.load(os.path.join(d, "gdev_cycle_action.npy"))}


def load_equilibrium_games(d):
    """The per-game arrays a run directory holds (training.greedy_equilibrium)."""
    cyc, diff, loss = (np.load(os.path.join(d, "geq_%s.npy" % f)) for f in ("cycle", "diff", "loss"))
    g = {"mu": cyc[0], "lam": cyc[1], "start": cyc[2], "iters": np.load(os.path.join(d, "geq_iters.npy")),
         "n_diff_all": diff[0], "n_diff_on": diff[1], "loss_all": loss[0], "loss_on": loss[1], "loss_all_mean": loss[2],
         "loss_on_mean": loss[3], "v_on": np.load(os.path.join(d, "geq_value.npy"))}
    if os.path.isfile(os.path.join(d, "geq_policy.npy")):
        g.update(br_policy=np.load(os.path.join(d, "geq_policy.npy")), v_opt=np.load(os.path.join(d, "geq_v_opt.npy")),
                 v_pi=np.load(os.path.join(d, "geq_v_pi.npy")))
    return g


def save_attractor_games(d, r):
    """gattr_games int32 [6, G], gattr_slots int32 [3, KEEP, G], gattr_cycle float64 [2, KEEP, N, G] (attractors.
    save_games' shapes and orders), gattr_start int32 [G]; with start weights gattr_start_mass [KEEP + 1, G] (the slots,
    then the attractors not kept) and gattr_start_reward [N, G]; with per-tuple arrays gattr_state uint16 [2, G, T]
    (rep, mu)."""
    np.save(os.path.join(d, "gattr_games.npy"), np.stack([r[f] for f in at.GAME_INT]).astype(np.int32))
    np.save(os.path.join(d, "gattr_slots.npy"), np.stack([r[f] for f in at.SLOT_INT]).astype(np.int32))
    np.save(os.path.join(d, "gattr_cycle.npy"), np.stack([r[f] for f in at.SLOT_FLOAT]).astype(np.float64))
    np.save(os.path.join(d, "gattr_start.npy"), np.asarray(r["start"], np.int32))
    if "start_mass" in r:
        np.save(os.path.join(d, "gattr_start_mass.npy"),
                np.concatenate([r["start_mass"], np.asarray(r["start_mass_other"])[None]]).astype(np.float64))
        np.save(os.path.join(d, "gattr_start_reward.npy"), np.asarray(r["start_reward"], np.float64))
    if "tuple_rep" in r:
        np.save(os.path.join(d, "gattr_state.npy"), np.stack([r["tuple_rep"], r["tuple_mu"]]).astype(np.uint16))


def load_attractor_games(d):
    """The per-game arrays a run directory holds (training.greedy_attractors)."""
    gm, sl, cy = (np.load(os.path.join(d, "gattr_%s.npy" % f)) for f in ("games", "slots", "cycle"))
    g = {f: gm[k] for k, f in enumerate(at.GAME_INT)}
    g.update({f: sl[k] for k, f in enumerate(at.SLOT_INT)})
    g.update({f: cy[k] for k, f in enumerate(at.SLOT_FLOAT)})
    g["start"] = np.load(os.path.join(d, "gattr_start.npy"))
    if os.path.isfile(os.path.join(d, "gattr_start_mass.npy")):
        sm = np.load(os.path.join(d, "gattr_start_mass.npy"))
        g.update(start_mass=sm[:-1], start_mass_other=sm[-1],
                 start_reward=np.load(os.path.join(d, "gattr_start_reward.npy")))
    if os.path.isfile(os.path.join(d, "gattr_state.npy")):
        st = np.load(os.path.join(d, "gattr_state.npy"))
        g.update(tuple_rep=st[0], tuple_mu=st[1])
    return g


def write_attractors(exp_path, batch, config, opt, ids, n_groups, tuple_policy=None):
    """train_one's training.greedy_attractors outputs: the gattr_*.npy files (save_attractor_games) and
    greedy_attractors.json."""
    tabs = tp.tables(config)
    r = attractors(batch, weights=opt["weights"], policies=opt["policies"], tuple_policy=tuple_policy, tabs=tabs)
    save_attractor_games(exp_path, r)
    nash, cartel = dv.optimal(config)
    summary = summarize_attractors(r, ids, n_groups, nash, cartel)
    label = UNIFORM_LABEL if opt["weights"] == "uniform" else ("none" if opt["weights"] is None else "given per tuple")
    an.save_json(os.path.join(exp_path, "greedy_attractors.json"),
                 {"options": opt, "n_states": int(r["n_states"]), "keep": KEEP, "nash": nash, "cartel": cartel,
                  "quantiles": list(at.QUANTILES), "start_weights": label, "summary": summary})
    return r


def write_deviation(exp_path, batch, config, opt, ids, n_groups, spec=None, histograms=False, budget=dv.ROW_BUDGET,
                    tuple_policy=None):
    """train_one's training.greedy_deviation outputs, with the shapes of deviation.write_artefacts': gdev_cycle.npy int32
    [3, G] (mu, lam, start), gdev_cycle_reward / gdev_cycle_action [N, G], per deviator gdev<d>_post.npy int32 [4, G]
    (mu_post, lam_post, ret_step, act_dev) and gdev<d>_gain.npy [G], gdev<d>_*.npy group statistics with a spec, and
    greedy_deviation.json; with the option "noise" the test under demand noise after them (write_deviation_noise).
    Returns the last deviator's per-game arrays."""
    from . import trainer
    nash, cartel = dv.optimal(config)
    tabs = tp.tables(config)
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    summary = []
    for d in opt["agents"]:
        r = deviation(batch, deviator=d, steps=opt["steps"], dev_len=opt["dev_len"], action=opt["action"],
                      horizon=opt["horizon"], group_stats=spec, budget=budget, tuple_policy=tuple_policy, tabs=tabs)
        if d == opt["agents"][0]:
            np.save(os.path.join(exp_path, "gdev_cycle.npy"), np.stack([r["mu"], r["lam"], r["start"]]).astype(np.int32))
            np.save(os.path.join(exp_path, "gdev_cycle_reward.npy"), r["cycle_reward"])
            np.save(os.path.join(exp_path, "gdev_cycle_action.npy"), r["cycle_action"])
        np.save(os.path.join(exp_path, "gdev%d_post.npy" % d),
                np.stack([r["mu_post"], r["lam_post"], r["ret_step"], r["act_dev"]]).astype(np.int32))
        np.save(os.path.join(exp_path, "gdev%d_gain.npy" % d), r["gain"])
        if spec is not None:
            trainer.save_group_stats(exp_path, "gdev%d" % d, r["group_stats"], spec, histograms)
        summary += summarize_deviation(r, ids, n_groups, nash, cartel, d)
    an.save_json(os.path.join(exp_path, "greedy_deviation.json"),
                 dict(dv.describe(dict(opt, horizon_used=int(r["horizon"])), nash, cartel, summary), T=int(tabs["T"])))
    if opt.get("noise"):        # the test under demand noise after it; what is above is what it is without the option
        write_deviation_noise(exp_path, batch, config, opt, ids, n_groups, spec=spec, histograms=histograms, budget=budget,
                              tuple_policy=tuple_policy)
    return dict(r, full_cycle=opt["horizon"] is None)


def write_equilibrium(exp_path, batch, config, opt, ids, n_groups, tuple_policy=None, deviation=None):
    """train_one's training.greedy_equilibrium outputs, with the shapes of equilibrium.save_games': geq_cycle.npy int32
    [3, G] (mu, lam, start), geq_iters [N, G], geq_diff [2, N, G], geq_loss [4, N, G], geq_value [N, G], with
    policies geq_policy, geq_v_opt, geq_v_pi [N, G, T], and greedy_equilibrium.json.  deviation: what write_deviation
    returned for the same strategies and starts; with the full cycle (no horizon) its cycle rewards serve the collusive
    fractions, else one thrl_tuple_walk finds them."""
    tabs = tp.tables(config)
    if tuple_policy is None:
        tuple_policy = tp.extract(batch, tabs)
    r = equilibrium(batch, agents=opt["agents"], policies=opt["policies"], tol=opt["tol"], tuple_policy=tuple_policy,
                    tabs=tabs)
    np.save(os.path.join(exp_path, "geq_cycle.npy"), np.stack([r["mu"], r["lam"], r["start"]]).astype(np.int32))
    np.save(os.path.join(exp_path, "geq_iters.npy"), np.asarray(r["iters"], np.int32))
    np.save(os.path.join(exp_path, "geq_diff.npy"), np.stack([r["n_diff_all"], r["n_diff_on"]]).astype(np.int32))
    np.save(os.path.join(exp_path, "geq_loss.npy"),
            np.stack([r["loss_all"], r["loss_on"], r["loss_all_mean"], r["loss_on_mean"]]).astype(np.float64))
    np.save(os.path.join(exp_path, "geq_value.npy"), np.asarray(r["v_on"], np.float64))
    if "br_policy" in r:
        np.save(os.path.join(exp_path, "geq_policy.npy"), np.asarray(r["br_policy"], np.uint16))
        np.save(os.path.join(exp_path, "geq_v_opt.npy"), np.asarray(r["v_opt"], np.float64))
        np.save(os.path.join(exp_path, "geq_v_pi.npy"), np.asarray(r["v_pi"], np.float64))
    if deviation is not None and deviation["full_cycle"]:    # the cycle the equilibrium check's path ends in
        cycle_reward = deviation["cycle_reward"]
    else:
        cycle_reward = tp.run(batch, start=r["start"], tuple_policy=tuple_policy, tabs=tabs)["cycle_reward"]
    nash, cartel = dv.optimal(config)
    delta = np.where(r["lam"] > 0, dv.profit_gain(cycle_reward, nash, cartel), -np.inf)      # no path: not collusive
    summary = summarize_equilibrium(r, ids, n_groups, opt["agents"], opt["tol"], delta)
    an.save_json(os.path.join(exp_path, "greedy_equilibrium.json"), eq.describe(opt, r["n_states"], summary))
    if opt.get("noise"):        # the check under demand noise after it; what is above is what it is without the option
        from . import tuple_stationary as ts
        nz = opt["noise"]
        rn = equilibrium_noise(batch, agents=opt["agents"], noise_prob=nz["noise_prob"], eval_tol=nz["eval_tol"],
                               max_sweeps=nz["max_sweeps"], policies=opt["policies"], tol=opt["tol"],
                               tuple_policy=tuple_policy, tabs=ts.tables(config, nz["resolution"]))
        save_equilibrium_noise_games(exp_path, rn)
        rows = summarize_equilibrium_noise(rn, ids, n_groups, opt["agents"], opt["tol"])
        an.save_json(os.path.join(exp_path, "greedy_equilibrium_noise.json"),
                     {"options": opt, "n_cells": int(rn["n_cells"]), "T": int(rn["T"]), "quantiles": list(an.QUANTILES),
                      "summary": [x for x in rows if x["agent"] is not None],
                      "perfect": [x for x in rows if x["agent"] is None]})
    return r
