"""Sampled play: the DEVIATION TEST -- the expected impulse response of the agents' stochastic policies to a forced
deviation of one of them (thrl_sampled_deviation, include/thrl_sampled_deviation.h).

sampled_play says what the stochastic policies earn in the long run and sampled_response what each agent gives up against
rivals that sample.  This module asks the question that separates collusion from failure to learn: if one agent departs
from its policy for a few periods, do the others' SAMPLED policies punish it, how deep is the punishment, how long until
play is back, and was the departure profitable?  greedy_deviation answers it for the argmax strategies only; a softmax
that spreads its mass is not its argmax.

No episodes are sampled.  The tuple played is a Markov chain on the T action tuples whose row depends on the tuple only
through its price; run() propagates a distribution through that chain, dev_len periods with the deviator's policy replaced
by a deterministic strategy of the price (a fixed action, the one-period best response to the rivals' mixed policies, the
patient best reply of sampled_response, or any strategy given), then steps - dev_len plain periods, and returns per game
(definitions in the header) base_reward, base_action [N, G], base_price, dev_share, gain, gain_dev, low, low_step,
ret_step, dist, mass [G], optionally the rows of every period.  Noise-free play only; the version under demand noise is
the follow-up.

In train_one the analysis is the sub-key "deviation" of training.sampled_play, beside "response": true, or {"agents",
"steps", "dev_len", "action", "ret_tol"}.  It writes sampled_deviation.json, sdev_*.npy and sdev<d>_*.npy per deviator
(with training.group_stats also the response curves' statistics under the same prefix); utils.sampled_deviation_summary
and utils.sampled_deviation_games read them.  Sharded runs (th_rl_amd.launch) are out of scope, as sampled_play is.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from . import deviation as dv
from . import sampled_play as sp
from . import tuple_play as tp
from ._lib import ThrlError

DEFAULTS = dict(agents=None, steps=32, dev_len=1, action="best_response", ret_tol=1e-6)
NOISE_FOLLOW_UP = ("the deviation test of sampled play under demand noise is the follow-up of the noise-free one and not built "
                   "yet: drop \"noise\" or \"deviation\"")
MAX_LDS = _lib.SD_MAX_LDS
ACTIONS = ("best_response", "best_reply")
AGENT = ("base_reward", "base_action")
FLOAT = ("base_price", "dev_share", "gain", "gain_dev", "low", "dist", "mass")
INT = ("low_step", "ret_step")
PER_GAME = AGENT + FLOAT + INT + ("gamma", "epsilon", "stat_iters", "solved")


def parse_options(opt, config):
    """training.sampled_play.deviation (true or a dict) -> the dict with every key filled in: agents (the deviators,
    default all), steps K, dev_len L (1 <= L <= K <= DEV_MAX_STEPS), action ("best_response", "best_reply" = the patient
    best reply of sampled_response, or an action index of every deviator), ret_tol (>= 0).  Refuses a working set above a
    CU's LDS."""
    name = "training.sampled_play.deviation"
    out = an.options("sampled_play.deviation", opt, DEFAULTS)
    n = len(config["agents"])
    ag = list(range(n)) if out["agents"] is None else out["agents"]
    if not isinstance(ag, (list, tuple)) or not ag or any(isinstance(d, bool) or not isinstance(d, int) or not 0 <= d < n
                                                          for d in ag):
        raise ValueError("%s.agents must be a non-empty list of agents in [0, %d), got %r" % (name, n, ag))
    out["agents"] = sorted(set(ag))
    for f in ("steps", "dev_len"):
        if isinstance(out[f], bool) or not isinstance(out[f], int):
            raise ValueError("%s.%s must be an integer, got %r" % (name, f, out[f]))
    if not 1 <= out["dev_len"] <= out["steps"] <= _lib.DEV_MAX_STEPS:
        raise ValueError("%s: needs 1 <= dev_len <= steps <= %d, got dev_len=%d steps=%d"
                         % (name, _lib.DEV_MAX_STEPS, out["dev_len"], out["steps"]))
    if out["action"] not in ACTIONS:
        idx = dv.action_index(out["action"])
        acts = [int(dict(_lib.QTABLE_DEFAULTS, **config["agents"][d])["actions"]) for d in out["agents"]]
        if idx >= min(acts):
            raise ValueError("%s.action=%d is not an action of every deviator (%s)" % (name, idx, acts))
    t = out["ret_tol"]
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0.0:
        raise ValueError("%s.ret_tol must be a number >= 0, got %r" % (name, t))
    out["ret_tol"] = float(t)
    ws = working_set(config)
    if not ws["fits"]:
        raise ValueError("%s: a game's working set is %d bytes (T=%d, D=%d), a CU's LDS holds %d"
                         % (name, ws["bytes"], ws["T"], ws["D"], MAX_LDS))
    return out


def working_set(config, tabs=None):
    """The LDS bytes one game takes in thrl_sampled_deviation, by include/thrl_sampled_deviation.h's formula (sd_layout):
    sampled_play.working_set's sum + r16(2 D) + r16(8 D) + 512.  Returns dict(bytes, T, D, fits)."""
    tabs = sp.tables(config) if tabs is None else tabs
    ws = sp.working_set(config, tabs)
    D = int(ws["D"])
    b = int(ws["bytes"]) + sp._r16(2 * D) + sp._r16(8 * D) + 512
    return dict(bytes=int(b), T=int(ws["T"]), D=D, fits=b <= MAX_LDS)


def _to_device(x, dev, dtype):
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    x = np.asarray(x)
    if x.dtype.kind in "iub":                            # (torch takes no uint16 array)
        x = x.astype(np.int64)
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype).contiguous()


def run(batch, deviator=0, steps=32, dev_len=1, action="best_response", epsilon="current", gamma=None, ret_tol=1e-6,
        weights="stationary", rows=False, group_stats=None, budget=None, n_games=None, probs=None, dpolicy=None, tabs=None,
        tol=1e-12, max_iters=8192):
    """thrl_sampled_deviation for the first n_games (default all) games of `batch` (a MixedGameBatch of QTable / Reinforce
    / ActorCritic agents, or a GameBatch).  action: "best_response" (the one-period best response to the rivals' mixed
    policies), an action index, "best_reply" (sampled_response.run(agents=[deviator], policies=True) on the same rows and
    its br_policy; a game that call left unsolved is not solved here: zeros, -1 in the steps, zeros in its rows) or a
    [G, D] array of actions per distinct price.  epsilon: sampled_play's rules.  gamma: sampled_response.resolve_gamma's (None = the
    deviator's own, the per-game sweep where there is one).  weights: "stationary" = sampled_play.run(pi=True, tol,
    max_iters) on the same rows -- a game whose iteration stopped at its step limit starts from its last iterate all the
    same, and a game that call did not solve is not solved here -- or an array [G, T].  rows=True adds reward_rows,
    action_rows [steps, N, G], price_rows and dist_rows [steps, G]; group_stats (a GroupSpec): reward_rows / action_rows are
    reduced on the device; both produced in tau-chunks of at most `budget` bytes per device buffer.  probs, dpolicy, tabs as
    in sampled_play.run.  Returns a dict of numpy arrays."""
    import torch
    from . import sampled_response as sr
    from . import tuple_stationary as ts
    N = batch.N
    G = sp._games(batch, n_games)
    K, L, d = int(steps), int(dev_len), int(deviator)
    if not 0 <= d < N:
        raise ThrlError("deviator %d out of [0, %d)" % (d, N))
    if group_stats is not None and group_stats.G != G:
        raise ThrlError("group_stats spec is for %d games, this call has %d" % (group_stats.G, G))
    budget = dv.ROW_BUDGET if budget is None else int(budget)
    if tabs is None:
        tabs = sp.tables(batch.config)
    tp._batch_tables(batch, tabs)
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    ws = working_set(batch.config, tabs)
    if not ws["fits"]:                                   # what the call answers from the shape alone
        err = ThrlError("thrl_sampled_deviation refused (thrl_err %d): %d bytes of LDS per game (T=%d, n_prices=%d), at most %d"
                        % (_lib.ERR_UNSUPPORTED, ws["bytes"], T, D, MAX_LDS))
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    kinds = tp._kinds(batch)
    dev = batch.device
    a = _lib.SampledDeviationArgs()
    a.n_games, a.n_tuples, a.n_prices = G, T, D
    a.deviator, a.dev_len, a.n_steps, a.ret_tol = d, L, K, float(ret_tol)
    given = not isinstance(action, str) and (hasattr(action, "dim") or np.ndim(action) == 2)
    a.dev_action = -1 if given or action in ACTIONS else dv.action_index(action)
    for i, k in enumerate(kinds):
        a.kind[i] = tp.KINDS[k]
    with torch.cuda.device(dev):
        eps, eps_g = sp.resolve_epsilon(batch, epsilon, G)
        gam, gam_g = sr.resolve_gamma(batch, gamma, G)
        for i in range(N):
            a.eps[i] = eps[i]
        a.gamma = gam[d]
        if eps_g is not None:
            a.eps_g = eps_g.data_ptr()
        if gam_g is not None:
            a.sweep_gamma = gam_g.data_ptr()
        if probs is None:
            probs = sp.price_probs(batch, tabs["dprice"], n_games=G)
        if dpolicy is None:
            dpolicy = ts.price_policy(batch, tabs["dprice"], n_games=G)
        an.check_policy(batch, dpolicy, (G, N, D), "sampled_deviation", "dpolicy")
        sp.bind_rows(batch, kinds, G, "sampled_deviation", ("probs", probs, D, a.prob))
        a.dpolicy = dpolicy.data_ptr()
        e = epsilon if eps_g is None else eps_g
        stat_iters = np.zeros(G, np.int32)
        if isinstance(weights, str):
            if weights != "stationary":
                raise ThrlError("sampled_deviation: weights must be 'stationary' or a [G, T] array, got %r" % (weights,))
            st = sp.run(batch, epsilon=e, tol=tol, max_iters=max_iters, pi=True, n_games=G, probs=probs, dpolicy=dpolicy, tabs=tabs)
            x0 = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
            stat_iters = np.asarray(st["iters"], np.int32)
        else:
            if weights is None:
                raise ThrlError("sampled_deviation: weights must be 'stationary' or a [G, T] array, got None")
            x0 = _to_device(weights, dev, torch.float64)
            if tuple(x0.shape) != (G, T):
                raise ThrlError("sampled_deviation: weights must be shaped %s, got %s" % ((G, T), tuple(x0.shape)))
        a.weights = x0.data_ptr()
        dev_policy = unsolved = None
        if given:
            dev_policy = _to_device(action, dev, torch.int16)
            if tuple(dev_policy.shape) != (G, D):
                raise ThrlError("sampled_deviation: a strategy given as action must be shaped %s, got %s"
                                % ((G, D), tuple(dev_policy.shape)))
        elif action == "best_reply":
            br = sr.run(batch, agents=[d], epsilon=e, gamma=gamma, policies=True, pi=False, n_games=G, probs=probs,
                        dpolicy=dpolicy, tabs=tabs)
            dev_policy = torch.from_numpy(np.ascontiguousarray(br["br_policy"][d]).view(np.int16)).to(dev)
            if (br["iters"][d] < 0).any():               # not solved there: not solved here
                unsolved = torch.from_numpy(np.flatnonzero(br["iters"][d] < 0)).to(dev)
        if dev_policy is not None:
            a.flags = _lib.SD_POLICY
            a.dev_policy = dev_policy.data_ptr()
        keep = an.bind_tables(a, tabs, [("grp_first", (D + 1,), np.int32), ("grp_perm", (T,), np.int32),
                                        ("reward", (N, T), np.float64), ("scaled", (N, T), np.float64),
                                        ("price", (T,), np.float64)], dev, "sampled_deviation")
        out = an.outputs(dev, (AGENT, (N, G), "float64"), (FLOAT, (G,), "float64"), (INT, (G,), "int32"))
        an.bind(a, out)
        want = bool(rows) or group_stats is not None
        chunk = max(1, min(K, budget // (8 * N * G))) if want else K
        st = group_stats.zeros(K, dev) if group_stats is not None else None
        host = {f: [] for f in ("reward_rows", "action_rows", "price_rows", "dist_rows")}
        b0 = 0
        while True:
            k = min(chunk, K - b0) if want else 0
            buf = {}
            if k:
                buf["reward_rows"] = torch.empty((k, N, G), dtype=torch.float64, device=dev)
                buf["action_rows"] = torch.empty((k, N, G), dtype=torch.float64, device=dev)
                if rows:
                    buf["price_rows"] = torch.empty((k, G), dtype=torch.float64, device=dev)
                    buf["dist_rows"] = torch.empty((k, G), dtype=torch.float64, device=dev)
            a.row_begin, a.row_count = b0, k
            for f in host:
                setattr(a, f, buf[f].data_ptr() if f in buf else None)
            _lib.check(batch.L.thrl_sampled_deviation(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                       "thrl_sampled_deviation")
            if unsolved is not None:                     # what the kernel writes for a game it does not solve
                for t in buf.values():
                    t[..., unsolved] = 0.0
            if st is not None and k:
                group_stats.reduce(batch.L, buf["reward_rows"], buf["action_rows"], k, st, batch._stream(), at=b0)
            if rows and k:
                for f in host:
                    host[f].append(buf[f].cpu().numpy())
            b0 += k
            if b0 >= K or not want:
                break
        torch.cuda.synchronize(dev)
        if unsolved is not None:
            for f, t in out.items():
                t[..., unsolved] = -1 if f in INT else 0
        res = an.fetch(out)
        if rows:
            for f in host:
                res[f] = np.concatenate(host[f], axis=0)
        if st is not None:
            from .group_stats import to_numpy
            res["group_stats"] = to_numpy(st)
        del keep
        res["epsilon"] = np.repeat(np.asarray(eps, np.float64)[:, None], G, axis=1) if eps_g is None else eps_g.cpu().numpy()
        res["gamma"] = np.full(G, gam[d], np.float64) if gam_g is None else gam_g[d].cpu().numpy()
        if dev_policy is not None:
            res["dev_policy"] = dev_policy.cpu().numpy().view(np.uint16)
    res["solved"] = solved(res["epsilon"], kinds)
    if unsolved is not None:
        res["solved"][unsolved.cpu().numpy()] = False
    res["stat_iters"] = stat_iters
    res["deviator"], res["T"], res["n_prices"], res["lds_bytes"], res["ret_tol"] = d, T, D, ws["bytes"], float(ret_tol)
    return res


def solved(epsilon, kinds):
    """bool [G]: the games thrl_sampled_deviation solves, those whose QTable agents' epsilon lies in [0, 1]."""
    e = np.asarray(epsilon, np.float64)
    ok = np.ones(e.shape[1], bool)
    with np.errstate(invalid="ignore"):
        for i, k in enumerate(kinds):
            if k == "QTable":
                ok &= (e[i] >= 0.0) & (e[i] <= 1.0)
    return ok


# ---------------------------------------------------------------------------------------------- host side
def summarize(games, ids, n_groups, deviators):
    """The summary rows, one per (group, deviator), deviation.summarize_noise's columns: games[d] = the dict of per-game
    arrays of deviator d (run / load_games) in game order, ids = group id per game.  Every statistic but `games` is over
    the solved games: solved (their number), deviates (the share with dev_share > 0), dev_share_mean, unprofitable (the
    share with gain < 0), gain_mean, gain_q25 / q50 / q75, gain_dev_mean, low_mean, returned (the share with ret_step >=
    0), ret_step_mean over those, dist_mean."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    out = []
    for k in range(int(n_groups)):
        for d in deviators:
            g = games[d]
            m = (ids == k) & np.asarray(g["solved"], bool)
            f = {name: np.asarray(g[name], np.float64)[m] for name in FLOAT}
            ret = np.asarray(g["ret_step"])[m]
            row = {"group": k, "deviator": int(d), "games": int(np.sum(ids == k)), "solved": int(m.sum()),
                   "deviates": an.frac(f["dev_share"] > 0), "dev_share_mean": an.mean(f["dev_share"]),
                   "unprofitable": an.frac(f["gain"] < 0), "gain_mean": an.mean(f["gain"])}
            an.quantiles(row, "gain", f["gain"])
            row.update(gain_dev_mean=an.mean(f["gain_dev"]), low_mean=an.mean(f["low"]), returned=an.frac(ret >= 0),
                       ret_step_mean=an.mean(ret[ret >= 0]), dist_mean=an.mean(f["dist"]))
            out.append(row)
    return out


def describe(options, T, n_prices, summary):
    """sampled_deviation.json's content."""
    return {"options": options, "T": int(T), "n_prices": int(n_prices), "quantiles": list(an.QUANTILES), "summary": summary}


# ---------------------------------------------------------------------------------------------- artefacts
def save_games(d, deviator, r):
    """sdev<d>_games float64 [7, G] (base_price, dev_share, gain, gain_dev, low, dist, mass), sdev<d>_steps int32 [2, G]
    (low_step, ret_step), sdev<d>_base float64 [2, N, G] (base_reward, base_action), sdev<d>_gamma float64 [G]; sdev_epsilon
    float64 [N, G], sdev_solved bool [G] and sdev_stat_iters int32 [G] (the stationary iteration behind the weights) are
    the same for every deviator."""
    np.save(os.path.join(d, "sdev%d_games.npy" % deviator), np.stack([r[f] for f in FLOAT]).astype(np.float64))
    np.save(os.path.join(d, "sdev%d_steps.npy" % deviator), np.stack([r[f] for f in INT]).astype(np.int32))
    np.save(os.path.join(d, "sdev%d_base.npy" % deviator), np.stack([r[f] for f in AGENT]).astype(np.float64))
    np.save(os.path.join(d, "sdev%d_gamma.npy" % deviator), np.asarray(r["gamma"], np.float64))
    np.save(os.path.join(d, "sdev_epsilon.npy"), np.asarray(r["epsilon"], np.float64))
    np.save(os.path.join(d, "sdev_solved.npy"), np.asarray(r["solved"], bool))
    np.save(os.path.join(d, "sdev_stat_iters.npy"), np.asarray(r["stat_iters"], np.int32))


def load_games(d, deviator):
    """The per-game arrays one run directory holds for `deviator` (training.sampled_play.deviation)."""
    gm = np.load(os.path.join(d, "sdev%d_games.npy" % deviator))
    st = np.load(os.path.join(d, "sdev%d_steps.npy" % deviator))
    base = np.load(os.path.join(d, "sdev%d_base.npy" % deviator))
    g = {f: gm[k] for k, f in enumerate(FLOAT)}
    g.update({f: st[k] for k, f in enumerate(INT)})
    g.update({f: base[k] for k, f in enumerate(AGENT)})
    g["gamma"] = np.load(os.path.join(d, "sdev%d_gamma.npy" % deviator))
    for f in ("epsilon", "solved", "stat_iters"):
        g[f] = np.load(os.path.join(d, "sdev_%s.npy" % f))
    return g


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, epsilon="current", tabs=None, pi=None, stat_iters=None,
                    spec=None, histograms=False, budget=None):
    """train_one's training.sampled_play.deviation outputs: the per-game sdev_*.npy and sdev<d>_*.npy files, with a spec
    the response curves' group statistics under the prefix sdev<d>, and sampled_deviation.json.  epsilon: sampled_play's
    option; pi, stat_iters: its distributions where it stored them, with its step counts (else computed here, once)."""
    from . import trainer
    from . import tuple_stationary as ts
    tabs = sp.tables(config) if tabs is None else tabs
    probs = sp.price_probs(batch, tabs["dprice"])
    dpolicy = ts.price_policy(batch, tabs["dprice"])
    if pi is None:
        st = sp.run(batch, epsilon=epsilon, pi=True, probs=probs, dpolicy=dpolicy, tabs=tabs)
        pi, stat_iters = st["pi"], st["iters"]
    games = {}
    for d in opt["agents"]:
        r = run(batch, deviator=d, steps=opt["steps"], dev_len=opt["dev_len"], action=opt["action"], epsilon=epsilon,
                ret_tol=opt["ret_tol"], weights=pi, group_stats=spec, budget=budget, probs=probs, dpolicy=dpolicy, tabs=tabs)
        if stat_iters is not None:
            r["stat_iters"] = np.asarray(stat_iters, np.int32)
        games[d] = r
        save_games(exp_path, d, r)
        if spec is not None:
            trainer.save_group_stats(exp_path, "sdev%d" % d, r["group_stats"], spec, histograms)
    an.save_json(os.path.join(exp_path, "sampled_deviation.json"),
                 describe(opt, r["T"], r["n_prices"], summarize(games, ids, n_groups, opt["agents"])))
    return games
