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
ret_step, dist, mass [G], optionally the rows of every period.

run_noise() is the same test UNDER DEMAND NOISE (thrl_sampled_deviation_noise, include/thrl_sampled_deviation_noise.h),
the environment the reference ships: the chain is sampled_play's under noise, the deviator's strategy lives on the D
distinct prices and then the Jn nodes of the redrawn price (sampled_response.run_noise's order, so its br_policy is the
patient best reply as it stands), and every period's reward and price are expectations over the redrawn demand.

In train_one the analysis is the sub-key "deviation" of training.sampled_play, beside "response": true, or {"agents",
"steps", "dev_len", "action", "ret_tol"}.  It writes sampled_deviation.json, sdev_*.npy and sdev<d>_*.npy per deviator
(with training.group_stats also the response curves' statistics under the same prefix); utils.sampled_deviation_summary
and utils.sampled_deviation_games read them.  Beside sampled_play's "noise" the key opts in with its own "noise": true
and then runs at sampled_play's noise_prob and resolution; it writes sampled_deviation_noise.json, sdevn_*.npy and
sdevn<d>_*.npy (utils.sampled_deviation_noise_summary / _games) and none of the noise-free files.  Sharded runs
(th_rl_amd.launch) are out of scope, as sampled_play is.
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
NOISE_FOLLOW_UP = ("the deviation test of sampled play under demand noise is the follow-up of the noise-free one and opted into: "
                   "set \"noise\": true inside \"deviation\", or drop \"noise\" or \"deviation\"")
MAX_LDS = _lib.SD_MAX_LDS
ACTIONS = ("best_response", "best_reply")
AGENT = ("base_reward", "base_action")
FLOAT = ("base_price", "dev_share", "gain", "gain_dev", "low", "dist", "mass")
INT = ("low_step", "ret_step")
PER_GAME = AGENT + FLOAT + INT + ("gamma", "epsilon", "stat_iters", "solved")


def parse_options(opt, config, noise=None):
    """training.sampled_play.deviation (true or a dict) -> the dict with every key filled in: agents (the deviators,
    default all), steps K, dev_len L (1 <= L <= K <= DEV_MAX_STEPS), action ("best_response", "best_reply" = the patient
    best reply of sampled_response, or an action index of every deviator), ret_tol (>= 0).  Refuses a working set above a
    CU's LDS.  The optional key "noise" (true or false) opts into the test under demand noise and stays in the result only
    when given; true needs `noise`, the parsed "noise" of training.sampled_play (its noise_prob and resolution are the
    test's), the working set checked is then working_set_noise's, and with action "best_reply" also
    sampled_response.working_set_noise's."""
    name = "training.sampled_play.deviation"
    under_noise = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        under_noise = opt.pop("noise")
        if not isinstance(under_noise, bool):
            raise ValueError("%s.noise must be true or false, got %r" % (name, under_noise))
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
    if under_noise and noise is None:
        raise ValueError("%s.noise: training.sampled_play has no \"noise\", whose noise_prob and resolution this mode takes" % name)
    if under_noise:
        from . import sampled_response as sr
        sets = [(name + ".noise", working_set_noise(config, noise["resolution"]))]
        if out["action"] == "best_reply":
            sets.append((name + ".noise: action \"best_reply\"", sr.working_set_noise(config, noise["resolution"])))
        for what, ws in sets:
            if not ws["fits"]:
                raise ValueError("%s: under noise a game's working set is %d bytes (T=%d, D=%d, Jn=%d), a CU's LDS holds %d"
                                 % (what, ws["bytes"], ws["T"], ws["D"], ws["Jn"], MAX_LDS))
    else:
        ws = working_set(config)
        if not ws["fits"]:
            raise ValueError("%s: a game's working set is %d bytes (T=%d, D=%d), a CU's LDS holds %d"
                             % (name, ws["bytes"], ws["T"], ws["D"], MAX_LDS))
    if under_noise is not None:
        out["noise"] = under_noise
    return out


def working_set(config, tabs=None):
    """The LDS bytes one game takes in thrl_sampled_deviation, by include/thrl_sampled_deviation.h's formula (sd_layout):
    sampled_play.working_set's sum + r16(2 D) + r16(8 D) + 512.  Returns dict(bytes, T, D, fits)."""
    tabs = sp.tables(config) if tabs is None else tabs
    ws = sp.working_set(config, tabs)
    D = int(ws["D"])
    b = int(ws["bytes"]) + sp._r16(2 * D) + sp._r16(8 * D) + 512
    return dict(bytes=int(b), T=int(ws["T"]), D=D, fits=b <= MAX_LDS)


def working_set_noise(config, resolution=sp.NOISE_DEFAULTS["resolution"], tabs=None, n_nodes=None):
    """The LDS bytes one game takes in thrl_sampled_deviation_noise, by include/thrl_sampled_deviation_noise.h's formula
    (sdn_layout): sampled_play.working_set's sum under noise + r16(2 (D + Jn)) + r16(8 D) + 512.  Jn from resolution
    (sampled_play.n_nodes_of) unless n_nodes is given.  Returns dict(bytes, T, D, Jn, fits)."""
    tabs = sp.tables(config) if tabs is None else tabs
    ws = sp.working_set(config, tabs, resolution=resolution, n_nodes=n_nodes)
    D, Jn = int(ws["D"]), int(ws["Jn"])
    b = int(ws["bytes"]) + sp._r16(2 * (D + Jn)) + sp._r16(8 * D) + 512
    return dict(bytes=int(b), T=int(ws["T"]), D=D, Jn=Jn, fits=b <= MAX_LDS)


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
    return _run(batch, False, deviator, steps, dev_len, action, epsilon, gamma, ret_tol, weights, rows, group_stats, budget,
                n_games, probs, dpolicy, tabs, tol, max_iters)


def run_noise(batch, deviator=0, steps=32, dev_len=1, action="best_response", epsilon="current", gamma=None, ret_tol=1e-6,
              weights="stationary", rows=False, group_stats=None, budget=None, n_games=None, probs=None, dpolicy=None, tabs=None,
              tol=1e-12, max_iters=8192, noise_prob=None, resolution=sp.NOISE_DEFAULTS["resolution"], nprobs=None, npolicy=None):
    """thrl_sampled_deviation_noise for the first n_games (default all) games of `batch`: run()'s test under demand noise.
    deviator .. max_iters as in run(), with these differences: a strategy given as action is a [G, D + Jn] array, the
    distinct prices first, then the nodes; "best_reply" takes sampled_response.run_noise's br_policy (and is refused where
    that call's own working set does not fit); weights "stationary" = the long-run distribution of sampled play under the
    same noise, sampled_play.run(noise_prob=..., pi=True).  noise_prob: a number in [0, 1], an array [G] (device data: an
    entry outside [0, 1] leaves that game unsolved) or None = the batch's own (sampled_play.resolve_noise).  resolution:
    the uniform cuts behind the nodes; tabs: sampled_play.noise_tables(batch.config, resolution); nprobs / npolicy: the
    strategies at tabs["xn"] as in sampled_play.run.  The result also holds noise_prob and max_jump [G] (sampled_play's
    honesty figure of the midpoint rule), n_nodes and resolution."""
    return _run(batch, True, deviator, steps, dev_len, action, epsilon, gamma, ret_tol, weights, rows, group_stats, budget,
                n_games, probs, dpolicy, tabs, tol, max_iters, noise_prob, resolution, nprobs, npolicy)


def _run(batch, noise, deviator, steps, dev_len, action, epsilon, gamma, ret_tol, weights, rows, group_stats, budget, n_games,
         probs, dpolicy, tabs, tol, max_iters, noise_prob=None, resolution=None, nprobs=None, npolicy=None):
    """run()'s body (noise false) and run_noise()'s (true): under noise the call also takes the nodes and the band, the
    noise probability, the strategies at the nodes and four more tables, and the deviator's strategy is over the D + Jn
    states."""
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
    if noise and (tabs is None or "xn" not in tabs):
        tabs = sp.noise_tables(batch.config, resolution, tabs=tabs)
    if tabs is None:
        tabs = sp.tables(batch.config)
    tp._batch_tables(batch, tabs)
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    Jn, W = (int(tabs["n_nodes"]), int(tabs["band_w"])) if noise else (0, 0)
    S = D + Jn                                           # the states the deviator's strategy lives on
    call = "thrl_sampled_deviation_noise" if noise else "thrl_sampled_deviation"
    ws = working_set_noise(batch.config, tabs=tabs, n_nodes=Jn) if noise else working_set(batch.config, tabs)
    if not ws["fits"]:                                   # what the call answers from the shape alone
        err = ThrlError("%s refused (thrl_err %d): %d bytes of LDS per game (T=%d, n_prices=%d%s), at most %d"
                        % (call, _lib.ERR_UNSUPPORTED, ws["bytes"], T, D, ", n_nodes=%d" % Jn if noise else "", MAX_LDS))
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    kinds = tp._kinds(batch)
    dev = batch.device
    a = _lib.SampledDeviationNoiseArgs() if noise else _lib.SampledDeviationArgs()
    a.n_games, a.n_tuples, a.n_prices = G, T, D
    tab_list = [("grp_first", (D + 1,), np.int32), ("grp_perm", (T,), np.int32), ("reward", (N, T), np.float64),
                ("scaled", (N, T), np.float64), ("price", (T,), np.float64)]
    if noise:
        a.n_nodes, a.band_w = Jn, W
        tab_list += [("band_lo", (T,), np.int32), ("band", (T, W), np.float64), ("noise_price", (T,), np.float64),
                     ("noise_reward", (N, T), np.float64)]
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
        sets = [("probs", probs, D, a.prob)]
        chain = {}                                       # what sampled_play.run and sampled_response.run_noise take on top
        if noise:
            p_noise, p_g = an.resolve_noise(batch, noise_prob, G, "sampled_deviation", zero_ok=True)
            if p_g is not None:
                a.noise_prob_g = p_g.data_ptr()
            else:
                a.noise_prob = p_noise
            if nprobs is None:
                nprobs = sp.price_probs(batch, tabs["xn"], n_games=G)
            if npolicy is None:
                npolicy = ts.price_policy(batch, tabs["xn"], n_games=G)
            an.check_policy(batch, npolicy, (G, N, Jn), "sampled_deviation", "npolicy")
            sets.append(("nprobs", nprobs, Jn, a.nprob))
            a.npolicy = npolicy.data_ptr()
            chain = dict(noise_prob=p_noise if p_g is None else p_g, nprobs=nprobs, npolicy=npolicy)
        sp.bind_rows(batch, kinds, G, "sampled_deviation", *sets)
        a.dpolicy = dpolicy.data_ptr()
        e = epsilon if eps_g is None else eps_g
        stat_iters = np.zeros(G, np.int32)
        if isinstance(weights, str):
            if weights != "stationary":
                raise ThrlError("sampled_deviation: weights must be 'stationary' or a [G, T] array, got %r" % (weights,))
            st = sp.run(batch, epsilon=e, tol=tol, max_iters=max_iters, pi=True, n_games=G, probs=probs, dpolicy=dpolicy, tabs=tabs,
                        **chain)
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
            if tuple(dev_policy.shape) != (G, S):
                raise ThrlError("sampled_deviation: a strategy given as action must be shaped %s, got %s"
                                % ((G, S), tuple(dev_policy.shape)))
        elif action == "best_reply":
            if noise:
                br = sr.run_noise(batch, agents=[d], epsilon=e, gamma=gamma, policies=True, pi=False, n_games=G, probs=probs,
                                  dpolicy=dpolicy, ntabs=tabs, **chain)
            else:
                br = sr.run(batch, agents=[d], epsilon=e, gamma=gamma, policies=True, pi=False, n_games=G, probs=probs,
                            dpolicy=dpolicy, tabs=tabs)
            dev_policy = torch.from_numpy(np.ascontiguousarray(br["br_policy"][d]).view(np.int16)).to(dev)
            if (br["iters"][d] < 0).any():               # not solved there: not solved here
                unsolved = torch.from_numpy(np.flatnonzero(br["iters"][d] < 0)).to(dev)
        if dev_policy is not None:
            a.flags = _lib.SD_POLICY                     # THRL_SDN_POLICY has the same value
            a.dev_policy = dev_policy.data_ptr()
        keep = an.bind_tables(a, tabs, tab_list, dev, "sampled_deviation")
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
            _lib.check(getattr(batch.L, call)(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()), call)
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
        if noise:
            res["noise_prob"] = np.full(G, p_noise, np.float64) if p_g is None else p_g.cpu().numpy()
            res["max_jump"] = max_jump(nprobs, G, dev).cpu().numpy()
    res["solved"] = solved(res["epsilon"], kinds, res.get("noise_prob"))
    if unsolved is not None:
        res["solved"][unsolved.cpu().numpy()] = False
    res["stat_iters"] = stat_iters
    res["deviator"], res["T"], res["n_prices"], res["lds_bytes"], res["ret_tol"] = d, T, D, ws["bytes"], float(ret_tol)
    if noise:
        res["n_nodes"], res["resolution"] = Jn, int(tabs.get("resolution", resolution))
    return res


def max_jump(nprobs, G, dev):
    """device float64 [G]: thrl_sampled_noise_chain's max_jump of the networks' node rows nprobs ({i: float32 [G, Jn, A_i]}),
    the largest |Pn_i(k|j + 1) - Pn_i(k|j)| over the networks, the nodes 1 <= j < Jn - 1 and the actions (the difference
    of the two float32 values in float64); 0 without a network."""
    import torch
    out = torch.zeros(G, dtype=torch.float64, device=dev)
    for x in nprobs.values():
        if x.shape[1] > 2:
            x = x.to(torch.float64)
            out = torch.maximum(out, (x[:, 2:, :] - x[:, 1:-1, :]).abs().amax(dim=(1, 2)))
    return out


def solved(epsilon, kinds, noise_prob=None):
    """bool [G]: the games thrl_sampled_deviation solves, those whose QTable agents' epsilon lies in [0, 1]; with noise_prob
    [G] those thrl_sampled_deviation_noise solves, whose noise probability lies in [0, 1] too."""
    e = np.asarray(epsilon, np.float64)
    ok = np.ones(e.shape[1], bool)
    with np.errstate(invalid="ignore"):
        if noise_prob is not None:
            p = np.asarray(noise_prob, np.float64)
            ok &= (p >= 0.0) & (p <= 1.0)
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


def summarize_noise(games, ids, n_groups, deviators):
    """summarize()'s rows for run_noise()'s arrays, each with max_jump_max, the chain's honesty figure of the midpoint rule
    (sampled_play.summarize) over the group's games, solved or not."""
    rows = summarize(games, ids, n_groups, deviators)
    ids = np.asarray(ids, np.int64).reshape(-1)
    for row in rows:
        m = ids == row["group"]
        row["max_jump_max"] = an.num(np.asarray(games[row["deviator"]]["max_jump"], np.float64)[m].max()) if m.any() else None
    return rows


def describe(options, T, n_prices, summary):
    """sampled_deviation.json's content."""
    return {"options": options, "T": int(T), "n_prices": int(n_prices), "quantiles": list(an.QUANTILES), "summary": summary}


def describe_noise(options, r, summary):
    """sampled_deviation_noise.json's content (r: a result of run_noise)."""
    d = describe(options, r["T"], r["n_prices"], summary)
    d.update(n_nodes=int(r["n_nodes"]), resolution=int(r["resolution"]))
    return d


# ---------------------------------------------------------------------------------------------- artefacts
NOISE_PREFIX = "sdevn"                                   # the files of the test under demand noise
NOISE_PER_GAME = PER_GAME + ("noise_prob", "max_jump")


def save_games(d, deviator, r, prefix="sdev"):
    """sdev<d>_games float64 [7, G] (base_price, dev_share, gain, gain_dev, low, dist, mass), sdev<d>_steps int32 [2, G]
    (low_step, ret_step), sdev<d>_base float64 [2, N, G] (base_reward, base_action), sdev<d>_gamma float64 [G]; sdev_epsilon
    float64 [N, G], sdev_solved bool [G] and sdev_stat_iters int32 [G] (the stationary iteration behind the weights) are
    the same for every deviator.  prefix NOISE_PREFIX: the same files of the test under demand noise, sdevn<d>_* and
    sdevn_*, and sdevn_noise_prob and sdevn_max_jump float64 [G]."""
    one = os.path.join(d, "%s%d_" % (prefix, deviator))
    np.save(one + "games.npy", np.stack([r[f] for f in FLOAT]).astype(np.float64))
    np.save(one + "steps.npy", np.stack([r[f] for f in INT]).astype(np.int32))
    np.save(one + "base.npy", np.stack([r[f] for f in AGENT]).astype(np.float64))
    np.save(one + "gamma.npy", np.asarray(r["gamma"], np.float64))
    np.save(os.path.join(d, prefix + "_epsilon.npy"), np.asarray(r["epsilon"], np.float64))
    np.save(os.path.join(d, prefix + "_solved.npy"), np.asarray(r["solved"], bool))
    np.save(os.path.join(d, prefix + "_stat_iters.npy"), np.asarray(r["stat_iters"], np.int32))
    if prefix == NOISE_PREFIX:
        np.save(os.path.join(d, prefix + "_noise_prob.npy"), np.asarray(r["noise_prob"], np.float64))
        np.save(os.path.join(d, prefix + "_max_jump.npy"), np.asarray(r["max_jump"], np.float64))


def load_games(d, deviator, prefix="sdev"):
    """The per-game arrays one run directory holds for `deviator` (training.sampled_play.deviation; prefix NOISE_PREFIX:
    with "noise")."""
    one = os.path.join(d, "%s%d_" % (prefix, deviator))
    gm, st, base = np.load(one + "games.npy"), np.load(one + "steps.npy"), np.load(one + "base.npy")
    g = {f: gm[k] for k, f in enumerate(FLOAT)}
    g.update({f: st[k] for k, f in enumerate(INT)})
    g.update({f: base[k] for k, f in enumerate(AGENT)})
    g["gamma"] = np.load(one + "gamma.npy")
    for f in ("epsilon", "solved", "stat_iters") + (("noise_prob", "max_jump") if prefix == NOISE_PREFIX else ()):
        g[f] = np.load(os.path.join(d, "%s_%s.npy" % (prefix, f)))
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


def write_artefacts_noise(exp_path, batch, config, opt, ids, n_groups, noise_prob, epsilon="current", tabs=None, pi=None,
                          stat_iters=None, spec=None, histograms=False, budget=None):
    """train_one's training.sampled_play.deviation outputs under demand noise: the per-game sdevn_*.npy and sdevn<d>_*.npy
    files, with a spec the response curves' group statistics under the prefix sdevn<d>, and sampled_deviation_noise.json.
    noise_prob and tabs (sampled_play.noise_tables) are sampled_play's own; epsilon: its option; pi, stat_iters: its
    distributions where it stored them, with its step counts (else computed here, once)."""
    from . import trainer
    from . import tuple_stationary as ts
    probs, nprobs = sp.price_probs(batch, tabs["dprice"]), sp.price_probs(batch, tabs["xn"])
    dpolicy, npolicy = ts.price_policy(batch, tabs["dprice"]), ts.price_policy(batch, tabs["xn"])
    rows = dict(probs=probs, dpolicy=dpolicy, tabs=tabs, noise_prob=noise_prob, nprobs=nprobs, npolicy=npolicy)
    if pi is None:
        st = sp.run(batch, epsilon=epsilon, pi=True, **rows)
        pi, stat_iters = st["pi"], st["iters"]
    games = {}
    for d in opt["agents"]:
        r = run_noise(batch, deviator=d, steps=opt["steps"], dev_len=opt["dev_len"], action=opt["action"], epsilon=epsilon,
                      ret_tol=opt["ret_tol"], weights=pi, group_stats=spec, budget=budget, **rows)
        if stat_iters is not None:
            r["stat_iters"] = np.asarray(stat_iters, np.int32)
        games[d] = r
        save_games(exp_path, d, r, NOISE_PREFIX)
        if spec is not None:
            trainer.save_group_stats(exp_path, "%s%d" % (NOISE_PREFIX, d), r["group_stats"], spec, histograms)
    an.save_json(os.path.join(exp_path, "sampled_deviation_noise.json"),
                 describe_noise(opt, r, summarize_noise(games, ids, n_groups, opt["agents"])))
    return games
