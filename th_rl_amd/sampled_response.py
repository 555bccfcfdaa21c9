"""Sampled play: exact best responses to the rivals' STOCHASTIC policies (thrl_sampled_response,
include/thrl_response.h) -- the exploitability of the policies the agents were trained with.

sampled_play says what the stochastic policies earn in the long run; this module says whether each of them is a good
reply to the others.  An agent conditions on the price alone, so agent i's problem against a sampling softmax and an
epsilon-greedy table lives on the D distinct prices of the config: V_pi, the value of its own mixed policy, and V*,
sigma*, its best deterministic reply, by Jacobi sweeps and policy iteration (definitions in the header).  run() returns
per selected agent and game iters (-1: not solved or capped), sweeps, n_diff, loss_all, loss_mean and, weighted by the
long-run distribution pi of sampled play, loss_w, gain_w (what the best reply adds to the discounted value), v_w and
br_prob_w (the long-run share of steps on which the agent already plays its best response).  (1 - gamma_i) gain_w is the
agent's exploitability in reward units per period; its sum over the agents is the profile's NashConv.  It separates
"prices above Nash because the profile is an epsilon-equilibrium" from "prices above Nash because nobody has learned to
undercut a randomising rival".

run() is noise-free play.  run_noise() is the same question in the environment the reference ships (NoisyPriceState,
thrl_sampled_response_noise, include/thrl_response_noise.h): the agent's states are the D distinct prices and then the Jn
quadrature nodes of the redrawn price (sampled_play.noise_tables), n_diff and loss_mean come per kind of state, and the
weights are the long-run distribution of the state in which a decision is made.

In train_one the analysis is the sub-key "response" of training.sampled_play, as "noise" is: true, or {"agents",
"eval_tol", "max_sweeps", "policies"}.  It writes sampled_response.json and sresp_*.npy; utils.sampled_response_summary
and utils.sampled_response_games read them.  With "noise": true in that dict (and sampled_play's own "noise", whose
noise_prob and resolution it takes) the analysis is run_noise's and writes sampled_response_noise.json and srespn_*.npy
(utils.sampled_response_noise_summary / sampled_response_noise_games).  Sharded runs (th_rl_amd.launch) are out of scope,
as sampled_play is.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from . import equilibrium as eq
from . import sampled_play as sp
from . import tuple_play as tp
from ._lib import ThrlError
from .deviation import optimal

DEFAULTS = dict(agents=None, eval_tol=1e-12, max_sweeps=8192, policies=False)
NOISE_FOLLOW_UP = ("best responses to sampled play under demand noise are the follow-up of the noise-free ones and opted into: "
                   "set \"noise\": true inside \"response\", or drop \"noise\" or \"response\"")
MAX_LDS = _lib.SR_MAX_LDS
MAX_TEAM_BYTES = 32 * 1024
INT = ("iters", "sweeps", "n_diff")
FLOAT = ("loss_all", "loss_mean")
WEIGHTED = ("loss_w", "gain_w", "v_w", "br_prob_w")
PER_GAME = INT + FLOAT + WEIGHTED + ("gamma", "epsilon", "br_policy", "v_opt", "v_pi")
NOISE_INT = ("iters", "sweeps", "n_diff_prices", "n_diff_nodes")
NOISE_FLOAT = ("loss_all", "loss_prices_mean", "loss_nodes_mean")


def parse_options(opt, config, noise=None):
    """training.sampled_play.response (true or a dict) -> the dict with every key filled in: agents (None = all, or a
    list), eval_tol (>= 0), max_sweeps (an integer in [1, STAT_MAX_ITERS]), policies (store sigma*, V* and V_pi).  Refuses
    a working set above a CU's LDS.  The optional key "noise" (true or false) opts into the analysis under demand noise
    and stays in the result only when given; true needs `noise`, the parsed "noise" of training.sampled_play (its
    noise_prob and resolution are the analysis'), and the working set checked is then working_set_noise's."""
    name = "training.sampled_play.response"
    under_noise = None
    if isinstance(opt, dict) and "noise" in opt:
        opt = dict(opt)
        under_noise = opt.pop("noise")
        if not isinstance(under_noise, bool):
            raise ValueError("%s.noise must be true or false, got %r" % (name, under_noise))
    out = an.options("sampled_play.response", opt, DEFAULTS)
    n = len(config["agents"])
    if out["agents"] is not None:
        ag = out["agents"]
        if not isinstance(ag, (list, tuple)) or not ag or any(isinstance(d, bool) or not isinstance(d, int) or not 0 <= d < n
                                                              for d in ag):
            raise ValueError("%s.agents must be a non-empty list of agents in [0, %d), got %r" % (name, n, ag))
        out["agents"] = sorted(set(ag))
    if isinstance(out["eval_tol"], bool) or not isinstance(out["eval_tol"], (int, float)) or not out["eval_tol"] >= 0.0:
        raise ValueError("%s.eval_tol must be a number >= 0, got %r" % (name, out["eval_tol"]))
    out["eval_tol"] = float(out["eval_tol"])
    if isinstance(out["max_sweeps"], bool) or not isinstance(out["max_sweeps"], int) \
            or not 1 <= out["max_sweeps"] <= _lib.STAT_MAX_ITERS:
        raise ValueError("%s.max_sweeps must be an integer in [1, %d], got %r" % (name, _lib.STAT_MAX_ITERS, out["max_sweeps"]))
    if not isinstance(out["policies"], bool):
        raise ValueError("%s.policies must be true or false, got %r" % (name, out["policies"]))
    if under_noise and noise is None:
        raise ValueError("%s.noise: training.sampled_play has no \"noise\", whose noise_prob and resolution this mode takes" % name)
    if under_noise:
        ws = working_set_noise(config, noise["resolution"])
        if not ws["fits"]:
            raise ValueError("%s.noise: under noise a game's working set is %d bytes (T=%d, D=%d, Jn=%d), a CU's LDS holds %d"
                             % (name, ws["bytes"], ws["T"], ws["D"], ws["Jn"], MAX_LDS))
    else:
        ws = working_set(config)
        if not ws["fits"]:
            raise ValueError("%s: a game's working set is %d bytes (T=%d, D=%d), a CU's LDS holds %d"
                             % (name, ws["bytes"], ws["T"], ws["D"], MAX_LDS))
    if under_noise is not None:
        out["noise"] = under_noise
    return out


def team_of(D, max_actions):
    """The threads that share one price's actions (sr_layout): the largest power of two with team * D <= 256 and team <=
    the largest action count, 1 where the staging of 8 D max_i A_i bytes would pass 32 KB."""
    team = 1
    while team * 2 * D <= 256 and team * 2 <= max_actions:
        team *= 2
    return 1 if 8 * D * max_actions > MAX_TEAM_BYTES else team


def _working_head(tabs, n_nodes=0):
    """(bytes, T, D) of what sr_layout and srn_layout share (sr_layout_head) over S = D + n_nodes states: the sum of
    r16(x) over five arrays of 8 S, two of 8 T, the staged rows (4 D A_i per network, 2 D per QTable agent), 2 (D + 1),
    2 T, 2 T, 2 S and 2 S."""
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    S = D + n_nodes
    r16 = sp._r16
    b = 5 * r16(8 * S) + 2 * r16(8 * T)
    for kind, A in zip(tabs["kinds"], tabs["n_actions"]):
        b += r16(2 * D) if kind == "QTable" else r16(4 * D * int(A))
    return b + r16(2 * (D + 1)) + 2 * r16(2 * T) + 2 * r16(2 * S), T, D


def working_set(config, tabs=None):
    """The LDS bytes one game takes in thrl_sampled_response, by include/thrl_response.h's formula (sr_layout): the sum of
    r16(x) over five arrays of 8 D, two of 8 T, 4 D A_i per network, 2 D per QTable agent, 2 (D + 1), 2 T, 2 T, 2 D, 2 D,
    2,048, the team's staging 8 D max_i A_i (where a team shares a price) and 256.  Returns dict(bytes, T, D, team, fits)."""
    tabs = sp.tables(config) if tabs is None else tabs
    b, T, D = _working_head(tabs)
    max_actions = max(int(a) for a in tabs["n_actions"])
    team = team_of(D, max_actions)
    b += 2048 + (sp._r16(8 * D * max_actions) if team > 1 else 0) + 256
    return dict(bytes=int(b), T=T, D=D, team=team, fits=b <= MAX_LDS)


def working_set_noise(config, resolution=sp.NOISE_DEFAULTS["resolution"], tabs=None, n_nodes=None):
    """The LDS bytes one game takes in thrl_sampled_response_noise, by include/thrl_response_noise.h's formula
    (srn_layout), S = D + Jn: the sum of r16(x) over five arrays of 8 S, two of 8 T, 4 D A_i per network, 2 D per QTable
    agent, 2 (D + 1), 2 T, 2 T, 2 S, 2 S, 2 Jn per QTable agent, 2,048 and 256.  The networks' node rows are not part of
    it.  Jn from resolution (sampled_play.n_nodes_of) unless n_nodes is given.  Returns dict(bytes, T, D, Jn, fits)."""
    tabs = sp.tables(config) if tabs is None else tabs
    Jn = int(n_nodes) if n_nodes is not None else sp.n_nodes_of(config, resolution)
    b, T, D = _working_head(tabs, Jn)
    b += sum(sp._r16(2 * Jn) for kind in tabs["kinds"] if kind == "QTable") + 2048 + 256
    return dict(bytes=int(b), T=T, D=D, Jn=Jn, fits=b <= MAX_LDS)


def resolve_gamma(batch, gamma, G):
    """(gamma [N] floats, device float64 [N, G] or None) for `gamma`: None = each agent's own (a network's, else the
    config's) and the per-game sweep array where a sweep has one; a number = every agent's; N numbers; or an array [N, G]
    (device data: an entry outside [0, 1) leaves that (agent, game) unsolved)."""
    import torch
    N = batch.N
    if gamma is None:
        nn = getattr(batch, "nn", None) or {}
        own = [float(nn[i].gamma) if i in nn else float(batch.cfg.gamma[i]) for i in range(N)]
        sw = getattr(batch, "sweep", None) or {}
        if "gamma" in sw:
            return own, sw["gamma"][:, :G].to(torch.float64).contiguous()
        return own, None
    if isinstance(gamma, torch.Tensor) or np.ndim(gamma) == 2:
        x = gamma if isinstance(gamma, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(gamma, np.float64))
        x = x.to(device=batch.device, dtype=torch.float64)
        if x.dim() != 2 or x.shape[0] != N or x.shape[1] < G:
            raise ThrlError("sampled_response: a per-game gamma must be [N=%d, G>=%d], got %s" % (N, G, tuple(x.shape)))
        return [0.0] * N, x[:, :G].contiguous()
    x = [float(gamma)] * N if np.ndim(gamma) == 0 else [float(v) for v in gamma]
    if len(x) != N:
        raise ThrlError("sampled_response: gamma holds %d numbers, the game has %d agents" % (len(x), N))
    return x, None


def _run(batch, noise, agents, epsilon, gamma, eval_tol, max_sweeps, policies, pi, n_games, probs, dpolicy, tabs,
         noise_prob=None, resolution=None, nprobs=None, npolicy=None):
    """run()'s body (noise false) and run_noise()'s (true): under noise the call also takes the nodes and the band, the
    noise probability, the strategies at the nodes and three more tables, the arrays over the states are [D + Jn], and the
    counts and mean losses come per kind of state."""
    import torch
    from . import tuple_stationary as ts
    N = batch.N
    G = sp._games(batch, n_games)
    ag, mask = eq.agents_mask(agents, N)
    if isinstance(max_sweeps, bool) or not 1 <= int(max_sweeps) <= _lib.STAT_MAX_ITERS:
        raise ThrlError("sampled_response: max_sweeps=%r out of [1, %d]" % (max_sweeps, _lib.STAT_MAX_ITERS))
    if noise and (tabs is None or "xn" not in tabs):
        tabs = sp.noise_tables(batch.config, resolution, tabs=tabs)
    if tabs is None:
        tabs = sp.tables(batch.config)
    tp._batch_tables(batch, tabs)
    T, D = int(tabs["n_tuples"]), int(tabs["n_prices"])
    Jn, W = (int(tabs["n_nodes"]), int(tabs["band_w"])) if noise else (0, 0)
    S = D + Jn
    call = "thrl_sampled_response_noise" if noise else "thrl_sampled_response"
    ws = working_set_noise(batch.config, tabs=tabs, n_nodes=Jn) if noise else working_set(batch.config, tabs)
    if not ws["fits"]:                                   # what the call answers from the shape alone (the library's own
        # message is the shared "(N=.., n_cells=..)" with n_cells = the states; this one names the parts)
        err = ThrlError("%s refused (thrl_err %d): %d bytes of LDS per game (T=%d, n_prices=%d%s), at most %d"
                        % (call, _lib.ERR_UNSUPPORTED, ws["bytes"], T, D, ", n_nodes=%d" % Jn if noise else "", MAX_LDS))
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    kinds = tp._kinds(batch)
    dev = batch.device
    a = _lib.SampledResponseNoiseArgs() if noise else _lib.SampledResponseArgs()
    a.n_games, a.n_tuples, a.n_prices, a.agents = G, T, D, mask
    a.max_sweeps, a.eval_tol = int(max_sweeps), float(eval_tol)
    tab_list = [("grp_first", (D + 1,), np.int32), ("grp_perm", (T,), np.int32), ("reward", (N, T), np.float64)]
    if noise:
        a.n_nodes, a.band_w = Jn, W
        tab_list += [("band_lo", (T,), np.int32), ("band", (T, W), np.float64), ("noise_reward", (N, T), np.float64)]
    for i, k in enumerate(kinds):
        a.kind[i] = tp.KINDS[k]
    with torch.cuda.device(dev):
        eps, eps_g = sp.resolve_epsilon(batch, epsilon, G)
        gam, gam_g = resolve_gamma(batch, gamma, G)
        for i in range(N):
            a.eps[i], a.gamma[i] = eps[i], gam[i]
        if eps_g is not None:
            a.eps_g = eps_g.data_ptr()
        if gam_g is not None:
            a.sweep_gamma = gam_g.data_ptr()
        if noise:
            p_noise, p_g = an.resolve_noise(batch, noise_prob, G, "sampled_response")
            if p_g is not None:
                a.noise_prob_g = p_g.data_ptr()
            else:
                a.noise_prob = p_noise
        if probs is None:
            probs = sp.price_probs(batch, tabs["dprice"], n_games=G)
        if dpolicy is None:
            dpolicy = ts.price_policy(batch, tabs["dprice"], n_games=G)
        if noise and nprobs is None:
            nprobs = sp.price_probs(batch, tabs["xn"], n_games=G)
        if noise and npolicy is None:
            npolicy = ts.price_policy(batch, tabs["xn"], n_games=G)
        an.check_policy(batch, dpolicy, (G, N, D), "sampled_response", "dpolicy")
        rows = [("probs", probs, D, a.prob)]
        chain = {}                                       # what sampled_play.run takes on top, for pi
        if noise:
            an.check_policy(batch, npolicy, (G, N, Jn), "sampled_response", "npolicy")
            rows.append(("nprobs", nprobs, Jn, a.nprob))
            a.npolicy = npolicy.data_ptr()
            chain = dict(noise_prob=p_noise if p_g is None else p_g, nprobs=nprobs, npolicy=npolicy)
        sp.bind_rows(batch, kinds, G, "sampled_response", *rows)
        a.dpolicy = dpolicy.data_ptr()
        pi_t = None
        if pi is None:
            e = epsilon if eps_g is None else eps_g
            st = sp.run(batch, epsilon=e, pi=True, n_games=G, probs=probs, dpolicy=dpolicy, tabs=tabs, **chain)
            pi_t = torch.from_numpy(np.ascontiguousarray(st["pi"])).to(dev)
        elif pi is not False:
            if isinstance(pi, torch.Tensor):
                pi_t = pi.to(device=dev, dtype=torch.float64).contiguous()
            else:
                pi_t = torch.from_numpy(np.ascontiguousarray(np.asarray(pi, np.float64))).to(dev)
            if tuple(pi_t.shape) != (G, T):
                raise ThrlError("sampled_response: pi must be shaped %s, got %s" % ((G, T), tuple(pi_t.shape)))
        if pi_t is not None:
            a.pi = pi_t.data_ptr()
        keep = an.bind_tables(a, tabs, tab_list, dev, "sampled_response")
        out = an.outputs(dev, (NOISE_INT if noise else INT, (N, G), "int32"), (NOISE_FLOAT if noise else FLOAT, (N, G), "float64"),
                         (WEIGHTED if pi_t is not None else (), (N, G), "float64"),
                         (("br_policy",) if policies else (), (N, G, S), "int16"),
                         (("v_opt", "v_pi") if policies else (), (N, G, S), "float64"))
        an.bind(a, out)
        _lib.check(getattr(batch.L, call)(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()), call)
        torch.cuda.synchronize(dev)
        res = an.fetch(out)
        del keep
        res["epsilon"] = np.repeat(np.asarray(eps, np.float64)[:, None], G, axis=1) if eps_g is None else eps_g.cpu().numpy()
        res["gamma"] = np.repeat(np.asarray(gam, np.float64)[:, None], G, axis=1) if gam_g is None else gam_g.cpu().numpy()
        if noise:
            res["noise_prob"] = np.full(G, p_noise, np.float64) if p_g is None else p_g.cpu().numpy()
        if pi_t is not None:
            res["pi"] = pi_t.cpu().numpy()
    if policies:
        res["br_policy"] = res["br_policy"].view(np.uint16)
    res["agents"], res["T"], res["n_prices"], res["lds_bytes"] = ag, T, D, ws["bytes"]
    if noise:
        res["n_nodes"], res["resolution"] = Jn, int(tabs.get("resolution", resolution))
    res["eval_tol"], res["max_sweeps"] = float(eval_tol), int(max_sweeps)
    return res


def run(batch, agents=None, epsilon="current", gamma=None, eval_tol=1e-12, max_sweeps=8192, policies=False, pi=None,
        n_games=None, probs=None, dpolicy=None, tabs=None):
    """thrl_sampled_response for the first n_games (default all) games of `batch` (a MixedGameBatch of QTable / Reinforce
    / ActorCritic agents, or a GameBatch).  agents: the agents solved (default all).  epsilon: sampled_play's rules.
    gamma: resolve_gamma's.  pi: the long-run distribution that weights loss_w, gain_w, v_w and br_prob_w: None = computed
    here with sampled_play.run(pi=True) on the same strategies, an array [G, T], or False = no weighted outputs.  probs,
    dpolicy, tabs as in sampled_play.run.  policies=True adds br_policy (uint16), v_opt, v_pi [N, G, D].  Returns a dict
    of numpy arrays, [N, G] with zeros for the agents that are not selected."""
    return _run(batch, False, agents, epsilon, gamma, eval_tol, max_sweeps, policies, pi, n_games, probs, dpolicy, tabs)


def run_noise(batch, agents=None, epsilon="current", gamma=None, eval_tol=1e-12, max_sweeps=8192, policies=False, pi=None,
              n_games=None, probs=None, dpolicy=None, tabs=None, noise_prob=None, resolution=sp.NOISE_DEFAULTS["resolution"],
              nprobs=None, npolicy=None, ntabs=None):
    """thrl_sampled_response_noise for the first n_games (default all) games of `batch`: run()'s question under demand
    noise, on the D distinct prices and then the Jn nodes of the redrawn price.  agents, epsilon, gamma, eval_tol,
    max_sweeps, policies, probs, dpolicy as in run().  noise_prob: a number in (0, 1], an array [G] (device data: an entry
    outside (0, 1] refuses that game) or None = the batch's own (sampled_play.resolve_noise).  resolution: the uniform
    cuts behind the nodes; ntabs (or tabs): sampled_play.noise_tables(batch.config, resolution); nprobs / npolicy: the
    strategies at ntabs["xn"] as in sampled_play.run.  pi: None = computed here with sampled_play.run(noise_prob=...,
    pi=True) on the same strategies, an array [G, T], or False = no weighted outputs.  policies=True adds br_policy
    (uint16), v_opt, v_pi [N, G, D + Jn], the prices first.  Returns a dict of numpy arrays, [N, G] with zeros for the
    agents that are not selected: iters, sweeps, n_diff_prices, n_diff_nodes, loss_all, loss_prices_mean,
    loss_nodes_mean, loss_w, gain_w, v_w, br_prob_w, gamma, epsilon, and noise_prob [G]."""
    return _run(batch, True, agents, epsilon, gamma, eval_tol, max_sweeps, policies, pi, n_games, probs, dpolicy,
                ntabs if ntabs is not None else tabs, noise_prob, resolution, nprobs, npolicy)


# ---------------------------------------------------------------------------------------------- host side
def exploitability(games):
    """(1 - gamma_i) * gain_w [N, G]: what agent i's best reply adds, in reward units per period."""
    return (1.0 - np.asarray(games["gamma"], np.float64)) * np.asarray(games["gain_w"], np.float64)


def summarize(games, agents, ids, n_groups, nash, cartel):
    """The summary rows.  One per (group, agent) with "agent": games, capped (the share of games not solved), br_all (the
    share of the solved games whose own policy loses nothing anywhere: loss_all <= 0), loss_all_q25 / q50 / q75,
    loss_w_mean, br_prob_w_mean and exploit_mean, the mean of (1 - gamma_i) * gain_w, over the solved games.  One per
    group with "agent": None: games, solved (the games solved for every selected agent), nashconv_mean (nashconv = the sum
    of the agents' exploitabilities) and nashconv_small, the share of those games with nashconv < 1 % of Cartel - Nash."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    iters = np.asarray(games["iters"], np.int64)
    loss_all = np.asarray(games["loss_all"], np.float64)
    has_w = "gain_w" in games
    ex = exploitability(games) if has_w else None
    out = []
    for k in range(int(n_groups)):
        m = ids == k
        every = m.copy()
        for i in agents:
            ms = m & (iters[i] >= 0)
            every &= iters[i] >= 0
            row = {"group": k, "agent": int(i), "games": int(m.sum()), "capped": an.frac(iters[i][m] < 0) if m.any() else None,
                   "br_all": an.frac(loss_all[i][ms] <= 0.0) if ms.any() else None}
            an.quantiles(row, "loss_all", loss_all[i][ms])
            if has_w:
                row["loss_w_mean"] = an.mean(np.asarray(games["loss_w"], np.float64)[i][ms])
                row["br_prob_w_mean"] = an.mean(np.asarray(games["br_prob_w"], np.float64)[i][ms])
                row["exploit_mean"] = an.mean(ex[i][ms])
            out.append(row)
        row = {"group": k, "agent": None, "games": int(m.sum()), "solved": int(every.sum())}
        if has_w:
            nc = np.zeros(ids.size)
            for i in agents:
                nc = nc + np.where(every, ex[i], 0.0)
            row["nashconv_mean"] = an.mean(nc[every])
            row["nashconv_small"] = an.frac(nc[every] < 0.01 * (float(cartel) - float(nash))) if every.any() else None
        out.append(row)
    return out


def summarize_noise(games, agents, ids, n_groups, nash, cartel, max_jump=None):
    """summarize()'s rows for run_noise()'s arrays.  A (group, agent) row also has diff_nodes_mean, the mean number of
    node-states where the best reply is not the modal action, over the solved games; a group's own row also has
    max_jump_max, the chain's honesty figure of the midpoint rule (sampled_play.summarize), over the group's games, where
    max_jump [G] is given."""
    rows = summarize(games, agents, ids, n_groups, nash, cartel)
    ids = np.asarray(ids, np.int64).reshape(-1)
    iters = np.asarray(games["iters"], np.int64)
    nodes = np.asarray(games["n_diff_nodes"], np.float64)
    for row in rows:
        m = ids == row["group"]
        if row["agent"] is not None:
            i = row["agent"]
            row["diff_nodes_mean"] = an.mean(nodes[i][m & (iters[i] >= 0)])
        elif max_jump is not None:
            row["max_jump_max"] = an.num(np.asarray(max_jump, np.float64)[m].max()) if m.any() else None
    return rows


# ---------------------------------------------------------------------------------------------- artefacts
class FileSet:
    """The files one analysis writes into a run directory.  json: the summary's name.  files: (name, fields, dtype), the
    fields stacked: <prefix>_counts int32 [len(ints), N, G], <prefix>_loss float64 [len(floats), N, G], <prefix>_weighted
    float64 [4, N, G] (loss_w, gain_w, v_w, br_prob_w).  plain: (field, name), float64 as run() returns it:
    <prefix>_gamma and <prefix>_epsilon [N, G], under noise <prefix>_noise_prob [G].  optional: (field, name, dtype),
    written with the policies: <prefix>_br_policy uint16, <prefix>_v_opt and <prefix>_v_pi float64 [N, G, states]."""

    def __init__(self, prefix, json, ints, floats, plain):
        self.json = json
        self.files = (("%s_counts.npy" % prefix, ints, np.int32), ("%s_loss.npy" % prefix, floats, np.float64),
                      ("%s_weighted.npy" % prefix, WEIGHTED, np.float64))
        self.plain = tuple((f, "%s_%s.npy" % (prefix, f)) for f in plain)
        self.optional = tuple((f, "%s_%s.npy" % (prefix, f), dt)
                              for f, dt in (("br_policy", np.uint16), ("v_opt", np.float64), ("v_pi", np.float64)))


PLAY_FILES = FileSet("sresp", "sampled_response.json", INT, FLOAT, ("gamma", "epsilon"))
NOISE_FILES = FileSet("srespn", "sampled_response_noise.json", NOISE_INT, NOISE_FLOAT, ("gamma", "epsilon", "noise_prob"))


def _save(fs, d, r):
    for name, fields, dt in fs.files:
        np.save(os.path.join(d, name), np.stack([np.asarray(r[f], dt) for f in fields]))
    for f, name in fs.plain:
        np.save(os.path.join(d, name), np.asarray(r[f], np.float64))
    for f, name, dt in fs.optional:
        path = os.path.join(d, name)
        if f in r:
            np.save(path, np.asarray(r[f], dt))
        elif os.path.isfile(path):               # a file left by an earlier run with other options
            os.remove(path)


def _load(fs, d):
    g = {}
    for name, fields, _ in fs.files:
        x = np.load(os.path.join(d, name))
        g.update({f: x[k] for k, f in enumerate(fields)})
    for f, name in fs.plain:
        g[f] = np.load(os.path.join(d, name))
    for f, name, _ in fs.optional:
        if os.path.isfile(os.path.join(d, name)):
            g[f] = np.load(os.path.join(d, name))
    return g


def save_games(d, r):
    """sresp_counts int32 [3, N, G] (iters, sweeps, n_diff), sresp_loss float64 [2, N, G] (loss_all, loss_mean),
    sresp_weighted float64 [4, N, G] (loss_w, gain_w, v_w, br_prob_w), sresp_gamma and sresp_epsilon float64 [N, G]; with
    the policies sresp_br_policy uint16, sresp_v_opt and sresp_v_pi float64 [N, G, D]."""
    _save(PLAY_FILES, d, r)


def save_games_noise(d, r):
    """srespn_counts int32 [4, N, G] (iters, sweeps, n_diff_prices, n_diff_nodes), srespn_loss float64 [3, N, G] (loss_all,
    loss_prices_mean, loss_nodes_mean), srespn_weighted float64 [4, N, G] (loss_w, gain_w, v_w, br_prob_w), srespn_gamma
    and srespn_epsilon float64 [N, G], srespn_noise_prob float64 [G]; with the policies srespn_br_policy uint16,
    srespn_v_opt and srespn_v_pi float64 [N, G, D + Jn]."""
    _save(NOISE_FILES, d, r)


def load_games(d):
    """The per-game arrays one run directory holds (training.sampled_play.response)."""
    return _load(PLAY_FILES, d)


def load_games_noise(d):
    """The per-game arrays one run directory holds (training.sampled_play.response with "noise")."""
    return _load(NOISE_FILES, d)


def describe(options, r, nash, cartel, summary):
    """sampled_response.json's content."""
    return {"options": options, "agents": [int(i) for i in r["agents"]], "T": int(r["T"]), "n_prices": int(r["n_prices"]),
            "nash": nash, "cartel": cartel, "quantiles": list(an.QUANTILES),
            "benchmark": "noise-free Nash and Cartel rewards (environment.get_optimal)", "summary": summary}


def describe_noise(options, r, nash, cartel, summary):
    """sampled_response_noise.json's content."""
    d = describe(options, r, nash, cartel, summary)
    d.update(n_nodes=int(r["n_nodes"]), resolution=int(r["resolution"]))
    return d


def _write(fs, exp_path, config, opt, r, rows, content):
    """The artefacts of the result r: the file set's per-game arrays and its json, content(opt, r, nash, cartel, summary)
    with the summary rows(r, r["agents"], nash, cartel)."""
    _save(fs, exp_path, r)
    nash, cartel = optimal(config)
    an.save_json(os.path.join(exp_path, fs.json), content(opt, r, nash, cartel, rows(r, r["agents"], nash, cartel)))
    return r


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, epsilon="current", tabs=None, pi=None):
    """train_one's training.sampled_play.response outputs: the per-game sresp_*.npy files and sampled_response.json.
    epsilon: sampled_play's option; pi: its distributions where it stored them (else computed here)."""
    r = run(batch, agents=opt["agents"], epsilon=epsilon, eval_tol=opt["eval_tol"], max_sweeps=opt["max_sweeps"],
            policies=opt["policies"], pi=pi, tabs=tabs)
    return _write(PLAY_FILES, exp_path, config, opt, r, lambda g, ag, nash, cartel: summarize(g, ag, ids, n_groups, nash, cartel),
                  describe)


def write_artefacts_noise(exp_path, batch, config, opt, ids, n_groups, noise_prob, epsilon="current", tabs=None, pi=None,
                          max_jump=None):
    """train_one's training.sampled_play.response outputs under demand noise: the per-game srespn_*.npy files and
    sampled_response_noise.json.  noise_prob and tabs (sampled_play.noise_tables) are sampled_play's own; pi: its
    distributions where it stored them (else computed here); max_jump: its honesty figure, carried into the summary."""
    r = run_noise(batch, agents=opt["agents"], epsilon=epsilon, eval_tol=opt["eval_tol"], max_sweeps=opt["max_sweeps"],
                  policies=opt["policies"], pi=pi, ntabs=tabs, noise_prob=noise_prob)
    return _write(NOISE_FILES, exp_path, config, opt, r,
                  lambda g, ag, nash, cartel: summarize_noise(g, ag, ids, n_groups, nash, cartel, max_jump=max_jump), describe_noise)
