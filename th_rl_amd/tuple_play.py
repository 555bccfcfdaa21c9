"""Greedy play of trained games whose agents may be networks (thrl_tuple_policy, thrl_tuple_walk, include/thrl.h): the
limit cycle of greedy play, its profit gain and cross-play for any mix of QTable, Reinforce and ActorCritic agents.

The QTable analyses index a strategy by the agent's table row; a network has no rows.  The game has a finite state
set of its own: with discrete agents and no noise the price after a step is a function of that step's action tuple.
So a strategy of any discrete agent is a table over the game's T = prod_i A_i tuples (agent 0 slowest), and greedy play
between any agents of any games is a walk on tuple indices.

tables(config) gives the per-config arrays (price, reward, scaled per tuple) in float64, every operation rounded once
in the reference's order; the device reads them and does no scaling arithmetic of its own.  extract(batch) fills the
strategies [G, N, T] on the device (networks evaluated by the function thrl_nn_act evaluates), run() plays one round
or a list of rounds of seats [N, M] from start tuples and returns mu, lam, cycle_start, cycle_reward, cycle_action per
match (definitions in include/thrl.h), optionally the rows of the path.  start_tuples() maps states to tuples: a
noise-free trained game's state is the price of a tuple; a fresh reset or a noisy run's state is none (-1: that match
is refused with mu = -1 and counted under no_start).

summarize_self() gives per group: matches (mu >= 0), no_start, cycles, fixed_points, lam_hist and the profit gain's
delta_mean / q25 / q50 / q75 (deviation.profit_gain); re-seated rounds are summarised by crossplay.summarize
(delta_self_mean, retained, seat_gain) with no_start added.  Sharded runs (th_rl_amd.launch) are refused.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .deviation import LAM_BINS, QUANTILES, ROW_BUDGET, default_horizon, lam_bin_names, optimal, profit_gain

DEFAULTS = dict(rounds=0, scheme="rotate", against="own", seed=0, steps=0, horizon=None)
KINDS = {"QTable": 0, "Reinforce": 1, "ActorCritic": 2, "CAC": 3}
MAX_TUPLES = _lib.TP_MAX_TUPLES
OUT = ("mu", "lam", "cycle_start", "cycle_reward", "cycle_action")


def _agent_params(config):
    """Per agent: (kind, actions, lo, hi) with the defaults of the agent's class."""
    from .mixed import NN_DEFAULTS
    out = []
    for a in config["agents"]:
        kind = a.get("name", "QTable")
        if kind not in KINDS:
            raise ValueError("tuple_play: agent %r is not supported (QTable, Reinforce, ActorCritic)" % kind)
        if kind == "CAC":
            raise ValueError("tuple_play: a CAC agent's action is continuous, the game has no action tuples")
        p = dict(_lib.QTABLE_DEFAULTS if kind == "QTable" else NN_DEFAULTS, **a)
        out.append((kind, int(p["actions"]), float(p["action_range"][0]), float(p["action_range"][1])))
    return out


def check_config(config):
    """ValueError for a config the tuple form does not cover: a CAC agent, or more than MAX_TUPLES tuples."""
    ps = _agent_params(config)
    T = 1
    for _, A, _, _ in ps:
        T *= A
        if T > MAX_TUPLES:
            raise ValueError("tuple_play: more than %d action tuples (actions %s)" % (MAX_TUPLES, [p[1] for p in ps]))
    return ps, T


def tables(config):
    """The per-config tuple tables: dict with T, n_actions [N], kinds, price [T], reward [N, T], scaled [N, T] (float64).
    Tuples are ordered with agent 0 slowest.  scaled_i(t) = k / (A - 1) * (hi - lo) + lo for a QTable agent and
    k / A * (hi - lo) + lo for a Reinforce / ActorCritic agent (the reference's two `scale`s); price and reward are
    env_step with intercept a and no noise: every operation rounded once, in the reference's order."""
    ps, T = check_config(config)
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    a, b = float(env["a"]), float(env["b"])
    nact = [p[1] for p in ps]
    idx = np.unravel_index(np.arange(T), nact)
    ratio = a / b
    scaled, quantity = [], []
    total = np.zeros(T, np.float64)
    for i, (kind, A, lo, hi) in enumerate(ps):
        x = idx[i].astype(np.float64) / (float(A) - 1.0 if kind == "QTable" else float(A))
        x = x * (hi - lo)
        x = x + lo
        scaled.append(x)
        quantity.append(ratio * x)
        total = total + quantity[-1]
    price = a - b * total
    price = np.where(price > 0.0, price, 0.0)
    reward = np.stack([price * qn for qn in quantity])
    return dict(T=T, n_actions=np.asarray(nact, np.int32), kinds=[p[0] for p in ps],
                price=np.ascontiguousarray(price), reward=np.ascontiguousarray(reward),
                scaled=np.ascontiguousarray(np.stack(scaled)))


def parse_options(opt, config):
    """training.greedy_cycles (true or a dict) -> the dict with every key filled in: rounds (re-seated rounds after the
    self-play round, 0 = none), scheme, against, seed (crossplay.pairings), steps (the length of the rows given to
    group_stats, 0 = none), horizon (None = deviation.default_horizon)."""
    from .crossplay import AGAINST, SCHEMES
    check_config(config)
    out = an.options("greedy_cycles", opt, DEFAULTS)
    for k in ("rounds", "steps", "seed"):
        if isinstance(out[k], bool) or not isinstance(out[k], (int, np.integer)):
            raise ValueError("training.greedy_cycles.%s must be an integer, got %r" % (k, out[k]))
        out[k] = int(out[k])
    if out["rounds"] < 0:
        raise ValueError("training.greedy_cycles.rounds=%d must be >= 0" % out["rounds"])
    if not 0 <= out["steps"] <= _lib.DEV_MAX_STEPS:
        raise ValueError("training.greedy_cycles.steps=%d out of [0, %d]" % (out["steps"], _lib.DEV_MAX_STEPS))
    if out["seed"] < 0:
        raise ValueError("training.greedy_cycles.seed=%d must be >= 0" % out["seed"])
    if out["scheme"] not in SCHEMES:
        raise ValueError("training.greedy_cycles.scheme must be one of %s, got %r" % (SCHEMES, out["scheme"]))
    if out["against"] not in AGAINST:
        raise ValueError("training.greedy_cycles.against must be one of %s, got %r" % (AGAINST, out["against"]))
    if out["horizon"] is not None:
        if isinstance(out["horizon"], bool) or not isinstance(out["horizon"], (int, np.integer)):
            raise ValueError("training.greedy_cycles.horizon must be an integer or null, got %r" % (out["horizon"],))
        out["horizon"] = int(out["horizon"])
        if not 1 <= out["horizon"] <= _lib.DEV_MAX_HORIZON:
            raise ValueError("training.greedy_cycles.horizon=%d out of [1, %d]" % (out["horizon"], _lib.DEV_MAX_HORIZON))
    return out


# ---------------------------------------------------------------------------------------------- the device calls
def _kinds(batch):
    return list(getattr(batch, "kinds", None) or ["QTable"] * batch.N)


def _batch_tables(batch, tabs):
    if tabs is None:
        tabs = tables(batch.config)
    if int(tabs["T"]) > MAX_TUPLES or list(tabs["n_actions"]) != [int(batch.cfg.n_actions[i]) for i in range(batch.N)]:
        raise ThrlError("tuple_play: the tables are not this batch's (actions %s)" % list(tabs["n_actions"]))
    return tabs


def extract(batch, tabs=None):
    """The strategies of every game of `batch` (a GameBatch, or a MixedGameBatch of QTable / Reinforce / ActorCritic
    agents) as a device int16 tensor [G, N, T] holding uint16 entries: thrl_tuple_policy.  The networks are read from
    batch.nn[i].params, the tables from batch.q; nothing of the batch is written."""
    import torch
    tabs = _batch_tables(batch, tabs)
    kinds = _kinds(batch)
    if not getattr(batch, "initialized", True):
        raise ThrlError("tuple_play: call init_tables() or set_tables() first")
    dev = batch.device
    T = int(tabs["T"])
    with torch.cuda.device(dev):
        price = torch.from_numpy(np.ascontiguousarray(tabs["price"], np.float64)).to(dev)
        pol = torch.empty((batch.G, batch.N, T), dtype=torch.int16, device=dev)
        a = _lib.TuplePolicyArgs()
        a.n_games, a.n_tuples = batch.G, T
        for i, k in enumerate(kinds):
            a.kind[i] = KINDS[k]
            if k != "QTable":
                a.nn_params[i] = batch.nn[i].params.data_ptr()
        a.price, a.tuple_policy = price.data_ptr(), pol.data_ptr()
        q = batch.q.data_ptr() if "QTable" in kinds else None
        _lib.check(batch.L.thrl_tuple_policy(ctypes.byref(batch.cfg), q, ctypes.byref(a), batch._stream()),
                   "thrl_tuple_policy")
        torch.cuda.synchronize(dev)
    return pol


def start_tuples(batch_or_prices, tabs):
    """int32 [G]: the first tuple whose price equals the state bit for bit, -1 when there is none.  Takes a batch (its
    .state), a torch tensor (any device; the result stays there) or an array of prices (numpy result)."""
    price = np.ascontiguousarray(tabs["price"], np.float64)
    # distinct price bit patterns, each with its first tuple
    bits, first = np.unique(price.view(np.int64), return_index=True)
    st = getattr(batch_or_prices, "state", batch_or_prices)
    try:
        import torch
        is_t = isinstance(st, torch.Tensor)
    except ImportError:
        is_t = False
    if not is_t:
        s = np.ascontiguousarray(np.asarray(st, np.float64).reshape(-1)).view(np.int64)
        at = np.minimum(np.searchsorted(bits, s), bits.size - 1)
        return np.where(bits[at] == s, first[at], -1).astype(np.int32)
    s = st.to(torch.float64).reshape(-1).contiguous().view(torch.int64)
    b = torch.from_numpy(bits).to(s.device)
    f = torch.from_numpy(first.astype(np.int64)).to(s.device)
    at = torch.clamp(torch.searchsorted(b, s), max=b.numel() - 1)
    return torch.where(b[at] == s, f[at], torch.full_like(at, -1)).to(torch.int32)


def identity(n_agents, n_games):
    from .crossplay import identity as ident
    return ident(n_agents, n_games)


def run(batch, seats=None, start=None, steps=0, rows=False, horizon=None, tuple_policy=None, group_stats=None,
        budget=ROW_BUDGET, tabs=None):
    """thrl_tuple_walk for the matches of `seats` on the games of `batch`.  seats: one round, int [N, M], or a list of
    rounds with the same M (crossplay.pairings); default: the identity (every game's own agents).  The strategies are
    extracted once (or taken from tuple_policy, a device int16 tensor [G, N, T] of extract()) and every round is played
    from them.  start int [M]: the start tuples (default: start_tuples of the state of seat 0's game; -1 refuses the
    match).  steps K > 0 with rows=True adds reward_rows / action_rows [K, N, M] per round, produced in chunks of at
    most `budget` bytes per device buffer; group_stats (a GroupSpec with G = M): the rows of all rounds are pooled per
    group on the device and returned raw under "group_stats".
    Returns a dict of numpy arrays: mu, lam, cycle_start [M], cycle_reward, cycle_action [N, M] for one round, with a
    leading round axis for a list; "start" [M] (per round for a list); "horizon"; "seats"."""
    import torch
    from .crossplay import MAX_POOLED_ROUNDS
    G, N = batch.G, batch.N
    tabs = _batch_tables(batch, tabs)
    T = int(tabs["T"])
    if seats is None:
        seats = identity(N, G)
    single = not isinstance(seats, (list, tuple)) and np.asarray(seats).ndim == 2
    rounds = [np.asarray(s) for s in ([seats] if single else list(seats))]
    if not rounds:
        raise ThrlError("tuple_play: no rounds")
    M = int(rounds[0].shape[-1]) if rounds[0].ndim == 2 else -1
    for s in rounds:
        if s.ndim != 2 or s.shape != (N, M) or M < 1 or s.dtype.kind not in "iu":
            raise ThrlError("tuple_play: every round must be an integer array [N=%d, M] with one M >= 1, got %s %s"
                            % (N, s.dtype, s.shape))
    K = int(steps)
    H = default_horizon([int(x) for x in tabs["n_actions"]]) if horizon is None else int(horizon)
    want = (bool(rows) or group_stats is not None) and K > 0
    if group_stats is not None and group_stats.G != M:
        raise ThrlError("group_stats spec is for %d games, the rounds have %d matches" % (group_stats.G, M))
    if group_stats is not None and len(rounds) > MAX_POOLED_ROUNDS:
        raise ThrlError("tuple_play: group_stats pools at most %d rounds, got %d" % (MAX_POOLED_ROUNDS, len(rounds)))
    dev = batch.device
    if tuple_policy is None:
        tuple_policy = extract(batch, tabs)
    else:
        an.check_policy(batch, tuple_policy, (G, N, T), "tuple_play", "tuple_policy")
    a = _lib.TupleWalkArgs()
    a.n_games, a.n_matches, a.n_tuples, a.n_steps, a.horizon = G, M, T, K, H
    res = {f: [] for f in OUT + ("start",)}
    host_r, host_a = [], []
    with torch.cuda.device(dev):
        d_rew = torch.from_numpy(np.ascontiguousarray(tabs["reward"], np.float64)).to(dev)
        d_sca = torch.from_numpy(np.ascontiguousarray(tabs["scaled"], np.float64)).to(dev)
        a.tuple_policy, a.reward, a.scaled = tuple_policy.data_ptr(), d_rew.data_ptr(), d_sca.data_ptr()
        s_given = None
        if start is not None:
            if isinstance(start, torch.Tensor):
                s_given = start.to(device=dev, dtype=torch.int32).reshape(M).contiguous()
            else:
                s_given = torch.from_numpy(np.ascontiguousarray(np.asarray(start).reshape(M).astype(np.int32))).to(dev)
        own = None
        st = group_stats.zeros(K, dev) if group_stats is not None and K > 0 else None
        chunk = max(1, min(K, int(budget) // (8 * N * M))) if want else 0
        for s in rounds:
            seat = torch.from_numpy(np.ascontiguousarray(s.astype(np.int32))).to(dev)
            if s_given is not None:
                t0 = s_given
            else:
                if own is None:
                    own = start_tuples(batch.state, tabs)
                ok = (seat[0] >= 0) & (seat[0] < G)
                t0 = torch.where(ok, own.index_select(0, seat[0].clamp(0, G - 1).to(torch.int64)),
                                 torch.full_like(seat[0], -1)).contiguous()
            out = {"mu": torch.zeros((M,), dtype=torch.int32, device=dev),
                   "lam": torch.zeros((M,), dtype=torch.int32, device=dev),
                   "cycle_start": torch.zeros((M,), dtype=torch.int32, device=dev),
                   "cycle_reward": torch.zeros((N, M), dtype=torch.float64, device=dev),
                   "cycle_action": torch.zeros((N, M), dtype=torch.float64, device=dev)}
            a.seat, a.start = seat.data_ptr(), t0.data_ptr()
            an.bind(a, out)
            rr_host, ra_host = [], []
            b0 = 0
            while True:
                k = min(chunk, K - b0) if want else 0
                rr = ra = None
                if k:
                    rr = torch.empty((k, N, M), dtype=torch.float64, device=dev)
                    ra = torch.empty((k, N, M), dtype=torch.float64, device=dev)
                a.row_begin, a.row_count = (b0, k) if k else (0, 0)
                a.reward_rows = rr.data_ptr() if rr is not None else None
                a.action_rows = ra.data_ptr() if ra is not None else None
                _lib.check(batch.L.thrl_tuple_walk(ctypes.byref(batch.cfg), ctypes.byref(a), batch._stream()),
                           "thrl_tuple_walk")
                if st is not None and k:
                    group_stats.reduce(batch.L, rr, ra, k, st, batch._stream(), at=b0)
                if rows and k:
                    rr_host.append(rr.cpu().numpy())
                    ra_host.append(ra.cpu().numpy())
                b0 += k
                if b0 >= K or not want:
                    break
            for f, t in out.items():
                res[f].append(t.cpu().numpy())
            res["start"].append(t0.cpu().numpy())
            if rows and want:
                host_r.append(np.concatenate(rr_host, axis=0))
                host_a.append(np.concatenate(ra_host, axis=0))
        torch.cuda.synchronize(dev)
        if st is not None:
            from .group_stats import to_numpy
            res["group_stats"] = to_numpy(st)
    for f in OUT + ("start",):
        res[f] = res[f][0] if single else np.stack(res[f])
    if rows and want:
        res["reward_rows"] = host_r[0] if single else np.stack(host_r)
        res["action_rows"] = host_a[0] if single else np.stack(host_a)
    res["horizon"] = H
    res["seats"] = rounds[0].astype(np.int32) if single else np.stack(rounds).astype(np.int32)
    return res


# ---------------------------------------------------------------------------------------------- host side
def summarize_self(self_play, ids, n_groups, nash, cartel):
    """One dict per group for the self-play round: self_play = mu, lam, start [G], cycle_reward [N, G]."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    mu, lam = np.asarray(self_play["mu"]).reshape(-1), np.asarray(self_play["lam"]).reshape(-1)
    start = np.asarray(self_play["start"]).reshape(-1)
    delta = profit_gain(self_play["cycle_reward"], nash, cartel)
    out = []
    for k in range(int(n_groups)):
        g = ids == k
        m = g & (mu >= 0)
        lk = lam[m]
        dk = delta[m & (lam > 0)]
        hist = [int(np.sum((lk >= lo) & (lk <= hi))) if hi is not None else int(np.sum(lk >= lo)) for lo, hi in LAM_BINS]
        qs = np.quantile(dk, QUANTILES) if dk.size else [None] * len(QUANTILES)
        out.append({"group": k, "matches": int(m.sum()), "no_start": int(np.sum(g & (start < 0))),
                    "cycles": int(np.sum(lk > 0)), "fixed_points": int(np.sum(lk == 1)), "lam_hist": hist,
                    "delta_mean": an.num(dk.mean()) if dk.size else None,
                    "delta_q25": an.num(qs[0]), "delta_q50": an.num(qs[1]), "delta_q75": an.num(qs[2])})
    return out


def summarize(games, self_play, ids, n_groups, nash, cartel):
    """The re-seated rounds: crossplay.summarize's rows, one per (group of seat 0, partner_group), with no_start (the
    matches of that cell refused for want of a start tuple) added.  games: seats [R, N, M], mu, lam, start [R, M],
    cycle_reward [R, N, M]."""
    from .crossplay import self_seat, summarize as xp_summarize
    rows = xp_summarize(games, self_play, ids, n_groups, nash, cartel)
    ids = np.asarray(ids, np.int64).reshape(-1)
    seats = np.asarray(games["seats"], np.int64)
    start = np.asarray(games["start"])
    if seats.ndim == 2:
        seats, start = seats[None], start[None]
    A = ids[seats[:, 0]]
    B = ids[seats[:, 1]] if seats.shape[1] > 1 else A
    away = np.stack([~self_seat(s) for s in seats])
    for r in rows:
        r["no_start"] = int(np.sum(away & (start < 0) & (A == r["group"]) & (B == r["partner_group"])))
    return rows


def combine(parts):
    """Per-match arrays of disjoint sets of games as one run's: concatenated along the match (= game) axis.  `seats`
    must hold global ids."""
    return an.combine(parts)


def describe(options, nash, cartel, T, self_summary, summary):
    """greedy_cycles.json's content."""
    return {"options": options, "nash": nash, "cartel": cartel, "T": int(T), "lam_bins": lam_bin_names(),
            "quantiles": list(QUANTILES), "self_play": self_summary, "summary": summary}


def save_games(d, games):
    """gcyc_seats int32 [R, N, G] (GLOBAL game ids; round 0 is the self-play round), gcyc_start int32 [R, G],
    gcyc_cycle int32 [R, 3, G] (mu, lam, cycle_start), gcyc_cycle_reward / gcyc_cycle_action [R, N, G]."""
    np.save(os.path.join(d, "gcyc_seats.npy"), np.asarray(games["seats"], np.int32))
    np.save(os.path.join(d, "gcyc_start.npy"), np.asarray(games["start"], np.int32))
    np.save(os.path.join(d, "gcyc_cycle.npy"),
            np.stack([games["mu"], games["lam"], games["cycle_start"]], axis=1).astype(np.int32))
    np.save(os.path.join(d, "gcyc_cycle_reward.npy"), np.asarray(games["cycle_reward"], np.float64))
    np.save(os.path.join(d, "gcyc_cycle_action.npy"), np.asarray(games["cycle_action"], np.float64))


def load_games(d):
    """The per-match arrays of one run directory, a leading round axis on each (round 0 = self-play); seats hold global
    game ids."""
    cyc = np.load(os.path.join(d, "gcyc_cycle.npy"))
    return {"seats": np.load(os.path.join(d, "gcyc_seats.npy")), "start": np.load(os.path.join(d, "gcyc_start.npy")),
            "mu": cyc[:, 0], "lam": cyc[:, 1], "cycle_start": cyc[:, 2],
            "cycle_reward": np.load(os.path.join(d, "gcyc_cycle_reward.npy")),
            "cycle_action": np.load(os.path.join(d, "gcyc_cycle_action.npy"))}


def analyse(batch, ids, n_groups, opt, group_stats=None, budget=ROW_BUDGET, tuple_policy=None):
    """The self-play round and the rounds of crossplay.pairings(ids, ...) for the options `opt` played on `batch` from
    the states it holds: the result of run() for the list [identity, round 1, ...], seats local.  tuple_policy: the
    strategies of extract() when the caller already has them."""
    from .crossplay import pairings
    seats = [identity(batch.N, batch.G)]
    if opt["rounds"] > 0:
        seats += pairings(ids, n_groups, opt["scheme"], opt["rounds"], opt["against"], opt["seed"], batch.N)
    return run(batch, seats, steps=opt["steps"], horizon=opt["horizon"], group_stats=group_stats, budget=budget,
               tuple_policy=tuple_policy)


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, spec=None, histograms=False, budget=ROW_BUDGET,
                    tuple_policy=None):
    """train_one's training.greedy_cycles outputs: the gcyc_*.npy files, with a spec and steps > 0 the rows' group
    statistics pooled over the rounds under prefix "gcyc" (group = seat 0's group), and greedy_cycles.json."""
    from . import trainer
    nash, cartel = optimal(config)
    tabs = tables(config)
    pooled = spec if opt["steps"] > 0 else None
    games = analyse(batch, ids, n_groups, opt, group_stats=pooled, budget=budget, tuple_policy=tuple_policy)
    off = int(batch.game_offset)
    save_games(exp_path, dict(games, seats=games["seats"].astype(np.int64) + off))
    if pooled is not None:
        trainer.save_group_stats(exp_path, "gcyc", games["group_stats"], spec, histograms)
    self_play = {f: games[f][0] for f in OUT + ("start",)}
    rest = {f: games[f][1:] for f in OUT + ("start", "seats")}
    summary = summarize(rest, self_play, ids, n_groups, nash, cartel) if rest["seats"].shape[0] else []
    opt = dict(opt, horizon_used=int(games["horizon"]), rounds_played=int(games["seats"].shape[0]))
    an.save_json(os.path.join(exp_path, "greedy_cycles.json"),
                 describe(opt, nash, cartel, tabs["T"], summarize_self(self_play, ids, n_groups, nash, cartel), summary))
