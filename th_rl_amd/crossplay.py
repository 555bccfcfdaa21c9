"""Cross-play of trained QTable games (thrl_crossplay, include/thrl.h): the robustness test that follows convergence,
the deviation test and the equilibrium check in the algorithmic-collusion literature (Eschenbaum, Mellgren, Zahn,
"Robust algorithmic collusion", 2022; Abada and Lambin 2023).  Those look at a game with the partners it was trained
with; this one seats agent 0 of game g against agent 1 of game h, which never met, lets them play greedily and finds
the limit cycle they end up in.  If the profit gain collapses, what was learned is a handshake between two particular
tables, not a strategy.

A round is a seat array int32 [N, M]: in match m seat i is taken by agent i of game seats[i][m] (roles are kept).
pairings() draws rounds with seat 0 of match m = game m, so every per-match array of such a round is game-shaped and a
group_stats spec of the batch applies unchanged.  run() extracts every game's greedy policy once (2 bytes per table
row) and plays any number of rounds from it; the per-match outputs (mu, lam, cycle_reward, cycle_action, optionally
the rows of the path from the start price) are defined in include/thrl.h.  summarize() gives, per (group A of seat 0,
group B of the partners):

    matches (self-seated and refused matches left out), cycles (lam > 0), fixed_points (lam == 1), lam_hist (LAM_BINS)
    delta_mean, delta_q25 / q50 / q75   the cross-play profit gain (deviation.profit_gain) over the matches with lam > 0
    delta_self_mean   the profit gain of the same matches' seat-0 games in their own self-play cycle
    retained          delta_mean / delta_self_mean (None unless the denominator is positive)
    seat_gain         per seat i, the mean over those matches of cycle_reward_i minus the self-play cycle reward of the
                      agent sitting there (agent i of game seats[i][m]): who gains and who is exploited

Statistics that have no matches are None.  In a sharded run (th_rl_amd.launch) partners are drawn INSIDE a shard -- the
tables of other ranks are not fetched -- so a sharded run's pairings are not the unsharded run's; the saved seats are
global game ids, so the merged files describe themselves.
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import analysis as an
from ._lib import ThrlError
from .analysis import save_json  # noqa: F401  (xp.save_json stays a public name)
from .deviation import LAM_BINS, QUANTILES, ROW_BUDGET, default_horizon, lam_bin_names, optimal, profit_gain

DEFAULTS = dict(rounds=8, scheme="rotate", against="own", steps=0, horizon=None, seed=0)
SCHEMES = ("rotate", "random")
AGAINST = ("own", "all")
MAX_POOLED_ROUNDS = 16
NEURAL_FOLLOW_UP = ("cross-play runs on QTable agents only; neural agents (greedy = argmax pi) are a "
                    "follow-up on the mixed path's policy tables")


def check_config(config):
    """ValueError for a config with neural agents (cross-play needs every agent's greedy table)."""
    an.check_qtable_only(config, "crossplay", NEURAL_FOLLOW_UP)


def parse_options(opt, config):
    """training.crossplay (true or a dict) -> the dict with every key filled in: rounds, scheme, against, steps (the
    length of the response rows, 0 = none), horizon (None = deviation.default_horizon), seed, and tables when given."""
    check_config(config)
    out = an.options("crossplay", opt, DEFAULTS, tables=True)
    for k in ("rounds", "steps", "seed"):
        if isinstance(out[k], bool) or not isinstance(out[k], (int, np.integer)):
            raise ValueError("training.crossplay.%s must be an integer, got %r" % (k, out[k]))
        out[k] = int(out[k])
    if out["rounds"] < 1:
        raise ValueError("training.crossplay.rounds=%d must be >= 1" % out["rounds"])
    if not 0 <= out["steps"] <= _lib.DEV_MAX_STEPS:
        raise ValueError("training.crossplay.steps=%d out of [0, %d]" % (out["steps"], _lib.DEV_MAX_STEPS))
    if out["seed"] < 0:
        raise ValueError("training.crossplay.seed=%d must be >= 0" % out["seed"])
    if out["scheme"] not in SCHEMES:
        raise ValueError("training.crossplay.scheme must be one of %s, got %r" % (SCHEMES, out["scheme"]))
    if out["against"] not in AGAINST:
        raise ValueError("training.crossplay.against must be one of %s, got %r" % (AGAINST, out["against"]))
    if out["horizon"] is not None:
        out["horizon"] = int(out["horizon"])
        if not 1 <= out["horizon"] <= _lib.DEV_MAX_HORIZON:
            raise ValueError("training.crossplay.horizon=%d out of [1, %d]" % (out["horizon"], _lib.DEV_MAX_HORIZON))
    return out


# ---------------------------------------------------------------------------------------------- pairings (host)
def pairings(ids, n_groups, scheme="rotate", rounds=1, against="own", seed=0, n_agents=2):
    """The rounds of a cross-play design: a list of int32 [N, G] seat arrays with seat 0 of match m = game m.

    ids [G]: group of every game, in [0, n_groups).  pos(m) = the position of game m among its own group's games in
    ascending id order.  With B the target group and n_B its number of games:
      scheme "rotate": seat i >= 1 of match m in round k = 1 .. rounds takes B's game at position
                       (pos(m) + i * k) mod n_B;
      scheme "random": a numpy.random.default_rng(seed) permutation `perm` of B's positions per seat and round, seat i
                       taking B's game at position perm[pos(m) mod n_B].  The permutations are drawn in the order
                       block, round, target group, seat.
    against "own": B = game m's own group, `rounds` rounds.  against "all": one block of `rounds` rounds per target
    group B = 0 .. n_groups - 1 (round index B * rounds + k - 1), the partners of EVERY game drawn from B: the
    group x group matrix.  A target group without games leaves every seat of the match on game m itself.
    A match in which a seat i >= 1 lands on game m itself is no cross-play: self_seat() flags it and summarize()
    leaves it out (a group of one game has nobody else to meet)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    G, N, R, ng = ids.size, int(n_agents), int(rounds), int(n_groups)
    if scheme not in SCHEMES:
        raise ValueError("pairings: scheme must be one of %s, got %r" % (SCHEMES, scheme))
    if against not in AGAINST:
        raise ValueError("pairings: against must be one of %s, got %r" % (AGAINST, against))
    if R < 1 or N < 1 or ng < 1:
        raise ValueError("pairings: rounds, n_agents and n_groups must be >= 1")
    if G and (ids.min() < 0 or ids.max() >= ng):
        raise ValueError("pairings: group ids must lie in [0, %d)" % ng)
    members = [np.flatnonzero(ids == k) for k in range(ng)]        # ascending game ids
    pos = np.zeros(G, np.int64)
    for mem in members:
        pos[mem] = np.arange(mem.size)
    rng = np.random.default_rng(int(seed)) if scheme == "random" else None
    own = np.arange(G, dtype=np.int64)
    out = []
    for block in ([None] if against == "own" else list(range(ng))):
        for k in range(1, R + 1):
            seats = np.tile(own, (N, 1))
            for B in range(ng):
                src = np.flatnonzero(ids == B) if block is None else (own if B == block else None)
                if src is None or members[B].size == 0 or src.size == 0:
                    continue
                n_B = members[B].size
                for i in range(1, N):
                    if rng is None:
                        at = (pos[src] + i * k) % n_B
                    else:
                        at = rng.permutation(n_B)[pos[src] % n_B]
                    seats[i, src] = members[B][at]
            out.append(seats.astype(np.int32))
    return out


def self_seat(seats):
    """bool [M]: matches in which some seat i >= 1 holds the game of seat 0 (no cross-play)."""
    s = np.asarray(seats)
    return (s[1:] == s[:1]).any(axis=0) if s.shape[0] > 1 else np.ones(s.shape[1], bool)


def identity(n_agents, n_games):
    """The self-play round: every seat of match m held by game m."""
    return np.tile(np.arange(int(n_games), dtype=np.int32), (int(n_agents), 1))


# ---------------------------------------------------------------------------------------------- the device call
def policy_entries(batch):
    return sum(int(batch.cfg.n_states[i]) + 1 for i in range(batch.N))


def extract(batch, q=None):
    """The greedy policies of every game of `batch` (or of the tables q) as a device int16 tensor [G, P] holding
    uint16 entries, the layout of thrl_policy_track: thrl_crossplay's extraction pass with one throw-away match."""
    import torch
    q = an.tables_tensor(batch, q, "crossplay")
    dev = batch.device
    with torch.cuda.device(dev):
        pol = torch.empty((batch.G, policy_entries(batch)), dtype=torch.int16, device=dev)
        a = _lib.CrossplayArgs()
        a.n_games, a.n_matches, a.horizon = batch.G, 1, 1
        keep = [torch.zeros((batch.N, 1), dtype=torch.int32, device=dev), batch.state[:1].contiguous(),
                torch.zeros((2,), dtype=torch.int32, device=dev), torch.zeros((2, batch.N), dtype=torch.float64, device=dev)]
        a.seat, a.state0, a.policy = keep[0].data_ptr(), keep[1].data_ptr(), pol.data_ptr()
        a.mu, a.lam = keep[2][:1].data_ptr(), keep[2][1:].data_ptr()
        a.cycle_reward, a.cycle_action = keep[3][0].data_ptr(), keep[3][1].data_ptr()
        _lib.check(batch.L.thrl_crossplay(ctypes.byref(batch.cfg), q.data_ptr(), ctypes.byref(a), batch._stream()),
                   "thrl_crossplay")
        torch.cuda.synchronize(dev)
    return pol


def run(batch, seats, steps=0, horizon=None, state0=None, rows=False, group_stats=None, q=None, policy=None,
        budget=ROW_BUDGET):
    """thrl_crossplay for the matches of `seats` on the games of `batch` (a GameBatch or an all-QTable MixedGameBatch;
    see GameBatch.crossplay).  seats: one round, int [N, M], or a list of rounds with the same M (pairings()); every
    entry is range-checked here.  The policies are extracted once, by the first round's call, and every round is
    played from them; policy (a device int16 / uint16-bits tensor [G, P], e.g. convergence.Tracker.policy or
    extract()) is played as it is and no table is read.  q: a device tensor shaped and typed like batch.q read in place
    of the batch's tables.  state0 [M]: the start prices (default: the state of seat 0's game).  steps K > 0 with
    rows=True adds reward_rows / action_rows [K, N, M] per round (the path from the start price), produced in chunks
    of at most `budget` bytes per device buffer; group_stats (a GroupSpec with G = M): the rows of all rounds are
    pooled per group of the spec on the device and returned raw under "group_stats".
    Returns a dict of numpy arrays: mu, lam [M], cycle_reward, cycle_action [N, M] for one round, with a leading
    round axis for a list; "horizon"; "seats"."""
    import torch
    G, N = batch.G, batch.N
    single = not isinstance(seats, (list, tuple)) and np.asarray(seats).ndim == 2
    rounds = [np.asarray(s) for s in ([seats] if single else list(seats))]
    if not rounds:
        raise ThrlError("crossplay: no rounds")
    M = int(rounds[0].shape[-1]) if rounds[0].ndim == 2 else -1
    for s in rounds:
        if s.ndim != 2 or s.shape != (N, M) or M < 1 or s.dtype.kind not in "iu":
            raise ThrlError("crossplay: every round must be an integer array [N=%d, M] with one M >= 1, got %s %s"
                            % (N, s.dtype, s.shape))
        if s.min() < 0 or s.max() >= G:
            raise ThrlError("crossplay: seats must lie in [0, %d), got [%d, %d]" % (G, int(s.min()), int(s.max())))
    K = int(steps)
    n_actions = [int(batch.cfg.n_actions[i]) for i in range(N)]
    H = default_horizon(n_actions) if horizon is None else int(horizon)
    want = (bool(rows) or group_stats is not None) and K > 0
    if group_stats is not None and group_stats.G != M:
        raise ThrlError("group_stats spec is for %d games, the rounds have %d matches" % (group_stats.G, M))
    if group_stats is not None and len(rounds) > MAX_POOLED_ROUNDS:
        raise ThrlError("crossplay: group_stats pools at most %d rounds (the fixed-point sums of a spec are sized for "
                        "one value per game, with a headroom of 16 for values inside its ranges), got %d"
                        % (MAX_POOLED_ROUNDS, len(rounds)))
    dev = batch.device
    given = policy is not None
    if given:
        an.check_policy(batch, policy, (G, policy_entries(batch)), "crossplay")
    else:
        q = an.tables_tensor(batch, q, "crossplay")
    a = _lib.CrossplayArgs()
    a.n_games, a.n_matches, a.n_steps, a.horizon = G, M, K, H
    res = {f: [] for f in ("mu", "lam", "cycle_reward", "cycle_action")}
    host_r, host_a = [], []
    with torch.cuda.device(dev):
        if not given:
            policy = torch.empty((G, policy_entries(batch)), dtype=torch.int16, device=dev)
        a.policy = policy.data_ptr()
        s0 = None if state0 is None else an.state0_tensor(batch, state0, M, "crossplay")
        st = group_stats.zeros(K, dev) if group_stats is not None and K > 0 else None
        chunk = max(1, min(K, int(budget) // (8 * N * M))) if want else 0
        for r, s in enumerate(rounds):
            seat = torch.from_numpy(np.ascontiguousarray(s.astype(np.int32))).to(dev)
            start = s0 if s0 is not None else batch.state.index_select(0, seat[0].to(torch.int64))
            out = {"mu": torch.zeros((M,), dtype=torch.int32, device=dev),
                   "lam": torch.zeros((M,), dtype=torch.int32, device=dev),
                   "cycle_reward": torch.zeros((N, M), dtype=torch.float64, device=dev),
                   "cycle_action": torch.zeros((N, M), dtype=torch.float64, device=dev)}
            a.seat, a.state0 = seat.data_ptr(), start.data_ptr()
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
                a.flags = _lib.XPLAY_POLICY_GIVEN if (given or r > 0 or b0 > 0) else 0
                _lib.check(batch.L.thrl_crossplay(ctypes.byref(batch.cfg), None if given else q.data_ptr(),
                                                  ctypes.byref(a), batch._stream()), "thrl_crossplay")
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
            if rows and want:
                host_r.append(np.concatenate(rr_host, axis=0))
                host_a.append(np.concatenate(ra_host, axis=0))
        torch.cuda.synchronize(dev)
        if st is not None:
            from .group_stats import to_numpy
            res["group_stats"] = to_numpy(st)
    for f in ("mu", "lam", "cycle_reward", "cycle_action"):
        res[f] = res[f][0] if single else np.stack(res[f])
    if rows and want:
        res["reward_rows"] = host_r[0] if single else np.stack(host_r)
        res["action_rows"] = host_a[0] if single else np.stack(host_a)
    res["horizon"] = H
    res["seats"] = rounds[0].astype(np.int32) if single else np.stack(rounds).astype(np.int32)
    return res


# ---------------------------------------------------------------------------------------------- host side
def summarize(games, self_play, ids, n_groups, nash, cartel):
    """The summary rows, one per (group A of seat 0, group B of the partners) in A-major order.  games: seats
    [R, N, M] (indices into `ids` and into self_play's game axis), mu, lam [R, M], cycle_reward [R, N, M];
    self_play: lam [G], cycle_reward [N, G] of every game's own cycle.  B is the group of seat 1's game (pairings()
    draws all partners of a match from one group); with one agent B = A."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    seats = np.asarray(games["seats"], np.int64)
    if seats.ndim == 2:
        games = {f: np.asarray(games[f])[None] for f in ("seats", "mu", "lam", "cycle_reward")}
        seats = np.asarray(games["seats"], np.int64)
    R, N, M = seats.shape
    mu, lam = np.asarray(games["mu"]).reshape(R, M), np.asarray(games["lam"]).reshape(R, M)
    cr = np.asarray(games["cycle_reward"], np.float64).reshape(R, N, M)
    self_lam = np.asarray(self_play["lam"]).reshape(-1)
    self_cr = np.asarray(self_play["cycle_reward"], np.float64)
    self_delta = profit_gain(self_cr, nash, cartel)
    A = ids[seats[:, 0]]                                        # [R, M]
    B = ids[seats[:, 1]] if N > 1 else A
    keep = np.stack([~self_seat(seats[r]) for r in range(R)]) & (mu >= 0)
    delta = np.stack([profit_gain(cr[r], nash, cartel) for r in range(R)])
    out = []
    for ga in range(int(n_groups)):
        for gb in range(int(n_groups)):
            m = keep & (A == ga) & (B == gb)
            lk = lam[m]
            cyc = m & (lam > 0)
            dk = delta[cyc]
            hist = [int(np.sum((lk >= lo) & (lk <= hi))) if hi is not None else int(np.sum(lk >= lo))
                    for lo, hi in LAM_BINS]
            qs = np.quantile(dk, QUANTILES) if dk.size else [None] * len(QUANTILES)
            both = cyc & (self_lam[seats[:, 0]] > 0)
            ds = self_delta[seats[:, 0]][both]
            d_mean = an.num(dk.mean()) if dk.size else None
            s_mean = an.num(ds.mean()) if ds.size else None
            gains = []
            for i in range(N):
                ok = cyc & (self_lam[seats[:, i]] > 0)
                diff = cr[:, i][ok] - self_cr[i][seats[:, i]][ok]
                gains.append(an.num(diff.mean()) if diff.size else None)
            out.append({"group": ga, "partner_group": gb, "matches": int(m.sum()), "cycles": int(cyc.sum()),
                        "fixed_points": int(np.sum(lk == 1)), "lam_hist": hist, "delta_mean": d_mean,
                        "delta_q25": an.num(qs[0]), "delta_q50": an.num(qs[1]), "delta_q75": an.num(qs[2]),
                        "delta_self_mean": s_mean,
                        "retained": d_mean / s_mean if d_mean is not None and s_mean is not None and s_mean > 0 else None,
                        "seat_gain": gains})
    return out


GAME_FILES = ("seats", "mu", "lam", "cycle_reward", "cycle_action")


def combine(parts):
    """Per-match arrays of disjoint shards as one run's: concatenated along the match (= game) axis.  `seats` must hold
    global ids (load_games), so that they index the concatenation (local_seats)."""
    return an.combine(parts)


def describe(options, nash, cartel, summary):
    """crossplay.json's content."""
    return {"options": options, "nash": nash, "cartel": cartel, "lam_bins": lam_bin_names(),
            "quantiles": list(QUANTILES), "summary": summary}


# ---------------------------------------------------------------------------------------------- artefacts
def save_games(d, games, self_play):
    """xplay_seats int32 [R, N, G] (GLOBAL game ids), xplay_cycle int32 [R, 2, G] (mu, lam), xplay_cycle_reward /
    xplay_cycle_action [R, N, G]; the self-play round the summary compares with: xplay_self_cycle int32 [2, G],
    xplay_self_reward [N, G]."""
    np.save(os.path.join(d, "xplay_seats.npy"), np.asarray(games["seats"], np.int32))
    np.save(os.path.join(d, "xplay_cycle.npy"), np.stack([games["mu"], games["lam"]], axis=1).astype(np.int32))
    np.save(os.path.join(d, "xplay_cycle_reward.npy"), np.asarray(games["cycle_reward"], np.float64))
    np.save(os.path.join(d, "xplay_cycle_action.npy"), np.asarray(games["cycle_action"], np.float64))
    np.save(os.path.join(d, "xplay_self_cycle.npy"), np.stack([self_play["mu"], self_play["lam"]]).astype(np.int32))
    np.save(os.path.join(d, "xplay_self_reward.npy"), np.asarray(self_play["cycle_reward"], np.float64))


def load_games(d):
    """(games, self_play) of one run directory (or shard); games["seats"] holds global game ids."""
    cyc = np.load(os.path.join(d, "xplay_cycle.npy"))
    sc = np.load(os.path.join(d, "xplay_self_cycle.npy"))
    games = {"seats": np.load(os.path.join(d, "xplay_seats.npy")), "mu": cyc[:, 0], "lam": cyc[:, 1],
             "cycle_reward": np.load(os.path.join(d, "xplay_cycle_reward.npy")),
             "cycle_action": np.load(os.path.join(d, "xplay_cycle_action.npy"))}
    return games, {"mu": sc[0], "lam": sc[1], "cycle_reward": np.load(os.path.join(d, "xplay_self_reward.npy"))}


def local_seats(games, offset):
    """games with the global ids of `seats` turned into indices of a run whose first game has global id `offset`."""
    return dict(games, seats=np.asarray(games["seats"], np.int64) - int(offset))


def analyse(batch, ids, n_groups, opt, state0=None, q=None, policy=None, group_stats=None, budget=ROW_BUDGET):
    """The rounds of pairings(ids, ...) for the options `opt` (parse_options) played on `batch`, and the self-play
    round: (games, self_play), games["seats"] local."""
    seats = pairings(ids, n_groups, opt["scheme"], opt["rounds"], opt["against"], opt["seed"], batch.N)
    if policy is None:
        policy = extract(batch, q)
    games = run(batch, seats, steps=opt["steps"], horizon=opt["horizon"], state0=state0, policy=policy,
                group_stats=group_stats, budget=budget)
    self_play = run(batch, identity(batch.N, batch.G), horizon=opt["horizon"], state0=state0, policy=policy)
    return games, self_play


def merged(shards, out, config, opt, ids, n_groups, first):
    """crossplay.json and xplay_*.npy of a sharded run (launch.merge_analysis).  Every shard drew its partners INSIDE
    the shard -- the tables of other ranks are not fetched -- so these are not the pairings of the unsharded run; the
    saved seats are global game ids, so the merged files say who met whom."""
    loaded = [load_games(s) for s in shards]
    games, self_play = combine(g for g, _ in loaded), combine(s for _, s in loaded)
    save_games(out, games, self_play)
    nash, cartel = optimal(config)
    offset = int(config.get("training", {}).get("game_offset", 0))
    return describe(opt, nash, cartel, summarize(local_seats(games, offset), self_play, ids, n_groups, nash, cartel))


def write_artefacts(exp_path, batch, config, opt, ids, n_groups, spec=None, histograms=False, budget=ROW_BUDGET,
                    q=None, state0=None):
    """train_one's training.crossplay outputs: the xplay_*.npy files, with a spec and steps > 0 the response rows'
    group statistics pooled over the rounds under prefix "xplay" (group = seat 0's group), and crossplay.json.
    q / state0 (device tensors): the tables and start prices played in place of the batch's
    (opt["tables"] == "converged")."""
    from . import trainer
    nash, cartel = optimal(config)
    games, self_play = analyse(batch, ids, n_groups, opt, state0=state0, q=q,
                               group_stats=spec if opt["steps"] > 0 else None, budget=budget)
    off = int(batch.game_offset)
    save_games(exp_path, dict(games, seats=games["seats"].astype(np.int64) + off), self_play)
    if spec is not None and opt["steps"] > 0:
        trainer.save_group_stats(exp_path, "xplay", games["group_stats"], spec, histograms)
    summary = summarize(games, self_play, ids, n_groups, nash, cartel)
    opt = dict(opt, horizon_used=int(games["horizon"]), rounds_played=int(games["seats"].shape[0]))
    save_json(os.path.join(exp_path, "crossplay.json"), describe(opt, nash, cartel, summary))
