"""What the post-training analyses share: the one table of `training` keys (REGISTRY), the host-side helpers every
analysis module used to carry a copy of, and the analysis methods of GameBatch and MixedGameBatch (AnalysisMethods).

The helpers come in three sections.  "summaries and JSON": num, mean, frac, quantiles, save_json, combine.  "options":
options, check_qtable_only, and for the long-run chain analyses (stationary, tuple_stationary, sampled_play)
check_own_noise and chain_options.  "device arguments": what a run() does around its library call -- games (n_games ->
G), state0_tensor, start_tensor, tables_tensor, check_policy, resolve_noise, bind_tables (the per-config tables, checked
and uploaded), outputs / bind / fetch (the output dict).  Each takes the caller's message prefix, so an error names the
analysis that raised it.

REGISTRY is read by trainer.train_one (parse the options before training, write the artefacts after it),
launch (which keys merge over shards and how) and the tests; utils has `<reader>_summary` / `<reader>_games` per record.
Order is execution order: a later analysis may read what an earlier one left (`after`).
"""
import collections
import ctypes
import importlib
import json

import numpy as np

from . import _lib
from ._lib import ThrlError

QUANTILES = (0.25, 0.5, 0.75)

# key         the `training` key; `<key>.json` is the analysis's summary file
# module      the module of th_rl_amd that holds it, parse / write: the names of its option parser and artefact writer
# reader      utils.<reader>_summary and utils.<reader>_games read the results
# converged   honours "tables": "converged" (the writer takes q= and state0=)
# tuple_policy  "extract": the run extracts every agent's strategy in tuple form once and the writer takes it;
#             "use": the writer takes it when another key had it extracted
# rows        the writer takes spec=, histograms= and budget= (response rows reduced per group)
# merge       th_rl_amd.launch merges the shards through the module's merged() hook
# copy        option keys the merge copies from shard 0's JSON (what only a run knows)
# after       (keyword, earlier key) pairs: the writer takes what that key's writer returned (None when it did not run)
Analysis = collections.namedtuple("Analysis", "key module parse write reader converged tuple_policy rows merge copy after")


def _a(key, module, reader, parse="parse_options", write="write_artefacts", converged=False, tuple_policy=None,
       rows=False, merge=False, copy=(), after=()):
    return Analysis(key, module, parse, write, reader, converged, tuple_policy, rows, merge, tuple(copy), tuple(after))


REGISTRY = (
    _a("convergence", "convergence", "convergence", merge=True),
    _a("deviation", "deviation", "deviation", converged=True, rows=True, merge=True, copy=("horizon_used", "tables")),
    _a("equilibrium", "equilibrium", "equilibrium", converged=True, merge=True, copy=("tables",)),   # dev_cycle_reward.npy
    _a("crossplay", "crossplay", "crossplay", converged=True, rows=True, merge=True,
       copy=("horizon_used", "rounds_played", "tables")),
    _a("attractors", "attractors", "attractor", converged=True, merge=True, copy=("tables",)),
    _a("stationary", "stationary", "stationary", converged=True, merge=True, copy=("tables",),
       after=(("with_attractors", "attractors"),)),
    _a("greedy_cycles", "tuple_play", "greedy_cycle", tuple_policy="extract", rows=True),
    _a("greedy_deviation", "tuple_analysis", "greedy_deviation", "parse_deviation_options", "write_deviation",
       tuple_policy="extract", rows=True),
    _a("greedy_equilibrium", "tuple_analysis", "greedy_equilibrium", "parse_equilibrium_options", "write_equilibrium",
       tuple_policy="extract", after=(("deviation", "greedy_deviation"),)),
    _a("greedy_attractors", "tuple_analysis", "greedy_attractor", "parse_attractor_options", "write_attractors",
       tuple_policy="extract"),
    _a("greedy_stationary", "tuple_stationary", "greedy_stationary", tuple_policy="extract"),
    _a("sampled_play", "sampled_play", "sampled_play", tuple_policy="use", rows=True,       # the sub-key "deviation"'s curves
       after=(("with_cycles", "greedy_cycles"),)),
)


def record(key):
    for a in REGISTRY:
        if a.key == key:
            return a
    raise KeyError("no analysis %r (known: %s)" % (key, ", ".join(a.key for a in REGISTRY)))


def module_of(a):
    return importlib.import_module("th_rl_amd." + a.module)


def enabled(training, key):
    """True when the `training` block asks for `key` (present, not null, not false)."""
    v = training.get(key)
    return v is not None and v is not False


# ---------------------------------------------------------------------------------------------- summaries and JSON
def num(x):
    """A JSON-safe number: None for None, NaN and infinities."""
    return None if x is None or not np.isfinite(x) else float(x)


def mean(x):
    x = np.asarray(x, np.float64)
    return num(x.mean()) if x.size else None


def frac(mask):
    return num(mask.mean()) if mask.size else None


def quantiles(row, name, x):
    """row[<name>_q25 / q50 / q75] = the QUANTILES of x (None without values)."""
    x = np.asarray(x, np.float64)
    qs = np.quantile(x, QUANTILES) if x.size else [None] * len(QUANTILES)
    for qq, v in zip(QUANTILES, qs):
        row["%s_q%d" % (name, int(round(qq * 100)))] = num(v)


def save_json(path, content):
    with open(path, "w") as f:
        json.dump(content, f, indent=2)


def combine(parts, other=None, only=None):
    """Per-game arrays of disjoint shards (in global game order) as one run's: concatenated along the game axis, the
    last one, except for the fields of `other` (field -> axis); only: the fields kept (default all)."""
    parts = list(parts)
    other = other or {}
    return {f: np.concatenate([np.asarray(p[f]) for p in parts], axis=other.get(f, -1))
            for f in parts[0] if only is None or f in only}


# ---------------------------------------------------------------------------------------------- options
def check_qtable_only(config, key, follow_up):
    """ValueError for a config with neural agents (the QTable analyses need every agent's greedy table)."""
    kinds = [a.get("name", "QTable") for a in config["agents"]]
    if any(k != "QTable" for k in kinds):
        raise ValueError("training.%s: agents %s: %s" % (key, kinds, follow_up))


def options(key, opt, defaults, tables=False):
    """training.<key> (true or a dict) -> dict(defaults) updated with it; ValueError for another type, for a key that
    is neither in `defaults` nor (with tables) "tables", and for a "tables" other than "final" or "converged"."""
    name = "training." + key
    if opt is True:
        opt = {}
    if not isinstance(opt, dict):
        raise ValueError("%s must be true or a dict, got %r" % (name, opt))
    known = set(defaults) | ({"tables"} if tables else set())
    bad = set(opt) - known
    if bad:
        raise ValueError("%s: unknown keys %s (known: %s)" % (name, sorted(bad), ", ".join(sorted(known))))
    out = dict(defaults)
    out.update(opt)
    if "tables" in out and out["tables"] not in ("final", "converged"):
        raise ValueError("%s.tables must be 'final' or 'converged', got %r" % (name, out["tables"]))
    return out


def check_own_noise(config, name):
    """ValueError when `name` asks for the run's own noise and the run has none: refused before training, as the
    batch would after it."""
    env = dict(_lib.ENV_DEFAULTS, **config["environment"])
    sweep = config.get("training", {}).get("sweep") or {}
    if float(env["noise_prob"]) == 0.0 and "noise_prob" not in sweep:
        raise ValueError("%s: the environment has noise_prob = 0: give the noise_prob to analyse" % name)


def chain_options(out, name, starts):
    """The checks a chain analysis's parsed options share: start in `starts`, tol a number >= 0 (made a float),
    max_iters an integer in [1, STAT_MAX_ITERS], pi a bool."""
    if out["start"] not in starts:
        raise ValueError("%s.start must be one of %s, got %r" % (name, starts, out["start"]))
    if isinstance(out["tol"], bool) or not isinstance(out["tol"], (int, float)) or not out["tol"] >= 0.0:
        raise ValueError("%s.tol must be a number >= 0, got %r" % (name, out["tol"]))
    out["tol"] = float(out["tol"])
    if isinstance(out["max_iters"], bool) or not isinstance(out["max_iters"], int) \
            or not 1 <= out["max_iters"] <= _lib.STAT_MAX_ITERS:
        raise ValueError("%s.max_iters must be an integer in [1, %d], got %r" % (name, _lib.STAT_MAX_ITERS, out["max_iters"]))
    if not isinstance(out["pi"], bool):
        raise ValueError("%s.pi must be true or false, got %r" % (name, out["pi"]))


# ---------------------------------------------------------------------------------------------- device arguments
def games(batch, n_games, what):
    """G: the first n_games (default all) games of the batch."""
    G = batch.G if n_games is None else int(n_games)
    if not 1 <= G <= batch.G:
        raise ThrlError("%s: n_games=%r out of [1, %d]" % (what, n_games, batch.G))
    return G


def start_tensor(start, G, dev, what):
    """Given start tuples (a tensor or an array) as a contiguous device int32 tensor [G]."""
    import torch
    if isinstance(start, torch.Tensor):
        t0 = start.to(device=dev, dtype=torch.int32).reshape(-1)[:G].contiguous()
    else:
        t0 = torch.from_numpy(np.ascontiguousarray(np.asarray(start).reshape(-1)[:G].astype(np.int32))).to(dev)
    if t0.numel() != G:
        raise ThrlError("%s: start must hold %d tuples" % (what, G))
    return t0


def resolve_noise(batch, noise_prob, G, what, zero_ok=False):
    """(scalar or None, device float64 [G] or None) for a noise_prob argument: None = the batch's per-game sweep array if
    it has one, else the config's value (0 asks for an explicit one); a number in (0, 1], or with zero_ok in [0, 1]; or an
    array / tensor [G] (device data: the kernel refuses a game whose entry is out of range)."""
    import torch
    if noise_prob is None:
        sw = getattr(batch, "sweep", None) or {}
        if "noise_prob" in sw:
            return None, sw["noise_prob"][:G].to(torch.float64).contiguous()
        noise_prob = float(batch.cfg.noise_prob)
        if noise_prob == 0.0:
            raise ThrlError("%s: the batch was configured without env noise (noise_prob = 0): pass the "
                            "noise_prob to analyse explicitly" % what)
    if isinstance(noise_prob, torch.Tensor):
        arr = noise_prob.to(device=batch.device, dtype=torch.float64).reshape(-1)[:G].contiguous()
    elif np.ndim(noise_prob) > 0:
        arr = torch.from_numpy(np.ascontiguousarray(np.asarray(noise_prob, np.float64).reshape(-1)[:G])).to(batch.device)
    else:
        p = float(noise_prob)
        if not (0.0 <= p if zero_ok else 0.0 < p) or not p <= 1.0:
            raise ThrlError("%s: noise_prob=%r out of %s0, 1]" % (what, noise_prob, "[" if zero_ok else "("))
        return p, None
    if arr.numel() != G:
        raise ThrlError("%s: noise_prob must hold %d values" % (what, G))
    return None, arr


def bind_tables(a, tabs, fields, dev, what):
    """The per-config tables `fields` = (field, shape, numpy dtype) of `tabs`, each made contiguous, checked against its
    shape, copied to `dev` and bound to a.<field>.  Returns the device tensors: the caller keeps them until the call is
    done."""
    import torch
    keep = []
    for f, shape, dt in fields:
        x = np.ascontiguousarray(tabs[f], dt)
        if x.shape != shape:
            raise ThrlError("%s: table %s has shape %s, expected %s" % (what, f, x.shape, shape))
        keep.append(torch.from_numpy(x).to(dev))
        setattr(a, f, keep[-1].data_ptr())
    return keep


def outputs(dev, *groups):
    """The output dict of a run(): every group is (fields, shape, torch dtype name); {field: zeroed tensor on dev}."""
    import torch
    return {f: torch.zeros(shape, dtype=getattr(torch, dt), device=dev) for fields, shape, dt in groups for f in fields}


def bind(a, out):
    """a.<field> = the device address of every output tensor."""
    for f, t in out.items():
        setattr(a, f, t.data_ptr())


def fetch(out):
    """The outputs as numpy arrays (synchronises through the copies)."""
    return {f: t.cpu().numpy() for f, t in out.items()}


def state0_tensor(batch, state0, G, what):
    """The start prices of the first G games (matches) as a contiguous device float64 tensor [G]: the batch's state
    for None, else the first G of a tensor or array."""
    import torch
    dev = batch.device
    if state0 is None:
        return batch.state[:G].contiguous()
    if isinstance(state0, torch.Tensor):
        s0 = state0.to(device=dev, dtype=torch.float64).reshape(-1)[:G].contiguous()
    else:
        s0 = torch.from_numpy(np.ascontiguousarray(np.asarray(state0, np.float64).reshape(-1)[:G])).to(dev)
    if s0.numel() != G:
        raise ThrlError("%s: state0 must hold %d prices" % (what, G))
    return s0


def tables_tensor(batch, q, what):
    """batch.q for None, else q checked to be shaped, typed and placed like it."""
    if q is None:
        return batch.q
    if tuple(q.shape) != tuple(batch.q.shape) or q.dtype != batch.q.dtype or q.device != batch.q.device \
            or not q.is_contiguous():
        raise ThrlError("%s: q must be a contiguous %s tensor %s on %s"
                        % (what, batch.q.dtype, tuple(batch.q.shape), batch.device))
    return q


def is_policy(x, shape, dev, more_games=False):
    """True for a contiguous 16-bit integer tensor of `shape` on `dev` (more_games: the first axis may be longer)."""
    import torch
    got = tuple(x.shape)
    same = len(got) == len(shape) and got[1:] == tuple(shape[1:]) and \
        (got[0] >= shape[0] if more_games else got[0] == shape[0])
    return same and x.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)) and x.device == dev \
        and x.is_contiguous()


def check_policy(batch, x, shape, what, name="policy", more_games=False):
    if not is_policy(x, shape, batch.state.device, more_games):
        raise ThrlError("%s: %s must be a contiguous 16-bit integer tensor %s on %s" % (what, name, shape, batch.device))
    return x


def n_states(batch, call, args):
    """S of the batch's config (include/thrl.h "States") from the library's own plan: `call` with `args` (its n_games
    set) and no tables; no device work."""
    s = ctypes.c_int32(-1)
    args.n_states = ctypes.pointer(s)
    rc = getattr(batch.L, call)(ctypes.byref(batch.cfg), None, ctypes.byref(args), None)
    if s.value < 0:
        _lib.check(rc, call)
    return int(s.value)


# ---------------------------------------------------------------------------------------------- the batch methods
class AnalysisMethods:
    """The analysis methods of GameBatch and MixedGameBatch.  The QTable analyses (deviation(_noise), equilibrium(_noise), crossplay,
    attractors, stationary, track_convergence) read the tables, which both classes lay out alike; a MixedGameBatch with a
    neural agent raises ThrlError there, and its greedy_* / sampled_play methods are the ones for any mix of QTable,
    Reinforce and ActorCritic agents.  Tables, counters, state, epsilon and the episode index are never touched."""

    def _qtable_only(self, method, follow_up):
        kinds = getattr(self, "kinds", None)            # a GameBatch has QTable agents only
        if kinds and any(k != "QTable" for k in kinds):
            raise ThrlError("%s.%s: agents %s: %s" % (type(self).__name__, method, kinds, follow_up))

    def _ready(self):
        if not self.initialized:
            raise ThrlError("%s: call init_tables() or set_tables() first" % type(self).__name__)

    def deviation(self, deviator=0, steps=32, dev_len=1, action="best_response", horizon=None, state0=None,
                  rows=False, group_stats=None, budget=None):
        """Deviation analysis of every game's greedy policies (thrl_deviation; definitions in include/thrl.h):
        the pre-shock cycle (mu, lam, cycle_reward / cycle_action [N, G]), deviator `deviator` playing `action`
        ("best_response" or an action index) for dev_len of `steps` periods, and the response (mu_post, lam_post,
        ret_step, act_dev, gain [G]).  horizon: None = min(prod n_actions + 1, 65536); state0 [G]: the start prices
        (default: the batch's state); the per-game sweep gamma discounts the gain.  Returns a dict of numpy arrays;
        rows=True adds reward_rows / action_rows [steps, N, G]; group_stats (a GroupSpec): the rows are reduced on
        the device in tau-chunks and the raw statistics [steps, n_groups, Q, ...] are returned under "group_stats"."""
        from . import deviation as dv
        self._qtable_only("deviation", dv.NEURAL_FOLLOW_UP)
        self._ready()
        return dv.run(self, deviator=deviator, steps=steps, dev_len=dev_len, action=action, horizon=horizon,
                      state0=state0, rows=rows, group_stats=group_stats, budget=budget or dv.ROW_BUDGET)

    def deviation_noise(self, deviator=0, steps=32, dev_len=1, action="best_response", noise_prob=None, ret_tol=1e-6,
                        weights="stationary", rows=False, group_stats=None, budget=None, q=None, policy=None, n_games=None,
                        tabs=None, tol=1e-12, max_iters=8192):
        """The deviation test UNDER DEMAND NOISE (thrl_deviation_noise; definitions in include/thrl.h): the expected
        impulse response of noisy greedy play to a deviation.  In the environment of stationary() a game follows no
        single path, so the test propagates a distribution over the price cells: from `weights` ("stationary" = each
        game's long-run distribution, stationary(pi=True, start="reset", tol, max_iters) at the same noise and policy;
        or [G, J] values) deviator `deviator` plays `action` ("best_response": its one-period best response in every
        cell, or an action index) for dev_len of `steps` periods, every other period is greedy.  Returns a dict of numpy
        arrays: base_reward, base_action [N, G] (what the start distribution earns; with stationary weights
        stationary()'s stat_reward), dev_share (the share of periods in which the deviation changes anything), gain
        (discounted by the per-game sweep gamma, else the deviator's), gain_dev (its first dev_len periods), low,
        low_step (the deviator's worst period after the deviation), ret_step (the first period from dev_len on whose
        distribution is within ret_tol of the start in total variation, -1: none), dist, mass [G], noise_prob [G],
        stat_iters [G], n_cells.  rows=True adds reward_rows / action_rows [steps, N, G] (the expected rewards and
        actions per period) and dist_rows [steps, G]; group_stats (a GroupSpec) reduces the rows on the device as
        deviation() does.  noise_prob, q, policy, n_games and tabs as in stationary()."""
        from . import deviation as dv
        self._qtable_only("deviation_noise", dv.NEURAL_FOLLOW_UP)
        self._ready()
        return dv.run_noise(self, deviator=deviator, steps=steps, dev_len=dev_len, action=action, noise_prob=noise_prob,
                            ret_tol=ret_tol, weights=weights, rows=rows, group_stats=group_stats,
                            budget=budget or dv.ROW_BUDGET, q=q, policy=policy, n_games=n_games, tabs=tabs, tol=tol,
                            max_iters=max_iters)

    def equilibrium(self, agents=None, state0=None, policies=False, tol=0.0):
        """Equilibrium check of every game's greedy strategies (thrl_equilibrium; definitions in include/thrl.h): for
        each agent in `agents` (default all) the exact best response to the others' greedy strategies, and whether
        its own is one.  Returns a dict of numpy arrays: mu, lam [G] (deviation's, default horizon); iters,
        n_diff_all, n_diff_on, loss_all, loss_on, loss_all_mean, loss_on_mean, v_on [N, G]; the host-side flags
        br_on, br_all [N, G], nash, perfect [G] for the tolerance `tol` (loss <= tol; 0.0 = exact); n_states, agents.
        policies=True adds br_policy (uint16), v_opt, v_pi [N, G, S].  state0 [G]: the start prices (default: the
        batch's state); the per-game sweep gamma is each game's discount factor."""
        from . import equilibrium as eq
        self._qtable_only("equilibrium", eq.NEURAL_FOLLOW_UP)
        self._ready()
        return eq.run(self, agents=agents, state0=state0, policies=policies, tol=tol)

    def equilibrium_noise(self, agents=None, noise_prob=None, eval_tol=1e-12, max_sweeps=8192, policies=False, tol=0.0,
                          q=None, policy=None, weights="stationary", n_games=None, tabs=None):
        """The equilibrium check UNDER DEMAND NOISE (thrl_equilibrium_noise; definitions in include/thrl.h): for each
        agent in `agents` (default all) the exact best response to the others' greedy strategies in the environment of
        stationary(), where every price cell is reachable and a strategy's value solves a linear system on the cells
        (Jacobi sweeps to eval_tol, at most max_sweeps per evaluation; policy iteration with a margin that evaluation
        error cannot cross).  Returns a dict of numpy arrays: iters (-1: not solved or capped), sweeps, n_diff_all,
        loss_all, loss_all_mean [N, G]; with weights loss_w, diff_w, v_w [N, G] (weights: "stationary" = each game's
        long-run distribution over the cells, stationary(pi=True, start="reset") at the same noise and policy -- its last
        iterate also where that iteration stopped at its step limit; None; or [G, J] values); the host-side flags br_all, br_w [N, G] and perfect [G] for the tolerance `tol`; noise_prob [G],
        n_cells, agents.  policies=True adds br_policy (uint16), v_opt, v_pi [N, G, J].  noise_prob, q, policy, n_games
        and tabs as in stationary(); the per-game sweep gamma is each game's discount factor."""
        from . import equilibrium as eq
        self._qtable_only("equilibrium_noise", eq.NEURAL_FOLLOW_UP)
        self._ready()
        return eq.run_noise(self, agents=agents, noise_prob=noise_prob, eval_tol=eval_tol, max_sweeps=max_sweeps,
                            policies=policies, tol=tol, q=q, policy=policy, weights=weights, n_games=n_games, tabs=tabs)

    def crossplay(self, seats, steps=0, horizon=None, state0=None, rows=False, group_stats=None, q=None, policy=None,
                  budget=None):
        """Cross-play of the greedy policies (thrl_crossplay; definitions in include/thrl.h): in match m of a round
        `seats` (int [N, M], or a list of rounds, e.g. crossplay.pairings) seat i is taken by agent i of game
        seats[i][m]; returns mu, lam [M] and cycle_reward / cycle_action [N, M] of the cycle their greedy play ends in
        (a leading round axis for a list), from the start prices state0 [M] (default: the state of seat 0's game).
        Every game's greedy policy is extracted once and all rounds are played from it; policy (a device [G, P]
        16-bit tensor such as a convergence tracker's) is played as it is.  steps K > 0 with rows=True adds the path's
        reward_rows / action_rows [K, N, M]; group_stats (a GroupSpec with G = M) pools the rows of all rounds on the
        device.  Identity seats give deviation's mu, lam, cycle_reward, cycle_action."""
        from . import crossplay as xp
        self._qtable_only("crossplay", xp.NEURAL_FOLLOW_UP)
        self._ready()
        return xp.run(self, seats, steps=steps, horizon=horizon, state0=state0, rows=rows, group_stats=group_stats,
                      q=q, policy=policy, budget=budget or xp.ROW_BUDGET)

    def attractors(self, state0=None, policies=False, q=None, policy=None, reset=True, n_games=None):
        """Attractor analysis of the greedy strategies (thrl_attractors; definitions in include/thrl.h): ALL limit
        cycles of every game's greedy map on the state set and their basins, where deviation follows the one
        path from the training state.  Returns a dict of numpy arrays: n_attr, mu_max, n_cycle_states [G]; the 8
        attractors with the largest basins as rep, lam, basin [8, G] and cycle_reward, cycle_action [8, N, G] (slots
        past n_attr: rep = -1 and zeros); the attractor of the training state, rep_x0, mu_x0, slot_x0 [G] (mu_x0 and
        that slot's lam are deviation's mu and lam); with reset=True (the environment's reset distribution,
        attractors.starts; False skips it, a (rows, w) pair replaces it) reset_mass [8, G], reset_mass_other [G] and
        reset_reward [N, G], the exact expectation of greedy play from a reset; n_states.  policies=True adds state_rep,
        state_mu (uint16) [G, S].  state0 [G]: the training states (default: the batch's state).  The greedy policies
        are extracted once from the tables (or from q); policy (a device [G, P] 16-bit tensor such as a convergence
        tracker's, or crossplay.extract's) is analysed as it is.  n_games: only the first n_games games."""
        from . import attractors as at
        self._qtable_only("attractors", at.NEURAL_FOLLOW_UP)
        self._ready()
        return at.run(self, state0=state0, policies=policies, q=q, policy=policy, reset=reset, n_games=n_games)

    def stationary(self, noise_prob=None, start="reset", state0=None, tol=1e-12, max_iters=8192, pi=False, q=None,
                   policy=None, n_games=None):
        """Greedy play under demand noise (thrl_stationary; definitions in include/thrl.h): the long-run distribution
        of every game's noisy greedy play over the price cells (attractors.starts), by lazy power iteration of its
        Markov chain, and what that distribution earns.  Returns a dict of numpy arrays: iters (steps taken; max_iters
        = the tolerance was not reached, -1 = not solved), change, mass [G], stat_reward, stat_action [N, G], stat_price
        [G], noise_prob [G] (the values analysed), n_cells, max_iters; pi=True adds pi [G, J].  noise_prob: the
        probability of a redrawn intercept per step, a number in (0, 1] or [G] values; None = the batch's per-game sweep
        array if it has one, else the config's value (ThrlError if that is 0); it need not be the one the games were
        trained with.  start: "reset" (the environment's reset distribution) or "state" (the unit mass on the cell of
        state0 [G], default the batch's state).  tol, max_iters: the stopping rule.  The greedy policies are extracted
        once from the tables (or from q); policy (a device [G, P] 16-bit tensor such as a convergence tracker's, or
        crossplay.extract's) is analysed as it is.  n_games: only the first n_games games."""
        from . import stationary as sn
        self._qtable_only("stationary", sn.NEURAL_FOLLOW_UP)
        self._ready()
        return sn.run(self, noise_prob=noise_prob, start=start, state0=state0, tol=tol, max_iters=max_iters, pi=pi, q=q,
                      policy=policy, n_games=n_games)

    def greedy_cycles(self, seats=None, start=None, steps=0, rows=False, horizon=None, tuple_policy=None,
                      group_stats=None, budget=None):
        """The limit cycle of greedy play for ANY mix of QTable, Reinforce and ActorCritic agents (tuple_play.run):
        every agent's strategy as a table over the game's action tuples (thrl_tuple_policy), then a walk on tuple
        indices (thrl_tuple_walk).  seats (default: every game's own agents) re-seat agents across games as
        crossplay does; start (default: the tuple whose price is the state of seat 0's game, -1 when the state is
        no tuple's price: that match gets mu = -1).  A batch with a CAC agent raises ValueError."""
        from . import tuple_play as tp
        self._ready()
        return tp.run(self, seats=seats, start=start, steps=steps, rows=rows, horizon=horizon,
                      tuple_policy=tuple_policy, group_stats=group_stats, budget=budget or tp.ROW_BUDGET)

    def greedy_deviation(self, deviator=0, steps=32, dev_len=1, action="best_response", horizon=None, start=None,
                         rows=False, group_stats=None, tuple_policy=None, budget=None):
        """The deviation test for ANY mix of QTable, Reinforce and ActorCritic agents (tuple_analysis.deviation,
        thrl_tuple_deviation): deviation's outputs on the strategies in tuple form, from the start tuples
        `start` int [G] (default: the tuple whose price is the game's state; -1 = none, the game is refused with
        mu = -1).  tuple_policy: the strategies of tuple_play.extract() (default: extracted here).  The gain is
        discounted by the per-game sweep gamma, else by the deviator's own gamma.  A batch with a CAC agent or more than
        4096 action tuples raises ValueError."""
        from . import tuple_analysis as ta
        self._ready()
        return ta.deviation(self, deviator=deviator, steps=steps, dev_len=dev_len, action=action, horizon=horizon,
                            start=start, rows=rows, group_stats=group_stats, tuple_policy=tuple_policy,
                            budget=budget or ta.dv.ROW_BUDGET)

    def greedy_deviation_noise(self, deviator=0, steps=32, dev_len=1, action="best_response", noise_prob=None,
                               resolution=1024, ret_tol=1e-6, weights="stationary", rows=False, group_stats=None,
                               budget=None, tuple_policy=None, cell_policy=None, n_games=None, tabs=None, tol=1e-12,
                               max_iters=8192):
        """The deviation test UNDER DEMAND NOISE for ANY mix of QTable, Reinforce and ActorCritic agents
        (tuple_analysis.deviation_noise, thrl_tuple_deviation_noise; definitions in include/thrl.h): the expected
        impulse response of noisy greedy play to a deviation.  In the environment of greedy_stationary() a game follows
        no single path of tuples, so the test propagates a distribution over the tuple greedy play intends: from
        `weights` ("stationary" = each game's long-run distribution over the tuple played, greedy_stationary(pi=True,
        start="reset", tol, max_iters) on the same tables and strategies -- its last iterate also where that iteration
        stopped at its step limit; or [G, T] values) deviator `deviator` plays `action` ("best_response": its one-period
        best response to the rivals' actions in every tuple, or an action index) in place of its own for dev_len of
        `steps` periods, every other period is greedy.  Returns a dict of numpy arrays: base_reward, base_action [N, G]
        (what the start distribution earns; with stationary weights greedy_stationary()'s stat_reward, bit for bit),
        dev_share (the share of periods in which the deviation changes anything), gain (discounted by the per-game sweep
        gamma, else the deviator's own gamma), gain_dev (its first dev_len periods), low, low_step (the deviator's worst
        period after the deviation), ret_step (the first period from dev_len on whose distribution is within ret_tol of
        the start in total variation, -1: none), dist, mass [G], noise_prob [G], stat_iters, n_switch, unresolved [G]
        (the sampling diagnostics of greedy_stationary()), T, n_cells.  rows=True adds reward_rows / action_rows
        [steps, N, G] (the expected rewards and actions per period) and dist_rows [steps, G]; group_stats (a GroupSpec)
        reduces the rows on the device as greedy_deviation() does.  noise_prob, resolution, tuple_policy, cell_policy,
        n_games and tabs as in greedy_stationary().  A batch with a CAC agent or more than 4096 action tuples or cells
        raises ValueError; a working set above a CU's LDS is THRL_ERR_UNSUPPORTED."""
        from . import tuple_analysis as ta
        self._ready()
        return ta.deviation_noise(self, deviator=deviator, steps=steps, dev_len=dev_len, action=action,
                                  noise_prob=noise_prob, resolution=resolution, ret_tol=ret_tol, weights=weights, rows=rows,
                                  group_stats=group_stats, budget=budget or ta.dv.ROW_BUDGET, tuple_policy=tuple_policy,
                                  cell_policy=cell_policy, n_games=n_games, tabs=tabs, tol=tol, max_iters=max_iters)

    def greedy_equilibrium(self, agents=None, start=None, policies=False, tol=0.0, tuple_policy=None):
        """The equilibrium check for ANY mix of QTable, Reinforce and ActorCritic agents (tuple_analysis.equilibrium,
        thrl_tuple_equilibrium): equilibrium's outputs with the game's T action tuples as the state set
        (n_states = T; policies=True adds br_policy, v_opt, v_pi [N, G, T]).  start and tuple_policy as in
        greedy_deviation; a game without a start tuple has mu = -1 and NaN on-path outputs.  A batch with a CAC agent
        or more than 4096 action tuples raises ValueError."""
        from . import tuple_analysis as ta
        self._ready()
        return ta.equilibrium(self, agents=agents, start=start, policies=policies, tol=tol, tuple_policy=tuple_policy)

    def greedy_equilibrium_noise(self, agents=None, noise_prob=None, resolution=1024, eval_tol=1e-12, max_sweeps=8192,
                                 policies=False, tol=0.0, tuple_policy=None, cell_policy=None, weights="stationary",
                                 n_games=None, tabs=None):
        """The equilibrium check UNDER DEMAND NOISE for ANY mix of QTable, Reinforce and ActorCritic agents
        (tuple_analysis.equilibrium_noise, thrl_tuple_equilibrium_noise; definitions in include/thrl.h): for each agent
        in `agents` (default all) the exact best response to the others' strategies in the environment of
        greedy_stationary(), on the S = T + J states "the price is exactly tuple t's" (the strategies of
        tuple_play.extract()) and "the price lies in cell k" (the strategies sampled at the midpoints of `resolution`
        uniform cells beside the QTable agents' breakpoints): Jacobi sweeps to eval_tol, at most max_sweeps per
        evaluation, policy iteration with a margin that evaluation error cannot cross.  Returns a dict of numpy arrays:
        iters (-1: not solved or capped), sweeps, n_diff_tuples, n_diff_cells, loss_all, loss_tuples_mean,
        loss_cells_mean [N, G]; with weights loss_w, diff_w, v_w [N, G] and pi [G, T] (weights: "stationary" = each
        game's long-run distribution over the tuple played, greedy_stationary(pi=True, start="reset") on the same tables
        and strategies -- its last iterate also where that iteration stopped at its step limit; None; or [G, T] values),
        from which the kernel derives where decisions are made in the long run; the host-side flags br_all, br_w [N, G]
        and perfect [G] for the tolerance `tol`; noise_prob [G], n_cells, T, n_states, agents.  policies=True adds
        br_policy (uint16), v_opt, v_pi [N, G, T + J], tuple-states first.  noise_prob, tuple_policy, cell_policy, n_games
        and tabs as in greedy_stationary(); the per-game sweep gamma is each game's discount factor, else the agent's
        own gamma.  A batch with a CAC agent or more than 4096 action tuples or cells raises ValueError; a working set
        above a CU's LDS is THRL_ERR_UNSUPPORTED."""
        from . import tuple_analysis as ta
        self._ready()
        return ta.equilibrium_noise(self, agents=agents, noise_prob=noise_prob, resolution=resolution, eval_tol=eval_tol,
                                    max_sweeps=max_sweeps, policies=policies, tol=tol, tuple_policy=tuple_policy,
                                    cell_policy=cell_policy, weights=weights, n_games=n_games, tabs=tabs)

    def greedy_attractors(self, start=None, weights="uniform", policies=False, tuple_policy=None):
        """The attractor analysis for ANY mix of QTable, Reinforce and ActorCritic agents (tuple_analysis.attractors,
        thrl_tuple_attractors): attractors' outputs with the game's T action tuples as the state set
        (n_states = T; policies=True adds tuple_rep, tuple_mu [G, T]) and start_mass, start_mass_other, start_reward in
        place of the reset_* fields: weights is a weight per start tuple, "uniform" = 1 / T (a start drawn uniformly over
        action profiles, not the environment's reset distribution), None = none, or T numbers.  start and tuple_policy
        as in greedy_deviation; a game without a start tuple has rep_x0 = mu_x0 = slot_x0 = -1.  A batch with a CAC
        agent or more than 4096 action tuples raises ValueError."""
        from . import tuple_analysis as ta
        self._ready()
        return ta.attractors(self, start=start, weights=weights, policies=policies, tuple_policy=tuple_policy)

    def greedy_stationary(self, noise_prob=None, start="reset", resolution=1024, tol=1e-12, max_iters=8192, pi=False,
                          tuple_policy=None, cell_policy=None, n_games=None, tabs=None):
        """Greedy play under demand noise for ANY mix of QTable, Reinforce and ActorCritic agents (tuple_stationary.run,
        thrl_price_policy + thrl_tuple_stationary): the long-run distribution over the tuple played and what it earns --
        stationary's outputs with pi [G, T] over the action tuples, plus n_switch and unresolved [G]: a network's
        strategy is sampled at the midpoints of `resolution` uniform cells of the price axis (beside the QTable agents'
        breakpoints), and unresolved is the share of the axis on which that sampling may be wrong.  start: "reset", "state"
        (the tuple played at the state the batch holds) or int [G] start tuples.  A batch with a CAC agent or more than
        4096 action tuples or cells raises ValueError."""
        from . import tuple_stationary as ts
        self._ready()
        return ts.run(self, noise_prob=noise_prob, start=start, resolution=resolution, tol=tol, max_iters=max_iters, pi=pi,
                      tuple_policy=tuple_policy, cell_policy=cell_policy, n_games=n_games, tabs=tabs)

    def sampled_play(self, epsilon="current", start="uniform", tol=1e-12, max_iters=8192, pi=False, n_games=None,
                     tuple_policy=None, probs=None, dpolicy=None, tabs=None, noise_prob=0.0, resolution=1024, nprobs=None,
                     npolicy=None):
        """The exact long-run profit of SAMPLED play (sampled_play.run, thrl_price_probs + thrl_sampled_chain): every
        agent plays the way it was trained -- a Reinforce / ActorCritic agent samples its softmax, a QTable agent is
        epsilon-greedy (epsilon: "current" = the batch's epsilon now, a number, one per agent, or an array [N, G]) --
        with no demand noise, so the tuple played is a Markov chain on the game's T action tuples: iters, change, mass,
        samp_price, agree [G] (the share of steps on which every agent plays its greedy action), samp_reward,
        samp_action [N, G], with pi the distribution [G, T].  start: "uniform", "state" or int [G] start tuples.  A batch
        with a CAC agent or more than 4096 action tuples raises ValueError; a working set above a CU's LDS is
        THRL_ERR_UNSUPPORTED.  Under demand noise (noise_prob: a number in (0, 1], an array [G], or None = the batch's
        own; the number 0.0, the default, is the noise-free call; thrl_sampled_noise_chain) the price is redrawn with that probability and the networks are taken at the
        nodes of `resolution` uniform cells of the price axis (nprobs, npolicy: the strategies there); there start "reset" is
        the environment's reset distribution; the result also holds noise_prob and max_jump [G]."""
        from . import sampled_play as sp
        self._ready()
        return sp.run(self, epsilon=epsilon, start=start, tol=tol, max_iters=max_iters, pi=pi, n_games=n_games,
                      tuple_policy=tuple_policy, probs=probs, dpolicy=dpolicy, tabs=tabs, noise_prob=noise_prob,
                      resolution=resolution, nprobs=nprobs, npolicy=npolicy)

    def sampled_response(self, agents=None, epsilon="current", gamma=None, eval_tol=1e-12, max_sweeps=8192, policies=False,
                         pi=None, n_games=None, probs=None, dpolicy=None, tabs=None):
        """Exact best responses to the rivals' STOCHASTIC policies (sampled_response.run, thrl_sampled_response;
        definitions in include/thrl_response.h): for each agent in `agents` (default all) the value V_pi of its own
        mixed policy against rivals that sample -- a network its softmax, a QTable agent epsilon-greedily -- and its best
        deterministic reply V*, sigma*, on the D distinct prices (Jacobi sweeps to eval_tol, at most max_sweeps per
        evaluation; policy iteration from the modal action).  Returns a dict of numpy arrays: iters (-1: not solved or
        capped), sweeps, n_diff, loss_all, loss_mean [N, G]; weighted by pi (None = the long-run distribution of
        sampled_play(pi=True), an array [G, T], or False = none) loss_w, gain_w, v_w, br_prob_w [N, G]; gamma, epsilon
        [N, G]; policies=True adds br_policy (uint16), v_opt, v_pi [N, G, D].  gamma: None = each agent's own (the
        per-game sweep where there is one), a number, N numbers or [N, G].  Noise-free play only."""
        from . import sampled_response as sr
        self._ready()
        return sr.run(self, agents=agents, epsilon=epsilon, gamma=gamma, eval_tol=eval_tol, max_sweeps=max_sweeps,
                      policies=policies, pi=pi, n_games=n_games, probs=probs, dpolicy=dpolicy, tabs=tabs)

    def sampled_response_noise(self, agents=None, epsilon="current", gamma=None, eval_tol=1e-12, max_sweeps=8192,
                               policies=False, pi=None, n_games=None, probs=None, dpolicy=None, tabs=None, noise_prob=None,
                               resolution=1024, nprobs=None, npolicy=None, ntabs=None):
        """sampled_response under DEMAND NOISE (sampled_response.run_noise, thrl_sampled_response_noise; definitions in
        include/thrl_response_noise.h): the same values and best replies on the D distinct prices and then the Jn nodes of
        the redrawn price (sampled_play.noise_tables(config, resolution)).  noise_prob: a number in (0, 1], an array [G]
        or None = the batch's own.  Returns sampled_response's arrays with n_diff_prices / n_diff_nodes and
        loss_prices_mean / loss_nodes_mean in place of n_diff / loss_mean, the weights being the long-run distribution of
        the state in which a decision is made (pi: None = sampled_play(noise_prob=..., pi=True)), and noise_prob [G];
        policies=True adds br_policy, v_opt, v_pi [N, G, D + Jn], the prices first."""
        from . import sampled_response as sr
        self._ready()
        return sr.run_noise(self, agents=agents, epsilon=epsilon, gamma=gamma, eval_tol=eval_tol, max_sweeps=max_sweeps,
                            policies=policies, pi=pi, n_games=n_games, probs=probs, dpolicy=dpolicy, tabs=tabs,
                            noise_prob=noise_prob, resolution=resolution, nprobs=nprobs, npolicy=npolicy, ntabs=ntabs)

    def sampled_deviation(self, deviator=0, steps=32, dev_len=1, action="best_response", epsilon="current", gamma=None,
                          ret_tol=1e-6, weights="stationary", rows=False, group_stats=None, budget=None, n_games=None,
                          probs=None, dpolicy=None, tabs=None, tol=1e-12, max_iters=8192):
        """The deviation test of SAMPLED play (sampled_deviation.run, thrl_sampled_deviation; definitions in
        include/thrl_sampled_deviation.h): the expected impulse response of the agents' stochastic policies -- a network
        its softmax, a QTable agent epsilon-greedily -- when `deviator` plays a deterministic strategy of the price for
        dev_len periods and its own policy again for the remaining steps - dev_len.  action: "best_response" (one period,
        to the rivals' mixed policies), an action index, "best_reply" (sampled_response's br_policy, the patient best
        reply) or a [G, D] array.  No episodes are sampled: a distribution over the tuple played is propagated from
        weights ("stationary" = the long-run distribution of sampled_play(pi=True, tol, max_iters), or an array [G, T]).
        Returns a dict of numpy arrays: base_reward, base_action [N, G]; base_price, dev_share (the share of periods the
        deviation changes), gain and gain_dev (the discounted gain of all steps and of the deviation itself; gamma: None
        = the deviator's own), low and low_step (the deepest punishment), ret_step (the first period at which the
        distribution is back within ret_tol in total variation, else -1), dist, mass, gamma, stat_iters [G]; epsilon
        [N, G]; solved [G].  rows=True adds reward_rows / action_rows [steps, N, G] and price_rows / dist_rows [steps, G];
        group_stats (a GroupSpec): the rows are reduced on the device.  Noise-free play; under demand noise:
        sampled_deviation_noise."""
        from . import sampled_deviation as sd
        self._ready()
        return sd.run(self, deviator=deviator, steps=steps, dev_len=dev_len, action=action, epsilon=epsilon, gamma=gamma,
                      ret_tol=ret_tol, weights=weights, rows=rows, group_stats=group_stats, budget=budget, n_games=n_games,
                      probs=probs, dpolicy=dpolicy, tabs=tabs, tol=tol, max_iters=max_iters)

    def sampled_deviation_noise(self, deviator=0, steps=32, dev_len=1, action="best_response", epsilon="current", gamma=None,
                                ret_tol=1e-6, weights="stationary", rows=False, group_stats=None, budget=None, n_games=None,
                                probs=None, dpolicy=None, tabs=None, tol=1e-12, max_iters=8192, noise_prob=None, resolution=1024,
                                nprobs=None, npolicy=None):
        """sampled_deviation under DEMAND NOISE (sampled_deviation.run_noise, thrl_sampled_deviation_noise; definitions in
        include/thrl_sampled_deviation_noise.h): the same impulse response in the chain of sampled_play(noise_prob=...),
        every period's reward and price in expectation over the redrawn demand.  The deviator's strategy lives on the D
        distinct prices and then the Jn nodes of the redrawn price (sampled_play.noise_tables(config, resolution)): action
        "best_response" is the one-period best response at each of them, "best_reply" sampled_response_noise's
        br_policy, an array is [G, D + Jn].  noise_prob: a number in [0, 1], an array [G] or None = the batch's own;
        weights "stationary" = the long-run distribution under the same noise.  Returns sampled_deviation's dict plus
        noise_prob, max_jump [G], n_nodes, lds_bytes, and dev_policy [G, D + Jn] when a strategy was given or computed."""
        from . import sampled_deviation as sd
        self._ready()
        return sd.run_noise(self, deviator=deviator, steps=steps, dev_len=dev_len, action=action, epsilon=epsilon, gamma=gamma,
                            ret_tol=ret_tol, weights=weights, rows=rows, group_stats=group_stats, budget=budget,
                            n_games=n_games, probs=probs, dpolicy=dpolicy, tabs=tabs, tol=tol, max_iters=max_iters,
                            noise_prob=noise_prob, resolution=resolution, nprobs=nprobs, npolicy=npolicy)

    def track_convergence(self, window, every=1, snapshot=False):
        """A convergence.Tracker of every game's greedy policies (thrl_policy_track; definitions in include/thrl.h),
        its baseline taken now at self.episode; tracker.check() after a launch that ends at a check episode.
        snapshot=True keeps each game's tables and state at its convergence (one more copy of q on the device).
        Only reads the tables."""
        from . import convergence as cv
        self._qtable_only("track_convergence", cv.NEURAL_FOLLOW_UP)
        return cv.Tracker(self, window, every, snapshot)
