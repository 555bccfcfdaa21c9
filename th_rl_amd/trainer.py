"""create_game / train_one -- the reference's trainer entry points (th_rl/trainer.py)
with the same signatures, config schema and output files, driving the GPU.

train_one runs the whole episode loop on the device through GameBatch (fused HIP
kernels).  The JSON schema is the reference's; the optional extra keys in the
"training" block select the batched mode and default to reference behaviour:

    "training": {"epochs": .., "print_freq": ..,
                 "n_games": 1,        # games trained in lockstep (independent replicas)
                 "seed": null,        # Philox seed (null: fresh OS entropy; numpy's global stream is left exactly
                                      # as the reference's train_one leaves it)
                 "philox_init": false, # true: tables / initial state from Philox keyed by (seed, global game id)
                                      # even for ONE game (what a 1-game shard of a sharded run needs)
                 "dtype": null,       # "float64" | "float32" (default f64 for 1 game, f32 otherwise)
                 "device": "cuda:0", "game_offset": 0, "kernel": "auto",
                 "resume": null,     # path of a batch.pt written by an earlier run: continue it
                 "game_logs": null,  # true (every game) or a list of global game ids: per-game learning curves
                                     # game_rewards.npy / game_actions.npy, float64 [epochs, N, kept games], and
                                     # game_ids.npy (int64 global ids); read one game with utils.game_log
                 "group_stats": null, # true or {"bins": 256, "quantiles": [0.25, 0.5, 0.75], "histograms": false,
                                     # "greedy_iters": 0, "ranges": {"total": [lo, hi], ...}}: per-group learning-curve
                                     # statistics reduced on the device (group_stats.py): groups.json and float64
                                     # group_mean / group_std / group_min / group_max.npy [epochs, n_groups, Q],
                                     # group_quantiles.npy [epochs, n_groups, Q, n_q], group_sums.npy int64 [.., Q, 2],
                                     # with histograms group_hist.npy uint32 [.., Q, bins + 2]; greedy_iters k > 0 adds
                                     # the same greedy_*.npy of play_greedy's rows ([k, ...]).  Q = 2N + 1 quantities:
                                     # reward_i, action_i, total.  Quantiles are of the per-epoch values; the reference
                                     # smooths each run with ewm(halflife=1000) first, which is off by default:
                                     # "smooth": 1000 (a halflife, or {"halflife": 1000}) smooths every game's curve on
                                     # the device (thrl_ewm_rows, pandas' ewm(halflife=h).mean(); one state for the whole
                                     # run) and adds the same files for the smoothed curves, group_smooth_*.npy, and
                                     # with game_logs game_rewards_smooth.npy / game_actions_smooth.npy; groups.json
                                     # gains "smooth": {"halflife", "decay"}.  Not with "resume": the smoothing state
                                     # is not checkpointed.
                 "equilibrium": null,  # true or {"agents": [all], "tol": 0.0, "policies": false, "tables": "final"}: after
                                       # training (and the deviation analysis) the equilibrium check of the greedy
                                       # strategies (equilibrium.py, QTable agents only): equilibrium.json, eq_*.npy;
                                       # "noise": true or {"noise_prob": null, "eval_tol": 1e-12, "max_sweeps": 8192}
                                       # adds the check UNDER DEMAND NOISE (noise_prob null = the run's own), weighted
                                       # by the long-run distribution of noisy greedy play: equilibrium_noise.json,
                                       # eqn_*.npy
                 "crossplay": null,  # true or {"rounds": 8, "scheme": "rotate" | "random", "against": "own" | "all",
                                     # "steps": 0, "horizon": null, "seed": 0, "tables": "final" | "converged"}: after
                                     # training (and the equilibrium check) greedy play between agents of DIFFERENT
                                     # games (crossplay.py, QTable agents only): crossplay.json (options, Nash, Cartel,
                                     # per-(group, partner group) summary), xplay_seats.npy int32 [rounds, N, G] (global
                                     # game ids), xplay_cycle.npy int32 [rounds, 2, G] (mu, lam), xplay_cycle_reward /
                                     # xplay_cycle_action.npy [rounds, N, G], xplay_self_cycle.npy [2, G] and
                                     # xplay_self_reward.npy [N, G] (each game's own cycle); with group_stats and
                                     # steps > 0 the path rows pooled over the rounds, xplay_*.npy [steps, ...]
                 "attractors": null,  # true or {"policies": false, "tables": "final" | "converged"}: after training (and
                                      # cross-play) ALL limit cycles of the greedy strategies and their basins
                                      # (attractors.py, QTable agents only): attractors.json (options, Nash, Cartel,
                                      # per-group summary), attr_games.npy int32 [6, G], attr_slots.npy int32 [3, 8, G],
                                      # attr_cycle.npy [2, 8, N, G], attr_reset_mass.npy [9, G], attr_reset_reward.npy
                                      # [N, G]; with policies attr_state.npy uint16 [2, G, S]
                 "stationary": null,  # true or {"noise_prob": null, "start": "reset", "tol": 1e-12, "max_iters": 8192,
                                      # "pi": false, "tables": "final" | "converged"}: after training (and the attractor
                                      # analysis) the long-run distribution of greedy play UNDER DEMAND NOISE and what
                                      # it earns (stationary.py, QTable agents only; noise_prob null = the run's own):
                                      # stationary.json (options, Nash, Cartel, per-group summary), stat_iters.npy int32
                                      # [G], stat_games.npy [4, G], stat_reward.npy / stat_action.npy [N, G]; with pi
                                      # stat_pi.npy [G, J]
                 "greedy_stationary": null,  # true or {"noise_prob": null, "start": "reset" | "state", "tol": 1e-12,
                                      # "max_iters": 8192, "pi": false, "resolution": 1024}: "stationary" for any mix of
                                      # QTable, Reinforce and ActorCritic agents (tuple_stationary.py): the chain of noisy
                                      # greedy play on the game's action tuples, a network's strategy sampled on
                                      # `resolution` uniform cells of the price axis: greedy_stationary.json,
                                      # gstat_iters.npy int32 [2, G] (iters, n_switch), gstat_games.npy [5, G],
                                      # gstat_reward.npy / gstat_action.npy [N, G]; with pi gstat_pi.npy [G, T]
                 "sampled_play": null,  # true or {"epsilon": "current", "start": "uniform" | "state", "tol": 1e-12,
                                      # "max_iters": 8192, "pi": false}: after training the exact long-run profit of
                                      # SAMPLED play, the way the agents were trained (sampled_play.py: a network samples
                                      # its softmax, a QTable agent is epsilon-greedy; with the further key "noise": true or
                                      # {"noise_prob": null (the run's own) | p, "resolution": 1024} under demand noise, where
                                      # "start" may be "reset": also splay_noise_prob.npy / splay_max_jump.npy [G]), for any mix of
                                      # QTable, Reinforce and ActorCritic agents: sampled_play.json, splay_iters.npy int32
                                      # [G], splay_games.npy [4, G] (change, mass, price, agree), splay_reward.npy /
                                      # splay_action.npy / splay_epsilon.npy [N, G]; with pi splay_pi.npy [G, T]
                                      # (its sub-keys "response" and "deviation": sampled_response.py, sampled_deviation.py)
                 "deviation": null,  # true or {"agents": [all], "steps": 32, "dev_len": 1, "action": "best_response",
                                     # "horizon": null}: after training (and the greedy statistics) the deviation
                                     # analysis of the greedy policies (deviation.py, QTable agents only): deviation.json
                                     # (options, Nash, Cartel, per-(group, deviator) summary), dev_cycle.npy int32 [2, G]
                                     # (mu, lam), dev_cycle_reward / dev_cycle_action.npy [N, G], per deviator d
                                     # dev<d>_post.npy int32 [4, G] (mu_post, lam_post, ret_step, act_dev) and
                                     # dev<d>_gain.npy [G]; with group_stats the response rows' dev<d>_*.npy [steps, ...];
                                     # "noise": true or {"noise_prob": null, "ret_tol": 1e-6, "tol": 1e-12, "max_iters":
                                     # 8192} adds the test UNDER DEMAND NOISE (noise_prob null = the run's own): the
                                     # expected response of noisy greedy play from its long-run distribution,
                                     # deviation_noise.json, devn_prob / devn_stat_iters.npy [G], per deviator
                                     # devn<d>_games.npy [6, G], devn<d>_steps.npy int32 [2, G], devn<d>_base.npy
                                     # [2, N, G] and with group_stats devn<d>_*.npy [steps, ...];
                                     # "tables": "final" (default) | "converged" (needs convergence.snapshot): analyse
                                     # each game's tables and state at its convergence (never converged: final tables)
                 "convergence": null, # true or {"window": ceil(100000 / max_steps), "every": 20, "stop": null,
                                     # "snapshot": false}: track every game's greedy policy (convergence.py, QTable
                                     # agents only) at the global episodes that are multiples of `every` (on GameBatch
                                     # rounded up to a multiple of thrl_training_cycle; launches are cut there); a game
                                     # has converged at the first check where its policy has not changed for `window`
                                     # episodes.  stop: a fraction in (0, 1] ends training at the first check where that
                                     # fraction of the run's games (all shards) has converged, epochs the cap; log.csv
                                     # and the per-epoch .npy then have episodes_run rows.  snapshot: keep each game's
                                     # tables and state at convergence on the device (stride * 4 B per game in float32,
                                     # * 8 B in float64, + 8 B).  Writes convergence.json (options, every_used,
                                     # episodes_run, stopped_early, per-group summary), conv_episode.npy /
                                     # conv_since.npy / conv_stable_since.npy int64 [G] (-1 = never), conv_changes.npy
                                     # int32 [G] and convergence.pt (the tracker; resume picks it up beside batch.pt)
                 "groups": null,     # group id of every game (default: one group per distinct sweep combination, in
                                     # order of first appearance; one group without a sweep)
                 "sweep": null}      # per-game hyper-parameters, e.g. {"gamma": [0.35, 0.95, ...]}: arrays of
                                     # length n_games (or [agent][game]) for gamma / alpha / eps / eps_end /
                                     # eps_step / noise_prob (+ entropy for neural agents) -- a config sweep
                                     # (main.py:13-21: one process per config and run) as ONE batched run,
                                     # for all-QTable games and for games with neural agents alike

n_games == 1: tables come from the constructed agents (numpy's global RNG, exactly where
the reference draws them) and the run is float64.  n_games > 1: every game's tables and
initial state come from Philox keyed by (seed, global game id).  Output files are the
reference's four artefacts for game 0 (`<i>.npy`, `<i>_counter.npy`, `config.json`,
`log.csv` -- the log is the MEAN over games), plus `batch.pt` with all games when
n_games > 1, with "game_logs" the kept games' own curves (game_rewards.npy, game_actions.npy,
game_ids.npy), and with "group_stats" the per-group statistics (groups.json, group_*.npy; utils.group_log and
utils.group_quantiles read them; with its "smooth" also those of the smoothed curves, group_smooth_*.npy).  There is no CPU fallback: without the HIP library or a GPU this raises.
"""
import json
import os
import time

from numpy.lib.format import open_memmap

import numpy
import pandas

from th_rl_amd.environments import *  # noqa: F401,F403  (class names are eval'd, as in the reference)
from th_rl_amd.agents import *        # noqa: F401,F403
from th_rl_amd import _lib, analysis
from th_rl_amd.batched import GameBatch


def create_game(configpath):
    """JSON -> (config, agents, environment), constructed by name like the reference."""
    config = json.load(open(configpath))
    agents = [eval(agent["name"])(**agent) for agent in config["agents"]]
    assert (
        len(agents) == config["environment"]["nplayers"]
    ), "Bad config. Check number of agents."
    environment = eval(config["environment"]["name"])(**config["environment"])
    return config, agents, environment


def _progress_line(print_eps, eps, elapsed, e, rew, act, names):
    head = ""
    if print_eps:
        head = "eps:{} | ".format(numpy.round(numpy.array(eps) * 1000) / 1000)
    return head + "time:{:2.2f} | episode:{:3d} | reward:{} | agents:{} | actions:{}".format(
        elapsed, e, numpy.round(100 * rew) / 100, ",".join(names), numpy.round(100 * act) / 100)


def resume_is_gamebatch(path):
    """True when `path` is a checkpoint written by GameBatch (so the continued run must use it too)."""
    if not path:
        return False
    import torch
    return torch.load(path, weights_only=True).get("kind") != "mixed"


def _eps_of_game0(batch):
    """Epsilon per agent as game 0 has it: with a per-game epsilon sweep the schedule lives on the device
    (batch.sweep['eps'][agent, game], decayed in the kernels); batch.eps is then only the config's scalar schedule,
    which game 0 never had.  The saved artefacts and the progress line are game 0's (trainer.py:79,101-110)."""
    eps = list(batch.eps)
    sw = getattr(batch, "sweep", None) or {}
    if "eps" in sw:
        col = sw["eps"][:, 0].cpu().numpy()
        for i in range(min(len(eps), len(col))):
            eps[i] = float(col[i])
    return eps


GAME_LOG_BUDGET = 256 << 20        # bytes per per-game device log buffer and chunk (as mixed.py's mean-log path)


def game_log_chunk(n_agents, n_games, cycle=1, budget=GAME_LOG_BUDGET):
    """Episodes per launch when per-game logs are kept: [k, N, G] float64 stays within `budget` bytes, rounded down to
    whole training cycles of the wave kernel (thrl_training_cycle; at least one cycle)."""
    k = max(1, budget // (8 * int(n_agents) * int(n_games)))
    c = max(1, int(cycle))
    return max(c, k // c * c)


def _npy_out(path, shape, dtype=numpy.float64):
    """.npy of `shape` filled in place (memory-mapped; an empty array is written as it is)."""
    if all(shape):
        return open_memmap(path, mode="w+", dtype=dtype, shape=shape)
    numpy.save(path, numpy.zeros(shape, dtype))
    return numpy.zeros(shape, dtype)


GROUP_FIELDS = ("mean", "std", "min", "max", "quantiles", "sums", "hist")


def group_stats_files(exp_path, prefix, rows, spec, histograms):
    """The memory-mapped group_*.npy (or greedy_*.npy) of a run: dict field -> array [rows, n_groups, Q, ...]."""
    cell = (int(rows), spec.n_groups, spec.Q)
    shapes = {"mean": cell, "std": cell, "min": cell, "max": cell, "quantiles": cell + (len(spec.quantiles),),
              "sums": cell + (2,), "hist": cell + (spec.bins + 2,)}
    dt = {"sums": numpy.int64, "hist": numpy.uint32}
    return {f: _npy_out(os.path.join(exp_path, "%s_%s.npy" % (prefix, f)), shapes[f], dt.get(f, numpy.float64))
            for f in GROUP_FIELDS if f != "hist" or histograms}


def write_group_stats(files, at, raw, describe):
    """Rows at .. at + len of the files from one chunk's raw outputs (group_stats.to_numpy / merge)."""
    from th_rl_amd.group_stats import finalize
    fin = finalize(raw, describe)
    k = raw["sums"].shape[0]
    for f, arr in files.items():
        arr[at:at + k] = raw[f] if f in ("sums", "hist") else fin[f]


def save_group_stats(exp_path, prefix, raw, spec, histograms):
    """The whole <prefix>_*.npy of one raw output: an analysis's response rows, or a sharded run's merged statistics."""
    files = group_stats_files(exp_path, prefix, raw["sums"].shape[0], spec, histograms)
    write_group_stats(files, 0, raw, spec.describe())
    for arr in files.values():
        if hasattr(arr, "flush"):
            arr.flush()


def group_spec_of(config, training, n_games):
    """training.group_stats -> (GroupSpec of this run's games, options) or (None, None)."""
    opt = training.get("group_stats", None)
    if opt is None or opt is False:
        return None, None
    from th_rl_amd.group_stats import GroupSpec, parse_options
    opt = parse_options(opt)
    spec = GroupSpec.from_config(config, n_games, opt, sweep=training.get("sweep", None),
                                 groups=training.get("groups", None), n_groups=training.get("n_groups", None))
    return spec, opt


def game_log_ids(spec, n_games, game_offset):
    """training.game_logs -> (global ids int64, local indices int64) of the games kept by this run: true = all,
    a list = those global ids (each must be one of this run's games, game_offset .. game_offset + n_games - 1)."""
    if spec is True:
        local = numpy.arange(n_games, dtype=numpy.int64)
    else:
        ids = numpy.asarray(list(spec), dtype=numpy.int64).reshape(-1)
        local = ids - int(game_offset)
        bad = ids[(local < 0) | (local >= n_games)]
        if bad.size:
            raise ValueError("training.game_logs: game ids %s are not in this run (global ids %d..%d)"
                             % (bad.tolist()[:8], game_offset, game_offset + n_games - 1))
    return local + int(game_offset), local


def _run_totals(converged, n_games):
    """(converged games, games) of the whole run: summed over the ranks of th_rl_amd.launch (its gloo group), so that
    every rank stops at the same check."""
    try:
        import torch.distributed as dist
        active = dist.is_available() and dist.is_initialized()
    except ImportError:
        active = False
    if not active:
        return int(converged), int(n_games)
    import torch
    t = torch.tensor([int(converged), int(n_games)], dtype=torch.int64)
    dist.all_reduce(t)
    return int(t[0]), int(t[1])


def train_one(exp_path, configpath, loadonly=False, print_eps=False):
    if not os.path.exists(exp_path):
        os.mkdir(os.path.join(exp_path))

    config, agents, environment = create_game(configpath)
    if not all(isinstance(a, (QTable, Reinforce, CAC)) for a in agents) or not isinstance(environment, NoisyPriceState):
        raise NotImplementedError(                      # (ActorCritic is a Reinforce subclass here)
            "train_one: the device path trains QTable, Reinforce, ActorCritic and CAC agents on NoisyPriceState")
    all_tabular = all(isinstance(a, QTable) for a in agents)

    training = config.get("training", {})
    opts = {}       # key -> parsed options of every analysis asked for (analysis.REGISTRY), refused before training
    for a in analysis.REGISTRY:
        if analysis.enabled(training, a.key):
            opts[a.key] = getattr(analysis.module_of(a), a.parse)(training[a.key], config)
    conv_opt = opts.get("convergence")
    for a in analysis.REGISTRY:
        if a.converged and opts.get(a.key, {}).get("tables") == "converged" and not (conv_opt and conv_opt["snapshot"]):
            raise ValueError('training.%s.tables = "converged" needs training.convergence with "snapshot": true' % a.key)
    epochs = training.get("epochs", 0)
    print_freq = training.get("print_freq", 500)
    n_games = int(training.get("n_games", 1))
    seed = training.get("seed", None)
    if seed is None:
        # independent of numpy's global stream: under numpy.random.seed(s) the constructors above and
        # environment.reset() below then draw exactly the values the reference's train_one draws
        seed = int(numpy.random.SeedSequence().entropy % (2 ** 31 - 1))
    dtype = training.get("dtype", None) or ("float64" if n_games == 1 else "float32")
    names = [a["name"] for a in config["agents"]]

    resume = training.get("resume", None)
    if resume and training.get("group_stats", None) not in (None, False):
        from th_rl_amd.group_stats import parse_options
        if parse_options(training["group_stats"]).get("smooth") is not None:
            raise ValueError("training.group_stats.smooth with training.resume: the smoothing state is not checkpointed, "
                             "so a continued run cannot carry the curve on")
    # Small all-QTable batches in float64 (the default for ONE game = the reference's own use), and those
    # the LDS-resident wave kernel cannot take (other than 2 agents, per-agent grids, T < min_memory), run one
    # wavefront per game through the mixed-agent episode kernel: it keeps train_one's per-step log arithmetic
    # (rewards_log += reward / max_steps, trainer.py:65), so a single game's log.csv is the reference's to the
    # last bit, and it is 4.7x (1 game) to 1.3x (16,384 games) faster than the one-thread-per-game generic
    # kernel, same bits.  Larger float64 batches use the wave kernel's float64 variant (tables, counters,
    # epsilon, state identical; logs to 1e-12).  Explicit "kernel" / "sweep" keys keep GameBatch.
    small_tabular = False
    if all_tabular and "kernel" not in training and not training.get("sweep") and n_games <= 16384 and not resume_is_gamebatch(resume):
        import ctypes
        cfg_probe, _ = _lib.cfg_from_config(config, n_games, {"float32": 0, "float64": 1}[str(dtype)])
        small_tabular = (str(dtype) == "float64"
                         or _lib.load().thrl_select_kernel(ctypes.byref(cfg_probe), 0) == _lib.KERNEL_GENERIC)
    if all_tabular and not small_tabular:
        batch = GameBatch(config, n_games=n_games, device=training.get("device", "cuda:0"), dtype=dtype,
                          seed=seed, game_offset=int(training.get("game_offset", 0)),
                          kernel=training.get("kernel", "auto"), sweep=training.get("sweep", None))
    else:
        # games with neural agents: fused episode kernel + batched network updates (mixed.py)
        from th_rl_amd.mixed import MixedGameBatch
        batch = MixedGameBatch(config, n_games=n_games, device=training.get("device", "cuda:0"), dtype=dtype,
                               seed=seed, game_offset=int(training.get("game_offset", 0)),
                               sweep=training.get("sweep", None))
    if resume:
        batch.load(resume)                              # tables, counters, state, epsilon, episode index
    elif n_games == 1 and not training.get("philox_init", False):
        state = environment.reset()                     # drawn once, as trainer.py:45
        if all_tabular and not small_tabular:
            batch.set_tables(numpy.concatenate([a.table.ravel() for a in agents])[None, :], [float(state[0])])
        else:
            flat = numpy.zeros((1, batch.stride))
            for i, a in enumerate(agents):
                if isinstance(a, QTable):
                    flat[0, batch.offsets[i]:batch.offsets[i] + a.table.size] = a.table.ravel()
                else:
                    batch.nn[i].set_params(a.flat_params())     # torch's default init, as in the reference
            batch.set_tables(flat, [float(state[0])])
    else:
        batch.init_tables()

    tracker = None
    if conv_opt is not None:
        import ctypes
        from th_rl_amd.convergence import every_used
        cycle = int(batch.L.thrl_training_cycle(ctypes.byref(batch.cfg))) if isinstance(batch, GameBatch) else 1
        conv_every = every_used(conv_opt["every"], cycle)
        tracker = batch.track_convergence(conv_opt["window"], conv_every, conv_opt["snapshot"])
        if resume and os.path.isfile(os.path.join(os.path.dirname(os.path.abspath(resume)), "convergence.pt")):
            tracker.load(os.path.join(os.path.dirname(os.path.abspath(resume)), "convergence.pt"))
        n_conv = tracker.converged()
    stopped_early = False

    rewards_log = numpy.zeros((epochs, len(agents)))
    actions_log = numpy.zeros((epochs, len(agents)))

    game_logs = training.get("game_logs", None)
    if game_logs is not None and game_logs is not False:
        import torch
        gids, local = game_log_ids(game_logs, n_games, int(training.get("game_offset", 0)))
        numpy.save(os.path.join(exp_path, "game_ids.npy"), gids)
        g_rew = _npy_out(os.path.join(exp_path, "game_rewards.npy"), (epochs, len(agents), len(gids)))
        g_act = _npy_out(os.path.join(exp_path, "game_actions.npy"), (epochs, len(agents), len(gids)))
        keep = None if game_logs is True else torch.from_numpy(local).to(batch.device)
    else:
        game_logs = None
        keep = None

    spec, gs_opt = group_spec_of(config, training, n_games)
    smoother = None
    if spec is not None and spec.smooth is not None:
        from th_rl_amd.group_stats import Smoother
        smoother = Smoother(len(agents), n_games, spec.smooth, batch.device)    # one for the whole run
        gsm_files = group_stats_files(exp_path, "group_smooth", epochs, spec, gs_opt["histograms"])
        if game_logs is not None:
            g_rew_s = _npy_out(os.path.join(exp_path, "game_rewards_smooth.npy"), (epochs, len(agents), len(gids)))
            g_act_s = _npy_out(os.path.join(exp_path, "game_actions_smooth.npy"), (epochs, len(agents), len(gids)))
    xp_opt, gc_opt = opts.get("crossplay"), opts.get("greedy_cycles")
    if spec is not None and xp_opt is not None and xp_opt["steps"] > 0:
        from th_rl_amd.crossplay import MAX_POOLED_ROUNDS
        n_rounds = xp_opt["rounds"] * (spec.n_groups if xp_opt["against"] == "all" else 1)
        if n_rounds > MAX_POOLED_ROUNDS:
            raise ValueError("training.crossplay: group_stats pools the rows of at most %d rounds, this run has %d"
                             % (MAX_POOLED_ROUNDS, n_rounds))
    if spec is not None and gc_opt is not None and gc_opt["steps"] > 0:
        from th_rl_amd.crossplay import MAX_POOLED_ROUNDS
        n_rounds = 1 + gc_opt["rounds"] * (spec.n_groups if gc_opt["against"] == "all" else 1)
        if n_rounds > MAX_POOLED_ROUNDS:
            raise ValueError("training.greedy_cycles: group_stats pools the rows of at most %d rounds (the self-play "
                             "round included), this run has %d" % (MAX_POOLED_ROUNDS, n_rounds))
    if spec is not None:
        from th_rl_amd.group_stats import save_json
        save_json(os.path.join(exp_path, "groups.json"), spec.describe())
        g_files = group_stats_files(exp_path, "group", epochs, spec, gs_opt["histograms"])
    if spec is not None or game_logs is not None:
        cycle = 1
        if isinstance(batch, GameBatch):
            import ctypes
            cycle = int(batch.L.thrl_training_cycle(ctypes.byref(batch.cfg))) or 1
        sub = game_log_chunk(len(agents), n_games, cycle)

    def run_logged(n, at):
        """n episodes from epoch `at`: the mean logs, the kept games' rows into the .npy files and the per-group
        statistics, in launches whose per-game device buffers stay within the byte budget."""
        d = 0
        while d < n:
            k = min(sub, n - d)
            kw = {} if smoother is None else {"smooth": smoother}
            out = batch.run(k, per_game_logs=game_logs is not None, keep_games=keep, group_stats=spec, **kw)
            rewards_log[at + d:at + d + k] = out["reward_log"]
            actions_log[at + d:at + d + k] = out["action_log"]
            if game_logs is not None:
                g_rew[at + d:at + d + k] = out["game_reward_log"]
                g_act[at + d:at + d + k] = out["game_action_log"]
            if spec is not None:
                write_group_stats(g_files, at + d, out["group_stats"], spec.describe())
            if smoother is not None:
                write_group_stats(gsm_files, at + d, out["group_stats_smooth"], spec.describe())
                if game_logs is not None:
                    g_rew_s[at + d:at + d + k] = out["game_reward_smooth"]
                    g_act_s[at + d:at + d + k] = out["game_action_smooth"]
            d += k

    t = time.time()
    done = 0
    chunk = max(1, int(print_freq)) if print_freq else epochs
    while done < epochs:
        n = min(chunk - (done % chunk), epochs - done)
        if tracker is not None:     # cut the launch at the next check episode
            n = min(n, conv_every - batch.episode % conv_every)
        if game_logs is not None or spec is not None:
            run_logged(n, done)
        else:
            out = batch.run(n) if isinstance(batch, GameBatch) else batch.run(n, per_game_logs=False)
            rewards_log[done:done + n] = out["reward_log"]
            actions_log[done:done + n] = out["action_log"]
        done += n
        if tracker is not None and tracker.due():
            # the count crosses to the host (and waits for the device) only when a stop or a progress line needs it
            counted = tracker.check(count=conv_opt["stop"] is not None or bool(print_freq and not done % print_freq))
            n_conv = n_conv if counted is None else counted
            if conv_opt["stop"] is not None:
                total_conv, total_games = _run_totals(n_conv, n_games)
                stopped_early = done < epochs and total_conv >= conv_opt["stop"] * total_games
        if print_freq and not done % print_freq:
            rew = numpy.mean(rewards_log[done - print_freq:done, :], axis=0)
            act = numpy.mean(actions_log[done - print_freq:done, :], axis=0)
            line = _progress_line(print_eps, _eps_of_game0(batch), time.time() - t, done - 1, rew, act, names)
            if tracker is not None:
                line += " | converged:{:.3f}".format(n_conv / n_games)
            print(line)
            t = time.time()
        if stopped_early:
            break
    episodes_run = done

    # Store result: the reference's artefacts, from game 0
    for i, a in enumerate(agents):
        if isinstance(a, QTable):
            a.table = batch.table(0, i)
            a.counter = batch.counter_of(0, i)
            a.epsilon = _eps_of_game0(batch)[i]
        else:
            a.set_flat_params(batch.nn[i].params[0].cpu().numpy())
        a.save(os.path.join(exp_path, str(i)))
    environment.state = numpy.float64(batch.states_numpy()[0])

    with open(os.path.join(exp_path, "config.json"), "w") as f:
        json.dump(config, f, indent=3)

    rpd = pandas.DataFrame(data=rewards_log[:episodes_run], columns=numpy.arange(len(agents)))
    apd = pandas.DataFrame(data=actions_log[:episodes_run], columns=numpy.arange(len(agents)))
    log = pandas.concat([rpd, apd], axis=1, keys=["rewards", "actions"])
    log.to_csv(os.path.join(exp_path, "log.csv"), index=None)
    if game_logs is not None and g_rew.size:
        g_rew.flush()
        g_act.flush()
        if smoother is not None:
            g_rew_s.flush()
            g_act_s.flush()
    if stopped_early:       # every per-epoch artefact has episodes_run rows
        from th_rl_amd.convergence import truncate_rows
        per_epoch = []
        if game_logs is not None:
            g_rew = g_act = None
            per_epoch += ["game_rewards.npy", "game_actions.npy"]
            if smoother is not None:
                g_rew_s = g_act_s = None
                per_epoch += ["game_rewards_smooth.npy", "game_actions_smooth.npy"]
        if spec is not None:
            for f in list(g_files):
                if hasattr(g_files[f], "flush"):
                    g_files[f].flush()
                g_files[f] = None
                per_epoch.append("group_%s.npy" % f)
            if smoother is not None:
                for f in list(gsm_files):
                    if hasattr(gsm_files[f], "flush"):
                        gsm_files[f].flush()
                    gsm_files[f] = None
                    per_epoch.append("group_smooth_%s.npy" % f)
        for name in per_epoch:
            truncate_rows(os.path.join(exp_path, name), episodes_run)
    if spec is not None:
        if gs_opt["greedy_iters"] > 0:          # utils.play_game of every trained game, reduced the same way
            it = gs_opt["greedy_iters"]
            _, _, raw = batch.play_greedy(iters=it, group_stats=spec)
            gr_files = group_stats_files(exp_path, "greedy", it, spec, gs_opt["histograms"])
            write_group_stats(gr_files, 0, raw, spec.describe())
            g_files.update({"greedy_" + f: a for f, a in gr_files.items()})
        if smoother is not None:
            g_files.update({"smooth_" + f: a for f, a in gsm_files.items()})
        for arr in g_files.values():
            if hasattr(arr, "flush"):
                arr.flush()

    # the analyses asked for, in the registry's order: each reads the batch and writes its own artefacts
    if spec is not None:
        ids, n_groups = spec.ids, spec.n_groups
    elif opts:
        from th_rl_amd.group_stats import assign_groups
        ids, n_groups, _ = assign_groups(n_games, sweep=training.get("sweep", None), groups=training.get("groups", None),
                                         n_groups=training.get("n_groups", None))
    done = {}               # key -> what its writer returned: the per-run context later analyses read (Analysis.after)
    converged = None        # (tables, start prices) at convergence, fetched once
    tuple_policy = None
    if any(analysis.record(k).tuple_policy == "extract" for k in opts):
        from th_rl_amd.tuple_play import extract as extract_tuple_policy
        tuple_policy = extract_tuple_policy(batch)      # every agent's strategy in tuple form, once for all greedy_* keys
    for a in analysis.REGISTRY:
        if a.key not in opts:
            continue
        opt, kw = opts[a.key], {}
        if a.key == "convergence":      # the one analysis that ran during training: its writer takes the tracker
            kw.update(tracker=tracker, every=conv_every, episodes_run=episodes_run, stopped_early=stopped_early)
        if a.converged:
            kw.update(q=None, state0=None)
            if tracker is not None:
                opt = dict(opt, tables=opt.get("tables", "final"))
                if opt["tables"] == "converged":
                    converged = converged or tracker.tables_at_convergence()
                    kw.update(q=converged[0], state0=converged[1])
        if a.rows:
            kw.update(spec=spec, histograms=bool(gs_opt and gs_opt["histograms"]), budget=GAME_LOG_BUDGET)
        if a.tuple_policy:
            kw.update(tuple_policy=tuple_policy)
        kw.update({name: done.get(key) for name, key in a.after})
        r = getattr(analysis.module_of(a), a.write)(exp_path, batch, config, opt, ids, n_groups, **kw)
        done[a.key] = True if r is None else r

    if n_games > 1 or resume or training.get("checkpoint", False):
        batch.save(os.path.join(exp_path, "batch.pt"))


# BASELINE.json's north_star names the entry point "trainer.train()"; the reference's is train_one.
train = train_one
