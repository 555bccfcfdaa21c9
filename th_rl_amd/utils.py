"""Evaluation helpers on the training path's edge (reference th_rl/utils.py:12-47).
The plotting functions of the reference are out of scope."""
import os

import numpy
import pandas

from th_rl_amd.trainer import create_game


def load_experiment(loc):
    """(config, agents, environment, actions, rewards) from a run directory, as utils.py:12-24."""
    config, agents, environment = create_game(os.path.join(loc, "config.json"))
    for i, agent in enumerate(agents):
        agent.load(os.path.join(loc, str(i)))
    log = pandas.read_csv(os.path.join(loc, "log.csv"))
    names = [a["name"] + str(i) for i, a in enumerate(config["agents"])]
    rcols = [c for c in log.columns if c.startswith("rewards")]
    acols = [c for c in log.columns if c.startswith("actions")]
    rewards = log[rcols].ewm(halflife=1000).mean()
    actions = log[acols].ewm(halflife=1000).mean()
    rewards.columns = names
    actions.columns = names
    return config, agents, environment, actions, rewards


def play_game(agents, environment, iters=1):
    """Greedy rollout through the object protocol (each call runs a device operator)."""
    rewards, actions = [], []
    for _ in range(iters):
        done = False
        next_state = environment.reset()
        while not done:
            acts = [agent.get_action(next_state) for agent in agents]
            scaled_acts = [agent.scale(act) for agent, act in zip(agents, acts)]
            next_state, reward, done = environment.step(scaled_acts)
            rewards.append(reward)
            actions.append(scaled_acts)
    return numpy.array(actions), numpy.array(rewards)


def play_game_batched(batch, iters=1, state0=None):
    """The same rollout for every game of a GameBatch in one kernel (thrl_play_greedy):
    per-iteration mean reward / mean scaled action, arrays [iters, N, G]."""
    return batch.play_greedy(iters=iters, state0=state0)


def game_log(exp_path, game_id, smooth=False):
    """One game's learning curve from a run trained with training.game_logs: a DataFrame with log.csv's columns
    (rewards / actions x agent, as train_one builds it) and one row per epoch.  The game is looked up by its GLOBAL
    id in exp_path's game_ids.npy and in those of exp_path/shard*/ (th_rl_amd.launch writes one set per rank).
    smooth=True: the curve smoothed on the device (game_rewards_smooth.npy / game_actions_smooth.npy of a run that
    also had training.group_stats.smooth), what the reference's load_experiment returns for a single run."""
    suffix = "_smooth" if smooth else ""
    import glob
    dirs = [exp_path] + sorted(glob.glob(os.path.join(exp_path, "shard*")))
    for d in dirs:
        ids_path = os.path.join(d, "game_ids.npy")
        if not os.path.isfile(ids_path):
            continue
        hit = numpy.flatnonzero(numpy.load(ids_path) == int(game_id))
        if hit.size:
            k = int(hit[0])
            if smooth and not os.path.isfile(os.path.join(d, "game_rewards_smooth.npy")):
                raise KeyError("game %d has no smoothed per-game log under %s (training.group_stats.smooth)"
                               % (int(game_id), d))
            rew = numpy.load(os.path.join(d, "game_rewards%s.npy" % suffix), mmap_mode="r")[:, :, k]
            act = numpy.load(os.path.join(d, "game_actions%s.npy" % suffix), mmap_mode="r")[:, :, k]
            n = rew.shape[1]
            rpd = pandas.DataFrame(data=numpy.array(rew), columns=numpy.arange(n))
            apd = pandas.DataFrame(data=numpy.array(act), columns=numpy.arange(n))
            return pandas.concat([rpd, apd], axis=1, keys=["rewards", "actions"])
    raise KeyError("game %d has no per-game log under %s (training.game_logs)" % (int(game_id), exp_path))


def load_group_stats(exp_path, prefix="group"):
    """(describe, fields) of a run trained with training.group_stats: groups.json and the group_*.npy (prefix
    "greedy": greedy_*.npy; "group_smooth": those of the smoothed curves, training.group_stats.smooth) of exp_path; when exp_path has none but exp_path/shard*/ do (a sharded run stopped before
    rank 0 merged them), the shards' raw outputs merged exactly (group_stats.merge)."""
    import glob
    import json
    from th_rl_amd import group_stats as gs
    top = os.path.join(exp_path, "groups.json")
    shards = sorted(glob.glob(os.path.join(exp_path, "shard*")))
    if os.path.isfile(os.path.join(exp_path, "%s_mean.npy" % prefix)):
        desc = json.load(open(top))
        fields = {f: numpy.load(os.path.join(exp_path, "%s_%s.npy" % (prefix, f)), mmap_mode="r")
                  for f in ("mean", "std", "min", "max", "quantiles")}
        return desc, fields
    have = [d for d in shards if os.path.isfile(os.path.join(d, "%s_hist.npy" % prefix))]
    if not have:
        raise KeyError("no per-group statistics (%s_*.npy) under %s (training.group_stats)" % (prefix, exp_path))
    desc = json.load(open(os.path.join(have[0], "groups.json")))
    parts = []
    for d in have:
        ld = lambda f: numpy.load(os.path.join(d, "%s_%s.npy" % (prefix, f)))
        vmin, vmax = ld("min"), ld("max")
        kmin = numpy.where(numpy.isnan(vmin), numpy.uint64(0), ~gs.order_key(numpy.nan_to_num(vmin)))
        kmax = numpy.where(numpy.isnan(vmax), numpy.uint64(0), gs.order_key(numpy.nan_to_num(vmax)))
        parts.append({"hist": ld("hist"), "sums": ld("sums"), "minmax": numpy.stack([kmin, kmax], axis=-1)})
    return desc, gs.finalize(gs.merge(parts), desc)


def group_log(exp_path, group, prefix="group"):
    """Group `group`'s mean curve over its games, with log.csv's columns (rewards / actions x agent), one row per
    epoch (prefix "greedy": per greedy iteration; prefix "group_smooth": the mean over the group's games of the curves
    smoothed per game, with training.group_stats.smooth)."""
    desc, f = load_group_stats(exp_path, prefix)
    n = (len(desc["quantities"]) - 1) // 2
    m = numpy.array(f["mean"][:, int(group), :])
    rpd = pandas.DataFrame(data=m[:, :n], columns=numpy.arange(n))
    apd = pandas.DataFrame(data=m[:, n:2 * n], columns=numpy.arange(n))
    return pandas.concat([rpd, apd], axis=1, keys=["rewards", "actions"])


def _quantile_column(q):
    return {0.5: "median", 0.0: "min", 1.0: "max"}.get(float(q), "%gth" % (100.0 * float(q)))


def group_quantiles(exp_path, group, quantity="total", prefix="group"):
    """utils.plot_learning_curve_conf's data for one group: a DataFrame with one column per configured quantile
    ("25th", "median", "75th" for the default [0.25, 0.5, 0.75]) of `quantity` over the group's games, one row per
    epoch, plus "Nash" and "Cartel" from environment.get_optimal() (the reference hard-codes 22.22 and 25).  The
    reference smooths every run's curve before it takes these quantiles: prefix="group_smooth" (a run with
    training.group_stats.smooth, halflife 1000 for the reference's) gives the quantiles of the smoothed curves."""
    desc, f = load_group_stats(exp_path, prefix)
    names = desc["quantities"]
    if quantity not in names:
        raise KeyError("quantity %r is not one of %s" % (quantity, names))
    q = names.index(quantity)
    vals = numpy.array(f["quantiles"][:, int(group), q, :])
    df = pandas.DataFrame(data=vals, columns=[_quantile_column(x) for x in desc["quantiles"]])
    cfg_dir = exp_path if os.path.isfile(os.path.join(exp_path, "config.json")) else None
    if cfg_dir is None:
        import glob
        hits = sorted(glob.glob(os.path.join(exp_path, "shard*", "shard_config.json")))
        path = hits[0] if hits else None
    else:
        path = os.path.join(cfg_dir, "config.json")
    if path is not None:
        _, _, environment = create_game(path)
        nash, cartel = environment.get_optimal()
        df["Nash"], df["Cartel"] = float(nash), float(cartel)
    return df


def _load_json(d, name):
    import json
    with open(os.path.join(d, name)) as f:
        return json.load(f)


def _run_dirs(exp_path, probe, what, key, shards=True):
    """The directories that hold an analysis's per-game arrays: exp_path when it has the file `probe`, else (with
    shards) its shard* subdirectories that have it, in rank order (th_rl_amd.launch writes one set per rank).
    KeyError when there is none."""
    import glob
    if os.path.isfile(os.path.join(exp_path, probe)):
        return [exp_path]
    dirs = []
    if shards:
        dirs = sorted((d for d in glob.glob(os.path.join(exp_path, "shard*")) if os.path.isfile(os.path.join(d, probe))),
                      key=lambda d: int(os.path.basename(d)[5:]))
    if not dirs:
        raise KeyError("no %s (%s) under %s (training.%s)" % (what, probe, exp_path, key))
    return dirs


def _game_offset(d, exp_path):
    """The global id of the first game of run directory `d`: training.game_offset of its config.json (a shard's
    shard_config.json), 0 without one."""
    name = "shard_config.json" if d != exp_path else "config.json"
    if not os.path.isfile(os.path.join(d, name)):
        return 0
    return int(_load_json(d, name).get("training", {}).get("game_offset", 0))


def deviation_summary(exp_path):
    """A run's deviation analysis (training.deviation): deviation.json's summary as a DataFrame with one row per
    (group, deviator) -- games, cycles, fixed_points, returned, unprofitable, ret_step_mean, the profit gain's mean
    and quantiles (delta_*), gain_mean, and one lam_<bin> column per bin of the lam histogram -- plus Nash and Cartel.
    The response curves of a run that also has training.group_stats are the per-group statistics of prefix
    "dev<d>": group_quantiles(exp_path, group, "total", prefix="dev0") and group_log(exp_path, group, prefix="dev0"),
    one row per period after the shock.  mu and lam of deviation_games are those of equilibrium_games for the same run
    (same tables, same start prices, default horizon)."""
    desc = _load_json(exp_path, "deviation.json")
    rows = []
    for r in desc["summary"]:
        r = dict(r)
        for name, n in zip(desc["lam_bins"], r.pop("lam_hist")):
            r["lam_" + name] = n
        rows.append(r)
    df = pandas.DataFrame(rows)
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def deviation_games(exp_path, deviator=0):
    """Per-game results of the deviation analysis for `deviator`, one row per game indexed by its GLOBAL id: mu, lam,
    mu_post, lam_post, ret_step, act_dev, gain, cycle_reward_<i> / cycle_action_<i> and the profit gain delta.  Reads
    exp_path's dev*.npy, or those of exp_path/shard*/ (th_rl_amd.launch writes one set per rank) in game order."""
    from th_rl_amd import deviation as dv
    dirs = _run_dirs(exp_path, "dev_cycle.npy", "deviation analysis", "deviation")
    frames = []
    for d in dirs:
        g = dv.load_games(d, int(deviator))
        nash, cartel = dv.optimal(_load_json(d, "shard_config.json" if d != exp_path else "config.json"))
        off = _game_offset(d, exp_path)
        n = g["gain"].shape[0]
        cols = {f: g[f] for f in dv.INT_FIELDS}
        cols["gain"] = g["gain"]
        for i in range(g["cycle_reward"].shape[0]):
            cols["cycle_reward_%d" % i] = g["cycle_reward"][i]
            cols["cycle_action_%d" % i] = g["cycle_action"][i]
        cols["delta"] = dv.profit_gain(g["cycle_reward"], nash, cartel)
        frames.append(pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def deviation_noise_summary(exp_path):
    """A run's deviation test under demand noise (training.deviation with "noise"): deviation_noise.json's summary as a
    DataFrame with one row per (group, deviator) -- games, solved, deviates, dev_share_mean, unprofitable, gain_mean and
    gain_q*, gain_dev_mean, low_mean, returned, ret_step_mean, dist_mean.  The expected response curves of a run that
    also has training.group_stats are the per-group statistics of prefix "devn<d>":
    group_quantiles(exp_path, group, "total", prefix="devn0"), one row per period after the shock."""
    if not os.path.isfile(os.path.join(exp_path, "deviation_noise.json")):
        raise KeyError("no deviation test under noise (deviation_noise.json) under %s (training.deviation.noise)" % exp_path)
    desc = _load_json(exp_path, "deviation_noise.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_cells"] = int(desc["n_cells"])
    return df


def deviation_noise_games(exp_path, deviator=0):
    """Per-game results of the deviation test under demand noise for `deviator`, one row per game indexed by its GLOBAL
    id: noise_prob, stat_iters, dev_share, gain, gain_dev, low, dist, mass, low_step, ret_step, base_reward_<i> /
    base_action_<i> and solved.  Reads exp_path's devn*.npy, or those of exp_path/shard*/ in game order."""
    from th_rl_amd import deviation as dv
    dirs = _run_dirs(exp_path, "devn_prob.npy", "deviation test under noise", "deviation.noise")
    frames = []
    for d in dirs:
        off = _game_offset(d, exp_path)
        g = dv.load_noise_games(d, int(deviator))
        cols = {"noise_prob": g["noise_prob"], "stat_iters": g["stat_iters"]}
        cols.update({f: g[f] for f in dv.NOISE_FLOAT + dv.NOISE_INT})
        for i in range(g["base_reward"].shape[0]):
            cols["base_reward_%d" % i] = g["base_reward"][i]
            cols["base_action_%d" % i] = g["base_action"][i]
        cols["solved"] = dv.solved_noise(g)
        n = g["noise_prob"].shape[0]
        frames.append(pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def equilibrium_summary(exp_path):
    """A run's equilibrium check (training.equilibrium): equilibrium.json's summary as a DataFrame.  Rows with an
    agent: games, br_on, br_all (fractions of games in which the agent's greedy strategy is a best response on the
    path / in every state), loss_on_q* / loss_all_q* (over the games with a positive loss), capped.  Rows with agent
    NaN: the group's nash and perfect fractions and, when the run has training.deviation, collusive (games with
    profit gain above collusive_gain), nash_collusive and perfect_collusive.  mu and lam of equilibrium_games are those
    of deviation_games for the same run (same tables, same start prices, default horizon)."""
    desc = _load_json(exp_path, "equilibrium.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_states"] = int(desc["n_states"])
    df["tol"] = float(desc["options"]["tol"])
    return df


def equilibrium_games(exp_path, agent=0):
    """Per-game results of the equilibrium check for `agent`, one row per game indexed by its GLOBAL id: mu, lam,
    iters, n_diff_all, n_diff_on, loss_all, loss_on, loss_all_mean, loss_on_mean, v_on, and the flags br_on, br_all
    (this agent) and nash, perfect (all solved agents) at the run's tol.  Reads exp_path's eq_*.npy, or those of
    exp_path/shard*/ in game order.  mu and lam equal deviation_games' for the same run."""
    from th_rl_amd import equilibrium as eq
    dirs = _run_dirs(exp_path, "eq_cycle.npy", "equilibrium check", "equilibrium")
    frames = []
    for d in dirs:
        opt = _load_json(d, "equilibrium.json")["options"]
        off = _game_offset(d, exp_path)
        g = eq.load_games(d)
        fl = eq.flags(g, opt["agents"], opt["tol"])
        cols = {"mu": g["mu"], "lam": g["lam"]}
        for f in eq.INT_FIELDS + eq.FLOAT_FIELDS:
            cols[f] = g[f][int(agent)]
        cols.update(br_on=fl["br_on"][int(agent)], br_all=fl["br_all"][int(agent)], nash=fl["nash"], perfect=fl["perfect"])
        n = g["mu"].shape[0]
        frames.append(pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def equilibrium_noise_summary(exp_path):
    """A run's equilibrium check under demand noise (training.equilibrium with "noise"): equilibrium_noise.json's
    summary as a DataFrame.  Rows with an agent: games, capped, br_all, br_w (fractions of games in which the agent's
    greedy strategy is a best response in every cell / where noisy greedy play is in the long run), loss_all_q* /
    loss_w_q* (over the games with a positive loss), diff_w_mean, sweeps_max.  Rows with agent NaN: the group's perfect
    fraction."""
    if not os.path.isfile(os.path.join(exp_path, "equilibrium_noise.json")):
        raise KeyError("no equilibrium check under noise (equilibrium_noise.json) under %s (training.equilibrium.noise)"
                       % exp_path)
    desc = _load_json(exp_path, "equilibrium_noise.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_cells"] = int(desc["n_cells"])
    df["tol"] = float(desc["options"]["tol"])
    return df


def equilibrium_noise_games(exp_path, agent=0):
    """Per-game results of the equilibrium check under demand noise for `agent`, one row per game indexed by its GLOBAL
    id: noise_prob, iters, sweeps, n_diff_all, loss_all, loss_all_mean, loss_w, diff_w, v_w, and the flags br_all, br_w
    (this agent) and perfect (all solved agents) at the run's tol.  Reads exp_path's eqn_*.npy, or those of
    exp_path/shard*/ in game order."""
    from th_rl_amd import equilibrium as eq
    dirs = _run_dirs(exp_path, "eqn_iters.npy", "equilibrium check under noise", "equilibrium.noise")
    frames = []
    for d in dirs:
        opt = _load_json(d, "equilibrium_noise.json")["options"]
        off = _game_offset(d, exp_path)
        g = eq.load_noise_games(d)
        fl = eq.flags_noise(g, opt["agents"], opt["tol"])
        cols = {"noise_prob": g["noise_prob"]}
        for f in eq.NOISE_INT + eq.NOISE_FLOAT + eq.NOISE_WEIGHTED:
            if f in g:
                cols[f] = g[f][int(agent)]
        cols["br_all"] = fl["br_all"][int(agent)]
        if "br_w" in fl:
            cols["br_w"] = fl["br_w"][int(agent)]
        cols["perfect"] = fl["perfect"]
        n = g["noise_prob"].shape[0]
        frames.append(pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def crossplay_summary(exp_path):
    """A run's cross-play (training.crossplay): crossplay.json's summary as a DataFrame with one row per (group of
    seat 0, partner_group) -- matches, cycles, fixed_points, the cross-play profit gain's mean and quantiles (delta_*),
    delta_self_mean (the same games in self-play), retained, seat_gain_<i> and one lam_<bin> column per bin of the lam
    histogram -- plus Nash and Cartel.  In a sharded run the partners were drawn inside each shard."""
    desc = _load_json(exp_path, "crossplay.json")
    rows = []
    for r in desc["summary"]:
        r = dict(r)
        for name, n in zip(desc["lam_bins"], r.pop("lam_hist")):
            r["lam_" + name] = n
        for i, v in enumerate(r.pop("seat_gain")):
            r["seat_gain_%d" % i] = v
        rows.append(r)
    df = pandas.DataFrame(rows)
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def crossplay_games(exp_path, round=0):
    """Per-match results of cross-play round `round`, one row per match indexed by the GLOBAL id of seat 0's game: seat_<i>
    (global game ids), self_seat, mu, lam, cycle_reward_<i> / cycle_action_<i>, the profit gain delta, and the same
    game's self-play lam_self and delta_self.  Reads exp_path's xplay_*.npy, or those of exp_path/shard*/
    (th_rl_amd.launch writes one set per rank) in game order."""
    from th_rl_amd import crossplay as xp
    dirs = _run_dirs(exp_path, "xplay_cycle.npy", "cross-play", "crossplay")
    frames = []
    for d in dirs:
        desc = _load_json(d, "crossplay.json")
        g, sp = xp.load_games(d)
        r = int(round)
        if not 0 <= r < g["seats"].shape[0]:
            raise KeyError("round %d out of [0, %d)" % (r, g["seats"].shape[0]))
        seats = g["seats"][r]
        cols = {"seat_%d" % i: seats[i] for i in range(seats.shape[0])}
        cols.update(self_seat=xp.self_seat(seats), mu=g["mu"][r], lam=g["lam"][r])
        for i in range(seats.shape[0]):
            cols["cycle_reward_%d" % i] = g["cycle_reward"][r, i]
            cols["cycle_action_%d" % i] = g["cycle_action"][r, i]
        cols["delta"] = xp.profit_gain(g["cycle_reward"][r], desc["nash"], desc["cartel"])
        cols["lam_self"] = sp["lam"]
        cols["delta_self"] = xp.profit_gain(sp["cycle_reward"], desc["nash"], desc["cartel"])
        frames.append(pandas.DataFrame(cols, index=pandas.Index(seats[0], name="game")))
    return pandas.concat(frames)


def greedy_cycle_summary(exp_path):
    """A run's greedy cycles (training.greedy_cycles, any mix of QTable / Reinforce / ActorCritic agents):
    greedy_cycles.json as a pair of DataFrames.  The first has one row per group for the self-play round -- matches,
    no_start (games whose state is no tuple's price), cycles, fixed_points, the profit gain's mean and quantiles
    (delta_*) and one lam_<bin> column per bin of the lam histogram; the second one row per (group of seat 0,
    partner_group) over the re-seated rounds, with crossplay_summary's columns and no_start (empty without such
    rounds).  Both carry Nash and Cartel."""
    desc = _load_json(exp_path, "greedy_cycles.json")

    def frame(rows):
        out = []
        for r in rows:
            r = dict(r)
            for name, n in zip(desc["lam_bins"], r.pop("lam_hist")):
                r["lam_" + name] = n
            for i, v in enumerate(r.pop("seat_gain", [])):
                r["seat_gain_%d" % i] = v
            out.append(r)
        df = pandas.DataFrame(out)
        df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
        return df

    return frame(desc["self_play"]), frame(desc["summary"])


def greedy_cycle_games(exp_path, round=0):
    """Per-match results of round `round` of training.greedy_cycles (0 = every game's own agents, k >= 1 the k-th
    re-seating), one row per match indexed by the GLOBAL id of seat 0's game: seat_<i> (global game ids), start (the
    start tuple, -1 = none), mu, lam, cycle_start, cycle_reward_<i> / cycle_action_<i> and the profit gain delta."""
    from th_rl_amd import tuple_play as tp
    _run_dirs(exp_path, "gcyc_cycle.npy", "greedy cycles", "greedy_cycles", shards=False)
    desc = _load_json(exp_path, "greedy_cycles.json")
    g = tp.load_games(exp_path)
    r = int(round)
    if not 0 <= r < g["seats"].shape[0]:
        raise KeyError("round %d out of [0, %d)" % (r, g["seats"].shape[0]))
    seats = g["seats"][r]
    cols = {"seat_%d" % i: seats[i] for i in range(seats.shape[0])}
    cols.update(start=g["start"][r], mu=g["mu"][r], lam=g["lam"][r], cycle_start=g["cycle_start"][r])
    for i in range(seats.shape[0]):
        cols["cycle_reward_%d" % i] = g["cycle_reward"][r, i]
        cols["cycle_action_%d" % i] = g["cycle_action"][r, i]
    cols["delta"] = tp.profit_gain(g["cycle_reward"][r], desc["nash"], desc["cartel"])
    return pandas.DataFrame(cols, index=pandas.Index(seats[0], name="game"))


def attractor_summary(exp_path):
    """A run's attractor analysis (training.attractors): attractors.json's summary as a DataFrame with one row per
    group -- games, single, the quantiles of n_attr and mu_max, delta_train_mean / delta_largest_mean /
    delta_reset_mean (profit gains of the training state's attractor, of the largest basin and in expectation over the
    environment's reset distribution), train_is_largest, train_mass_q*, luck_mean -- plus n_states, n_starts, Nash
    and Cartel."""
    desc = _load_json(exp_path, "attractors.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_states"], df["n_starts"] = int(desc["n_states"]), int(desc["n_starts"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def attractor_games(exp_path):
    """Per-game results of the attractor analysis, one row per game indexed by its GLOBAL id: n_attr, mu_max,
    n_cycle_states, rep_x0, mu_x0, slot_x0, per kept slot k rep_<k>, lam_<k>, basin_<k>, delta_<k> (its profit gain, NaN
    past n_attr) and mass_<k>, and delta_train, delta_reset, mass_other.  Reads exp_path's attr_*.npy, or those of
    exp_path/shard*/ (th_rl_amd.launch writes one set per rank) in game order."""
    from th_rl_amd import attractors as at
    dirs = _run_dirs(exp_path, "attr_games.npy", "attractor analysis", "attractors")
    frames = []
    for d in dirs:
        desc = _load_json(d, "attractors.json")
        off = _game_offset(d, exp_path)
        g = at.load_games(d)
        gn = at.gains(g, desc["nash"], desc["cartel"])
        cols = {f: g[f] for f in at.GAME_INT}
        for k in range(g["rep"].shape[0]):
            cols.update({"rep_%d" % k: g["rep"][k], "lam_%d" % k: g["lam"][k], "basin_%d" % k: g["basin"][k]})
            cols["delta_%d" % k] = numpy.where(g["rep"][k] >= 0, at.profit_gain(g["cycle_reward"][k], desc["nash"], desc["cartel"]),
                                               numpy.nan)
            if "reset_mass" in g:
                cols["mass_%d" % k] = g["reset_mass"][k]
        cols["delta_train"] = gn["train"]
        if gn["reset"] is not None:
            cols["delta_reset"] = gn["reset"]
            cols["mass_other"] = g["reset_mass_other"]
        n = g["n_attr"].shape[0]
        frames.append(pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def stationary_summary(exp_path):
    """A run's stationary analysis (training.stationary: greedy play under demand noise): stationary.json's summary as
    a DataFrame with one row per group -- games, converged (share with iters < max_iters), iters_q25 / q50 / q75 / max,
    delta_noise_mean / q25 / q50 / q75 (deviation.profit_gain of the long-run reward stat_reward; Nash and Cartel are
    deviation.optimal(config), the NOISE-FREE benchmark of every other analysis, so a delta below the noise-free one
    also carries the demand the noise removes), price_mean and, when attr_reset_reward.npy (training.attractors) is in
    the same directory, delta_reset_mean and noise_cost_mean = delta_reset - delta_noise -- plus n_cells, Nash and
    Cartel."""
    desc = _load_json(exp_path, "stationary.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_cells"] = int(desc["n_cells"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def stationary_games(exp_path):
    """Per-game results of the stationary analysis, one row per game indexed by its GLOBAL id: iters, change, mass,
    noise_prob, price, reward_<i>, action_<i>, delta_noise (against the noise-free Nash / Cartel) and, with
    attr_reset_reward.npy beside them, delta_reset.  Reads exp_path's stat_*.npy, or those of exp_path/shard*/
    (th_rl_amd.launch writes one set per rank) in game order."""
    from th_rl_amd import stationary as sn
    dirs = _run_dirs(exp_path, "stat_iters.npy", "stationary analysis", "stationary")
    frames = []
    for d in dirs:
        desc = _load_json(d, "stationary.json")
        off = _game_offset(d, exp_path)
        g = sn.load_games(d)
        cols = {"iters": g["iters"], "change": g["change"], "mass": g["mass"], "noise_prob": g["noise_prob"],
                "price": g["stat_price"]}
        for i in range(g["stat_reward"].shape[0]):
            cols["reward_%d" % i], cols["action_%d" % i] = g["stat_reward"][i], g["stat_action"][i]
        cols["delta_noise"] = sn.profit_gain(g["stat_reward"], desc["nash"], desc["cartel"])
        rr = sn.reset_reward_of(d, g["iters"].shape[0])
        if rr is not None:
            cols["delta_reset"] = sn.profit_gain(rr, desc["nash"], desc["cartel"])
        n = g["iters"].shape[0]
        frames.append(pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def convergence_summary(exp_path):
    """A run's convergence (training.convergence): convergence.json's summary as a DataFrame with one row per group --
    games, converged, fraction, converged_at_mean / q25 / q50 / q75, conv_since_mean / q25 / q50 / q75 (over the
    converged games), still_stable, changes_mean -- plus the run's window, every_used, episodes_run and
    stopped_early."""
    desc = _load_json(exp_path, "convergence.json")
    df = pandas.DataFrame(desc["summary"])
    df["window"] = int(desc["options"]["window"])
    df["every_used"] = int(desc["every_used"])
    df["episodes_run"] = int(desc["episodes_run"])
    df["stopped_early"] = bool(desc["stopped_early"])
    return df


def convergence_games(exp_path):
    """Per-game convergence, one row per game indexed by its GLOBAL id: converged_at (-1 = never), conv_since,
    stable_since, changes.  Reads exp_path's conv_*.npy, or those of exp_path/shard*/ in game order."""
    from th_rl_amd import convergence as cv
    dirs = _run_dirs(exp_path, "conv_episode.npy", "convergence arrays", "convergence")
    frames = []
    for d in dirs:
        off = _game_offset(d, exp_path)
        g = cv.load_games(d)
        n = g["converged_at"].shape[0]
        frames.append(pandas.DataFrame({f: g[f] for f in cv.FILES}, index=pandas.RangeIndex(off, off + n, name="game")))
    return pandas.concat(frames)


def greedy_deviation_summary(exp_path):
    """A run's deviation test in tuple form (training.greedy_deviation, any mix of QTable / Reinforce / ActorCritic
    agents): greedy_deviation.json's summary as a DataFrame with deviation_summary's columns, one row per (group,
    deviator), plus no_start (the group's games whose state is no tuple's price: refused, lam = 0) and T."""
    desc = _load_json(exp_path, "greedy_deviation.json")
    rows = []
    for r in desc["summary"]:
        r = dict(r)
        for name, n in zip(desc["lam_bins"], r.pop("lam_hist")):
            r["lam_" + name] = n
        rows.append(r)
    df = pandas.DataFrame(rows)
    df["Nash"], df["Cartel"], df["T"] = float(desc["nash"]), float(desc["cartel"]), int(desc["T"])
    return df


def greedy_deviation_games(exp_path, deviator=0):
    """Per-game results of training.greedy_deviation for `deviator`, one row per game indexed by its GLOBAL id: start
    (the start tuple, -1 = none), mu, lam, mu_post, lam_post, ret_step, act_dev, gain, cycle_reward_<i> /
    cycle_action_<i> and the profit gain delta."""
    from th_rl_amd import deviation as dv, tuple_analysis as ta
    _run_dirs(exp_path, "gdev_cycle.npy", "deviation test in tuple form", "greedy_deviation", shards=False)
    desc = _load_json(exp_path, "greedy_deviation.json")
    if int(deviator) not in desc["options"]["agents"]:
        raise KeyError("deviator %d was not analysed (agents %s)" % (int(deviator), desc["options"]["agents"]))
    off = _game_offset(exp_path, exp_path)
    g = ta.load_deviation_games(exp_path, int(deviator))
    cols = {"start": g["start"]}
    cols.update({f: g[f] for f in dv.INT_FIELDS})
    cols["gain"] = g["gain"]
    for i in range(g["cycle_reward"].shape[0]):
        cols["cycle_reward_%d" % i] = g["cycle_reward"][i]
        cols["cycle_action_%d" % i] = g["cycle_action"][i]
    cols["delta"] = dv.profit_gain(g["cycle_reward"], desc["nash"], desc["cartel"])
    n = g["gain"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def greedy_deviation_noise_summary(exp_path):
    """A run's deviation test under demand noise in tuple form (training.greedy_deviation with "noise"):
    greedy_deviation_noise.json's summary as a DataFrame with deviation_noise_summary's columns, one row per (group,
    deviator), plus n_switch_max and unresolved_mean (the sampling of the networks' strategies on the price cells), T and
    n_cells.  The expected response curves of a run that also has training.group_stats are the per-group statistics of
    prefix "gdevn<d>": group_quantiles(exp_path, group, "total", prefix="gdevn0"), one row per period after the shock."""
    if not os.path.isfile(os.path.join(exp_path, "greedy_deviation_noise.json")):
        raise KeyError("no deviation test under noise in tuple form (greedy_deviation_noise.json) under %s "
                       "(training.greedy_deviation.noise)" % exp_path)
    desc = _load_json(exp_path, "greedy_deviation_noise.json")
    df = pandas.DataFrame(desc["summary"])
    df["T"], df["n_cells"] = int(desc["T"]), int(desc["n_cells"])
    return df


def greedy_deviation_noise_games(exp_path, deviator=0):
    """Per-game results of the deviation test under demand noise in tuple form for `deviator`, one row per game indexed
    by its GLOBAL id: noise_prob, stat_iters, n_switch, unresolved, dev_share, gain, gain_dev, low, dist, mass, low_step,
    ret_step, base_reward_<i> / base_action_<i> and solved."""
    from th_rl_amd import deviation as dv, tuple_analysis as ta
    _run_dirs(exp_path, "gdevn_prob.npy", "deviation test under noise in tuple form", "greedy_deviation.noise", shards=False)
    desc = _load_json(exp_path, "greedy_deviation_noise.json")
    if int(deviator) not in desc["options"]["agents"]:
        raise KeyError("deviator %d was not analysed (agents %s)" % (int(deviator), desc["options"]["agents"]))
    off = _game_offset(exp_path, exp_path)
    g = ta.load_deviation_noise_games(exp_path, int(deviator))
    cols = {f: g[f] for f in ("noise_prob", "stat_iters", "n_switch", "unresolved")}
    cols.update({f: g[f] for f in dv.NOISE_FLOAT + dv.NOISE_INT})
    for i in range(g["base_reward"].shape[0]):
        cols["base_reward_%d" % i] = g["base_reward"][i]
        cols["base_action_%d" % i] = g["base_action"][i]
    cols["solved"] = dv.solved_noise(g)
    n = g["noise_prob"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def greedy_equilibrium_summary(exp_path):
    """A run's equilibrium check in tuple form (training.greedy_equilibrium): greedy_equilibrium.json's summary as a
    DataFrame with equilibrium_summary's columns (n_states = T, the game's action tuples) plus no_start."""
    desc = _load_json(exp_path, "greedy_equilibrium.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_states"] = int(desc["n_states"])
    df["tol"] = float(desc["options"]["tol"])
    return df


def greedy_equilibrium_games(exp_path, agent=0):
    """Per-game results of training.greedy_equilibrium for `agent`, one row per game indexed by its GLOBAL id: start,
    mu, lam, equilibrium_games' columns for this agent and the flags br_on, br_all (this agent) and nash, perfect (all
    solved agents) at the run's tol."""
    from th_rl_amd import equilibrium as eq, tuple_analysis as ta
    _run_dirs(exp_path, "geq_cycle.npy", "equilibrium check in tuple form", "greedy_equilibrium", shards=False)
    opt = _load_json(exp_path, "greedy_equilibrium.json")["options"]
    off = _game_offset(exp_path, exp_path)
    g = ta.load_equilibrium_games(exp_path)
    fl = eq.flags(g, opt["agents"], opt["tol"])
    cols = {"start": g["start"], "mu": g["mu"], "lam": g["lam"]}
    for f in eq.INT_FIELDS + eq.FLOAT_FIELDS:
        cols[f] = g[f][int(agent)]
    cols.update(br_on=fl["br_on"][int(agent)], br_all=fl["br_all"][int(agent)], nash=fl["nash"], perfect=fl["perfect"])
    n = g["mu"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def greedy_equilibrium_noise_summary(exp_path):
    """A run's equilibrium check under demand noise in tuple form (training.greedy_equilibrium with "noise"):
    greedy_equilibrium_noise.json as a DataFrame.  Rows with an agent: games, capped, br_all, br_w (fractions of games in
    which the agent's strategy is a best response in every state / where noisy play makes its decisions in the long
    run), loss_all_q* / loss_w_q* (over the games with a positive loss), diff_w_mean, sweeps_max, diff_tuples_mean,
    diff_cells_mean.  Rows with agent NaN: the group's perfect fraction."""
    if not os.path.isfile(os.path.join(exp_path, "greedy_equilibrium_noise.json")):
        raise KeyError("no equilibrium check under noise in tuple form (greedy_equilibrium_noise.json) under %s "
                       "(training.greedy_equilibrium.noise)" % exp_path)
    desc = _load_json(exp_path, "greedy_equilibrium_noise.json")
    df = pandas.DataFrame(desc["summary"] + desc["perfect"])
    df["n_cells"], df["T"] = int(desc["n_cells"]), int(desc["T"])
    df["tol"] = float(desc["options"]["tol"])
    return df


def greedy_equilibrium_noise_games(exp_path, agent=0):
    """Per-game results of the equilibrium check under demand noise in tuple form for `agent`, one row per game indexed
    by its GLOBAL id: noise_prob, iters, sweeps, n_diff_tuples, n_diff_cells, loss_all, loss_tuples_mean,
    loss_cells_mean, loss_w, diff_w, v_w, and the flags br_all, br_w (this agent) and perfect (all solved agents) at the
    run's tol."""
    from th_rl_amd import equilibrium as eq, tuple_analysis as ta
    _run_dirs(exp_path, "geqn_iters.npy", "equilibrium check under noise in tuple form", "greedy_equilibrium.noise",
              shards=False)
    opt = _load_json(exp_path, "greedy_equilibrium_noise.json")["options"]
    off = _game_offset(exp_path, exp_path)
    g = ta.load_equilibrium_noise_games(exp_path)
    fl = eq.flags_noise(g, opt["agents"], opt["tol"])
    cols = {"noise_prob": g["noise_prob"]}
    for f in ta.NOISE_INT + ta.NOISE_FLOAT + ta.NOISE_WEIGHTED:
        if f in g:
            cols[f] = g[f][int(agent)]
    cols["br_all"] = fl["br_all"][int(agent)]
    if "br_w" in fl:
        cols["br_w"] = fl["br_w"][int(agent)]
    cols["perfect"] = fl["perfect"]
    n = g["noise_prob"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def greedy_attractor_summary(exp_path):
    """A run's attractor analysis in tuple form (training.greedy_attractors, any mix of QTable / Reinforce / ActorCritic
    agents): greedy_attractors.json's summary as a DataFrame with attractor_summary's columns, delta_start_mean (the
    profit gain in expectation over the start weights, by default a start drawn uniformly over action profiles -- not
    the environment's reset distribution) in place of delta_reset_mean, plus no_start, n_states (= T), Nash and
    Cartel."""
    desc = _load_json(exp_path, "greedy_attractors.json")
    df = pandas.DataFrame(desc["summary"])
    df["n_states"] = int(desc["n_states"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def greedy_attractor_games(exp_path):
    """Per-game results of training.greedy_attractors, one row per game indexed by its GLOBAL id: start (the training
    tuple, -1 = none), n_attr, mu_max, n_cycle_states, rep_x0, mu_x0, slot_x0, per kept slot k rep_<k>, lam_<k>,
    basin_<k>, delta_<k> (its profit gain, NaN past n_attr) and mass_<k>, and delta_train, delta_start, mass_other."""
    from th_rl_amd import attractors as at, tuple_analysis as ta
    _run_dirs(exp_path, "gattr_games.npy", "attractor analysis in tuple form", "greedy_attractors", shards=False)
    desc = _load_json(exp_path, "greedy_attractors.json")
    off = _game_offset(exp_path, exp_path)
    g = ta.load_attractor_games(exp_path)
    gn = ta.attractor_gains(g, desc["nash"], desc["cartel"])
    cols = {"start": g["start"]}
    cols.update({f: g[f] for f in at.GAME_INT})
    for k in range(g["rep"].shape[0]):
        cols.update({"rep_%d" % k: g["rep"][k], "lam_%d" % k: g["lam"][k], "basin_%d" % k: g["basin"][k]})
        cols["delta_%d" % k] = numpy.where(g["rep"][k] >= 0, at.profit_gain(g["cycle_reward"][k], desc["nash"], desc["cartel"]),
                                           numpy.nan)
        if "start_mass" in g:
            cols["mass_%d" % k] = g["start_mass"][k]
    cols["delta_train"] = gn["train"]
    if gn["start"] is not None:
        cols["delta_start"] = gn["start"]
        cols["mass_other"] = g["start_mass_other"]
    n = g["n_attr"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def greedy_stationary_summary(exp_path):
    """A run's stationary analysis in tuple form (training.greedy_stationary: greedy play under demand noise for any mix
    of QTable / Reinforce / ActorCritic agents): greedy_stationary.json's summary as a DataFrame with
    stationary_summary's columns plus n_switch_max, unresolved_mean, unresolved_max (the share of the price axis on which
    a network's sampled strategy may differ from the true one), T, n_cells, Nash and Cartel."""
    desc = _load_json(exp_path, "greedy_stationary.json")
    df = pandas.DataFrame(desc["summary"])
    df["T"], df["n_cells"] = int(desc["T"]), int(desc["n_cells"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def greedy_stationary_games(exp_path):
    """Per-game results of training.greedy_stationary, one row per game indexed by its GLOBAL id: iters, change, mass,
    noise_prob, price, n_switch, unresolved, reward_<i>, action_<i>, delta_noise (against the noise-free Nash / Cartel)
    and, from the training state, start (the tuple played there)."""
    from th_rl_amd import stationary as sn, tuple_stationary as ts
    _run_dirs(exp_path, "gstat_iters.npy", "stationary analysis in tuple form", "greedy_stationary", shards=False)
    desc = _load_json(exp_path, "greedy_stationary.json")
    off = _game_offset(exp_path, exp_path)
    g = ts.load_games(exp_path)
    cols = {"iters": g["iters"], "change": g["change"], "mass": g["mass"], "noise_prob": g["noise_prob"],
            "price": g["stat_price"], "n_switch": g["n_switch"], "unresolved": g["unresolved"]}
    for i in range(g["stat_reward"].shape[0]):
        cols["reward_%d" % i], cols["action_%d" % i] = g["stat_reward"][i], g["stat_action"][i]
    cols["delta_noise"] = sn.profit_gain(g["stat_reward"], desc["nash"], desc["cartel"])
    if "start" in g:
        cols["start"] = g["start"]
    n = g["iters"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def sampled_play_summary(exp_path):
    """A run's sampled-play analysis (training.sampled_play: the exact long-run profit of the stochastic policies the
    agents were trained with, for any mix of QTable / Reinforce / ActorCritic agents): sampled_play.json's summary as a
    DataFrame, one row per group: games, converged, iters_*, delta_sampled_* (the profit gain of sampled play),
    agree_mean (the share of steps on which every agent plays its greedy action), price_mean; where greedy_cycles ran in
    the same experiment also delta_greedy_mean and randomness_cost_mean = delta_greedy - delta_sampled; plus T,
    n_prices, Nash and Cartel.  Under demand noise also max_jump_max, n_nodes, and where greedy_stationary analysed the
    same noise delta_greedy_noise_mean and randomness_cost_noise_mean."""
    desc = _load_json(exp_path, "sampled_play.json")
    df = pandas.DataFrame(desc["summary"])
    df["T"], df["n_prices"] = int(desc["T"]), int(desc["n_prices"])
    if "n_nodes" in desc:
        df["n_nodes"] = int(desc["n_nodes"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def sampled_play_games(exp_path):
    """Per-game results of training.sampled_play, one row per game indexed by its GLOBAL id: iters, change, mass, price,
    agree, reward_<i>, action_<i>, epsilon_<i>, delta_sampled (the profit gain, as stationary_games computes
    delta_noise) and, from the training state, start (the tuple played there); under demand noise also noise_prob and
    max_jump."""
    from th_rl_amd import sampled_play as sp
    from th_rl_amd.deviation import profit_gain
    _run_dirs(exp_path, "splay_iters.npy", "sampled-play analysis", "sampled_play", shards=False)
    desc = _load_json(exp_path, "sampled_play.json")
    off = _game_offset(exp_path, exp_path)
    g = sp.load_games(exp_path)
    cols = {"iters": g["iters"], "change": g["change"], "mass": g["mass"], "price": g["samp_price"], "agree": g["agree"]}
    for i in range(g["samp_reward"].shape[0]):
        cols["reward_%d" % i], cols["action_%d" % i] = g["samp_reward"][i], g["samp_action"][i]
        cols["epsilon_%d" % i] = g["epsilon"][i]
    cols["delta_sampled"] = profit_gain(g["samp_reward"], desc["nash"], desc["cartel"])
    for f in ("start", "noise_prob", "max_jump"):
        if f in g:
            cols[f] = g[f]
    n = g["iters"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def sampled_response_summary(exp_path):
    """A run's best responses to sampled play (training.sampled_play.response: how good a reply each agent's stochastic
    policy is to the others'): sampled_response.json's summary as a DataFrame.  One row per (group, agent): games, capped,
    br_all (the share of solved games whose policy loses nothing at any price), loss_all_q25 / q50 / q75, loss_w_mean,
    br_prob_w_mean (the long-run share of steps on which the agent already plays its best response) and exploit_mean, the
    mean of (1 - gamma_i) * gain_w in reward units per period; and one row per group with agent = NaN: solved,
    nashconv_mean (the sum of the agents' exploitabilities) and nashconv_small, the share of games whose NashConv is
    below 1 % of Cartel - Nash; plus T, n_prices, Nash and Cartel."""
    desc = _load_json(exp_path, "sampled_response.json")
    df = pandas.DataFrame(desc["summary"])
    df["T"], df["n_prices"] = int(desc["T"]), int(desc["n_prices"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def sampled_response_games(exp_path):
    """Per-game results of training.sampled_play.response, one row per game indexed by its GLOBAL id, per solved agent i:
    iters_<i>, sweeps_<i>, n_diff_<i>, loss_all_<i>, loss_mean_<i>, loss_w_<i>, gain_w_<i>, v_w_<i>, br_prob_w_<i>,
    gamma_<i>, epsilon_<i>, exploit_<i> = (1 - gamma_i) * gain_w; and nashconv, their sum over the solved agents (NaN
    where one of them is not solved)."""
    from th_rl_amd import sampled_response as sr
    _run_dirs(exp_path, "sresp_counts.npy", "sampled-response analysis", "sampled_play", shards=False)
    desc = _load_json(exp_path, "sampled_response.json")
    off = _game_offset(exp_path, exp_path)
    g = sr.load_games(exp_path)
    ex = sr.exploitability(g)
    cols = {}
    n = g["iters"].shape[1]
    nc = numpy.zeros(n)
    for i in desc["agents"]:
        for f in sr.INT + sr.FLOAT + sr.WEIGHTED + ("gamma", "epsilon"):
            cols["%s_%d" % (f, i)] = g[f][i]
        cols["exploit_%d" % i] = ex[i]
        nc = nc + ex[i]
    cols["nashconv"] = nc
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def sampled_response_noise_summary(exp_path):
    """A run's best responses to sampled play UNDER DEMAND NOISE (training.sampled_play.response with "noise": true):
    sampled_response_noise.json's summary as a DataFrame.  sampled_response_summary's rows, a (group, agent) row with
    diff_nodes_mean (the mean number of node-states where the best reply is not the modal action) beside them and a
    group's own row with max_jump_max (sampled_play's honesty figure of the quadrature); plus T, n_prices, n_nodes, Nash
    and Cartel."""
    desc = _load_json(exp_path, "sampled_response_noise.json")
    df = pandas.DataFrame(desc["summary"])
    df["T"], df["n_prices"], df["n_nodes"] = int(desc["T"]), int(desc["n_prices"]), int(desc["n_nodes"])
    df["Nash"], df["Cartel"] = float(desc["nash"]), float(desc["cartel"])
    return df


def sampled_response_noise_games(exp_path):
    """Per-game results of training.sampled_play.response under demand noise, one row per game indexed by its GLOBAL id:
    noise_prob, per solved agent i iters_<i>, sweeps_<i>, n_diff_prices_<i>, n_diff_nodes_<i>, loss_all_<i>,
    loss_prices_mean_<i>, loss_nodes_mean_<i>, loss_w_<i>, gain_w_<i>, v_w_<i>, br_prob_w_<i>, gamma_<i>, epsilon_<i>,
    exploit_<i> = (1 - gamma_i) * gain_w; and nashconv, their sum over the solved agents (NaN where one of them is not
    solved)."""
    from th_rl_amd import sampled_response as sr
    _run_dirs(exp_path, "srespn_counts.npy", "sampled-response analysis under noise", "sampled_play", shards=False)
    desc = _load_json(exp_path, "sampled_response_noise.json")
    off = _game_offset(exp_path, exp_path)
    g = sr.load_games_noise(exp_path)
    ex = sr.exploitability(g)
    cols = {"noise_prob": g["noise_prob"]}
    n = g["iters"].shape[1]
    nc = numpy.zeros(n)
    for i in desc["agents"]:
        for f in sr.NOISE_INT + sr.NOISE_FLOAT + sr.WEIGHTED + ("gamma", "epsilon"):
            cols["%s_%d" % (f, i)] = g[f][i]
        cols["exploit_%d" % i] = ex[i]
        nc = nc + ex[i]
    cols["nashconv"] = nc
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))


def sampled_deviation_summary(exp_path):
    """A run's deviation test of sampled play (training.sampled_play.deviation: do the others' stochastic policies punish
    a departure, and was it profitable): sampled_deviation.json's summary as a DataFrame with deviation_noise_summary's
    columns, one row per (group, deviator) -- games, solved, deviates, dev_share_mean, unprofitable, gain_mean and gain_q*,
    gain_dev_mean, low_mean, returned, ret_step_mean, dist_mean -- plus T and n_prices.  The expected response curves of a
    run that also has training.group_stats are the per-group statistics of prefix "sdev<d>":
    group_quantiles(exp_path, group, "total", prefix="sdev0"), one row per period after the shock."""
    if not os.path.isfile(os.path.join(exp_path, "sampled_deviation.json")):
        raise KeyError("no deviation test of sampled play (sampled_deviation.json) under %s (training.sampled_play.deviation)"
                       % exp_path)
    desc = _load_json(exp_path, "sampled_deviation.json")
    df = pandas.DataFrame(desc["summary"])
    df["T"], df["n_prices"] = int(desc["T"]), int(desc["n_prices"])
    return df


def sampled_deviation_games(exp_path, deviator=0):
    """Per-game results of the deviation test of sampled play for `deviator`, one row per game indexed by its GLOBAL id:
    stat_iters, gamma, base_price, dev_share, gain, gain_dev, low, dist, mass, low_step, ret_step, base_reward_<i> /
    base_action_<i> / epsilon_<i> and solved."""
    return _sampled_deviation_games(exp_path, deviator, "sdev", "sampled_deviation.json", "deviation test of sampled play",
                                    "sampled_play.deviation", ())


def sampled_deviation_noise_summary(exp_path):
    """A run's deviation test of sampled play UNDER DEMAND NOISE (training.sampled_play.deviation with "noise": true beside
    sampled_play's "noise"): sampled_deviation_noise.json's summary as a DataFrame with sampled_deviation_summary's
    columns plus max_jump_max, and T, n_prices, n_nodes and resolution.  The expected response curves of a run that also
    has training.group_stats are the per-group statistics of prefix "sdevn<d>"."""
    if not os.path.isfile(os.path.join(exp_path, "sampled_deviation_noise.json")):
        raise KeyError("no deviation test of sampled play under demand noise (sampled_deviation_noise.json) under %s "
                       "(training.sampled_play.deviation with \"noise\")" % exp_path)
    desc = _load_json(exp_path, "sampled_deviation_noise.json")
    df = pandas.DataFrame(desc["summary"])
    for f in ("T", "n_prices", "n_nodes", "resolution"):
        df[f] = int(desc[f])
    return df


def sampled_deviation_noise_games(exp_path, deviator=0):
    """sampled_deviation_games' columns for the test under demand noise, plus noise_prob and max_jump."""
    return _sampled_deviation_games(exp_path, deviator, "sdevn", "sampled_deviation_noise.json",
                                    "deviation test of sampled play under demand noise", "sampled_play.deviation with \"noise\"",
                                    ("noise_prob", "max_jump"))


def _sampled_deviation_games(exp_path, deviator, prefix, json_name, what, key, more):
    from th_rl_amd import sampled_deviation as sd
    _run_dirs(exp_path, prefix + "_stat_iters.npy", what, key, shards=False)
    desc = _load_json(exp_path, json_name)
    if int(deviator) not in desc["options"]["agents"]:
        raise KeyError("deviator %d was not analysed (agents %s)" % (int(deviator), desc["options"]["agents"]))
    off = _game_offset(exp_path, exp_path)
    g = sd.load_games(exp_path, int(deviator), prefix)
    cols = {f: g[f] for f in ("stat_iters", "gamma") + tuple(more)}
    cols.update({f: g[f] for f in sd.FLOAT + sd.INT})
    for i in range(g["base_reward"].shape[0]):
        cols["base_reward_%d" % i] = g["base_reward"][i]
        cols["base_action_%d" % i] = g["base_action"][i]
        cols["epsilon_%d" % i] = g["epsilon"][i]
    cols["solved"] = g["solved"]
    n = g["stat_iters"].shape[0]
    return pandas.DataFrame(cols, index=pandas.RangeIndex(off, off + n, name="game"))
