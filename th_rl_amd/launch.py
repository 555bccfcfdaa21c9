"""Seed-sharded multi-GPU training of one config on one node.

    python -m th_rl_amd.launch --config cfg.json --out runs/exp --gpus 8

One process per GPU (torch.multiprocessing spawn).  Games are independent, so rank r simply trains
the contiguous block of global game ids `sharding.shard_range(n_games, r, world)` with the matching
`game_offset`; the Philox streams are keyed by the global game id, so every game's result is the
same as in a single-GPU run of all games.  There is NO data-path collective: the only cross-rank
step is the weighted mean of the [epochs, N] logs over a gloo (CPU) group.  Outputs: rank 0 writes
the reference's artefacts for global game 0 and the merged log.csv into --out; every rank writes its
shard checkpoint `--out/shard<r>/batch.pt`, and with training.game_logs its shard's per-game logs
(`game_rewards.npy`, `game_actions.npy`, `game_ids.npy` with global ids; utils.game_log finds a game there).
With training.group_stats, group ids come from the global sweep (or training.groups) before the cut, every shard
writes its raw per-group statistics with histograms, and rank 0 merges them exactly into the top-level
groups.json / group_*.npy (merge_group_stats), the dev<d>_* and xplay_* statistics of training.deviation and
training.crossplay among them, and with group_stats.smooth the group_smooth_*.npy of the smoothed curves: every shard
keeps the smoothing state of its own games, so the merged statistics are the single-process ones bit for bit.  Every analysis of analysis.REGISTRY with a merge (convergence, deviation, equilibrium,
crossplay, attractors, stationary) is written per shard, and rank 0 concatenates the shards' per-game arrays in global
game order and writes the top-level <key>.json and .npy files (merge_analysis); the others are refused
(check_launch_config).  With training.crossplay every shard draws its partners INSIDE the shard (the tables of other
ranks are not fetched, so a sharded run's pairings are not the unsharded run's) and saves the seats as global game ids.
A convergence stop counts the games of every rank (the trainer all-reduces over the gloo group), so all ranks stop at
the same episode.
"""
import argparse
import json
import os
import socket

import numpy
import pandas


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def shard_training(config, rank, world):
    """The `training` block rank `rank` of `world` runs: its contiguous block of global game ids, with
    everything that must not depend on the shard size pinned to what the unsharded run would use --
    the table dtype (train_one's default is float64 for ONE game, float32 otherwise) and the Philox
    initialisation keyed by (seed, global game id) (train_one's one-game default draws the tables
    from numpy's global RNG instead).  Pure host logic (no GPU): tests/test_host_cpu.py."""
    from th_rl_amd import analysis
    from th_rl_amd.sharding import shard_range
    training = dict(config.get("training", {}))
    total = int(training.get("n_games", world))
    if training.get("seed") is None:
        raise SystemExit("th_rl_amd.launch needs an explicit training.seed (all shards must share it)")
    offset, n_local = shard_range(total, rank, world)
    if n_local < 1:
        raise ValueError("rank %d of %d has no games (n_games=%d): launch() clamps the world first" % (rank, world, total))
    training.setdefault("dtype", None)
    if not training["dtype"]:
        training["dtype"] = "float64" if total == 1 else "float32"
    training.update(n_games=n_local, game_offset=int(training.get("game_offset", 0)) + offset,
                    philox_init=(total > 1) or bool(training.get("philox_init", False)), checkpoint=True)
    gs = training.get("group_stats")
    if gs is not None and gs is not False:
        # group ids from the GLOBAL sweep / groups, so they agree across ranks; the largest group of the whole run
        # sizes the fixed-point scales (so the shards' sums add); histograms let rank 0 merge the quantiles
        from th_rl_amd.group_stats import assign_groups, parse_options
        ids, n_groups, _ = assign_groups(total, sweep=training.get("sweep"), groups=training.get("groups"),
                                         n_groups=training.get("n_groups"))
        opt = dict(parse_options(gs))
        opt.update(histograms=True, n_max=int(numpy.bincount(ids, minlength=n_groups).max()))
        training.update(group_stats=opt, groups=ids[offset:offset + n_local].tolist(), n_groups=int(n_groups))
    if any(analysis.enabled(training, a.key) for a in analysis.REGISTRY if a.merge) and (gs is None or gs is False):
        # the per-group summaries of each shard's <key>.json use the global group ids too
        from th_rl_amd.group_stats import assign_groups
        ids, n_groups, _ = assign_groups(total, sweep=training.get("sweep"), groups=training.get("groups"),
                                         n_groups=training.get("n_groups"))
        training.update(groups=ids[offset:offset + n_local].tolist(), n_groups=int(n_groups))
    sweep = training.get("sweep")
    if sweep:        # slice the per-game arrays to this shard
        def cut(v):
            a = numpy.asarray(v)
            return a[..., offset:offset + n_local].tolist()
        training["sweep"] = {k: cut(v) for k, v in sweep.items()}
    game_logs = training.get("game_logs")
    if game_logs is not None and game_logs is not True and game_logs is not False:
        # a list of global game ids: the ones in this shard (each rank writes its own game_*.npy)
        lo = training["game_offset"]
        training["game_logs"] = [int(i) for i in game_logs if lo <= int(i) < lo + n_local]
    return training, offset, n_local


def merge_group_stats(config, out, world):
    """Rank 0: the top-level groups.json and group_*.npy (greedy_*.npy) of a sharded run from the shards' raw
    outputs, combined exactly (group_stats.merge)."""
    from th_rl_amd import trainer
    from th_rl_amd.group_stats import GroupSpec, merge, parse_options, save_json
    training = config.get("training", {})
    total = int(training.get("n_games", world))
    opt = parse_options(training["group_stats"])
    spec = GroupSpec.from_config(config, total, opt, sweep=training.get("sweep"), groups=training.get("groups"),
                                 n_groups=training.get("n_groups"))
    desc = spec.describe()
    save_json(os.path.join(out, "groups.json"), desc)
    shards = [os.path.join(out, "shard%d" % r) for r in range(world)]
    prefixes = ["group"] + (["greedy"] if opt["greedy_iters"] > 0 else [])
    if opt.get("smooth") is not None:       # every shard smoothed its own games (they are disjoint): merged like the raw ones
        prefixes.append("group_smooth")
    dv = training.get("deviation")
    if dv is not None and dv is not False:
        from th_rl_amd.deviation import parse_options as deviation_options
        dvo = deviation_options(dv, config)
        prefixes += ["dev%d" % d for d in dvo["agents"]]
        if dvo.get("noise"):       # the response curves of the test under demand noise
            prefixes += ["devn%d" % d for d in dvo["agents"]]
    xp = training.get("crossplay")
    if xp is not None and xp is not False:
        from th_rl_amd.crossplay import parse_options as crossplay_options
        if crossplay_options(xp, config)["steps"] > 0:
            prefixes.append("xplay")
    for prefix in prefixes:
        parts = []
        for d in shards:
            ld = lambda f: numpy.load(os.path.join(d, "%s_%s.npy" % (prefix, f)), mmap_mode="r")
            # ~key(min) / key(max) of the shard's exact extremes: the same keys the kernel stored
            parts.append({"hist": ld("hist"), "sums": ld("sums"), "minmax": _keys(ld("min"), ld("max"))})
        trainer.save_group_stats(out, prefix, merge(parts), spec, opt["histograms"])


def merge_analysis(key, config, out, world):
    """Rank 0: the top-level <key>.json and per-game .npy files of a sharded run for one analysis of analysis.REGISTRY
    that has a merge: the shards' per-game arrays concatenated in global game order and summarised as one run, by the
    analysis module's merged() hook.  What only a run knows (the record's `copy` keys, e.g. horizon_used, or tables
    when the run tracks convergence) is taken from shard 0's JSON.  In cross-play every shard drew its partners INSIDE
    the shard, so the merged pairings are not those of the unsharded run (crossplay.merged)."""
    from th_rl_amd import analysis
    from th_rl_amd.group_stats import assign_groups
    a = analysis.record(key)
    if not a.merge:
        raise ValueError("training.%s has no sharded merge" % key)
    mod = analysis.module_of(a)
    training = config.get("training", {})
    total = int(training.get("n_games", world))
    opt = getattr(mod, a.parse)(training[key], config)
    ids, n_groups, _ = assign_groups(total, sweep=training.get("sweep"), groups=training.get("groups"),
                                     n_groups=training.get("n_groups"))
    shards = [os.path.join(out, "shard%d" % r) for r in range(world)]
    with open(os.path.join(shards[0], key + ".json")) as f:
        first = json.load(f)
    for k in a.copy:
        if k in first["options"]:
            opt[k] = first["options"][k]
    analysis.save_json(os.path.join(out, key + ".json"), mod.merged(shards, out, config, opt, ids, n_groups, first))


def _keys(vmin, vmax):
    from th_rl_amd.group_stats import order_key
    vmin, vmax = numpy.asarray(vmin), numpy.asarray(vmax)
    kmin = numpy.where(numpy.isnan(vmin), numpy.uint64(0), ~order_key(numpy.nan_to_num(vmin)))
    kmax = numpy.where(numpy.isnan(vmax), numpy.uint64(0), order_key(numpy.nan_to_num(vmax)))
    return numpy.stack([kmin, kmax], axis=-1)


def effective_world(config, gpus):
    """Never more ranks than games: an empty shard has nothing to run."""
    total = int(config.get("training", {}).get("n_games", gpus))
    return max(1, min(int(gpus), total))


def _worker(rank, world, port, config, out, devices_available):
    import torch
    import torch.distributed as dist
    from th_rl_amd import analysis, trainer
    from th_rl_amd.sharding import aggregate_logs
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    training, offset, n_local = shard_training(config, rank, world)
    training["device"] = "cuda:%d" % (rank % max(1, devices_available))
    shard_cfg = dict(config, training=training)
    shard_dir = os.path.join(out, "shard%d" % rank)
    os.makedirs(shard_dir, exist_ok=True)
    cpath = os.path.join(shard_dir, "shard_config.json")
    with open(cpath, "w") as f:
        json.dump(shard_cfg, f, indent=3)
    trainer.train_one(shard_dir, cpath)
    log = pandas.read_csv(os.path.join(shard_dir, "log.csv"), header=[0, 1], float_precision="round_trip")
    merged = aggregate_logs(log.to_numpy(dtype="float64"), n_local)
    dist.barrier()
    if rank == 0:
        n = len(config["agents"])
        for i in range(n):      # global game 0 lives in shard 0
            for suffix in (".npy", "_counter.npy", ""):
                src = os.path.join(shard_dir, str(i) + suffix)
                if os.path.exists(src) and os.path.isfile(src):
                    with open(src, "rb") as fi, open(os.path.join(out, str(i) + suffix), "wb") as fo:
                        fo.write(fi.read())
        with open(os.path.join(out, "config.json"), "w") as f:
            json.dump(config, f, indent=3)
        rpd = pandas.DataFrame(data=merged[:, :n], columns=numpy.arange(n))
        apd = pandas.DataFrame(data=merged[:, n:], columns=numpy.arange(n))
        pandas.concat([rpd, apd], axis=1, keys=["rewards", "actions"]).to_csv(os.path.join(out, "log.csv"), index=None)
        if training.get("group_stats"):
            merge_group_stats(config, out, world)
        for a in analysis.REGISTRY:      # in its order: stationary reads what the attractors' merge wrote
            if a.merge and analysis.enabled(training, a.key):
                merge_analysis(a.key, config, out, world)
    dist.destroy_process_group()


def check_launch_config(config):
    """ValueError for a training key that has no sharded form, the records of analysis.REGISTRY without a merge:
    training.greedy_cycles re-seats agents across games and its merge over shards is not built, nor is that of the other
    greedy_* keys and training.sampled_play."""
    from th_rl_amd import analysis
    for key in (a.key for a in analysis.REGISTRY if not a.merge):
        if analysis.enabled(config.get("training", {}), key):
            raise ValueError("training.%s is not available under th_rl_amd.launch (sharded runs are not merged); "
                             "run it through th_rl_amd.main / trainer.train_one on one device" % key)


def launch(configpath, out, gpus=None):
    """Train `configpath` with its games sharded over `gpus` processes (default: all visible GPUs)."""
    import torch
    import torch.multiprocessing as mp
    config = json.load(open(configpath))
    check_launch_config(config)                # before any shard starts
    avail = torch.cuda.device_count()          # device_count() does not initialise the GPU
    if avail < 1:
        from th_rl_amd._lib import ThrlError
        raise ThrlError("th_rl_amd.launch: no GPU visible; there is no CPU fallback")
    world = effective_world(config, int(gpus or avail))     # a shard needs at least one game
    os.makedirs(out, exist_ok=True)
    port = _free_port()
    mp.spawn(_worker, args=(world, port, config, out, avail), nprocs=world, join=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--gpus", type=int, default=None, help="processes to launch (default: visible GPUs)")
    a = ap.parse_args()
    launch(a.config, a.out, a.gpus)


if __name__ == "__main__":
    main()
