"""k_sp_chain on the host under sanitizers: writes mirror-generated inputs and outputs (tests/sampled_mirror.py) for five
cases -- the smallest shape (2 x 2 QTable, T = 4) from the uniform start with per-game epsilon and from start tuples with
scalar epsilon, three agents of mixed kinds (T = 12) from start tuples, and the heaviest working set thrl_sampled_chain
accepts (QTable 30 x Reinforce 32, T = D = 960) with both starts -- compiles profiles/sampled_host_check.cpp, the
kernel's own source as 256 host threads with barriers, with -fsanitize=address,undefined (with --tsan: -fsanitize=thread,
which watches the barriers for a race between the block's threads) and runs it on each.  No GPU.

    python profiles/sampled_host_check.py [--tsan] [--dir /tmp/sampled_host_check]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sampled_mirror as SPM                                      # noqa: E402
from th_rl_amd import sampled_play as sp                          # noqa: E402


def write_case(path, config, n_games, max_iters, seed, use_start, eps_per_game, n_blocks):
    tabs = sp.tables(config)
    rs = np.random.RandomState(seed)
    N, T, D = len(tabs["kinds"]), tabs["n_tuples"], tabs["n_prices"]
    probs = {}
    for i, k in enumerate(tabs["kinds"]):
        if k != "QTable":
            w = SPM.random_weights(rs, n_games, int(tabs["n_actions"][i]), k, tabs["price"].min(), tabs["price"].max())
            probs[i] = SPM.net_probs(w, int(tabs["n_actions"][i]), tabs["dprice"])
    pol = SPM.greedy_of(probs, tabs, rs, n_games)
    eps = rs.uniform(0, 0.2, (N, n_games))
    start = rs.randint(0, T, n_games).astype(np.int32)
    if n_games > 3:
        eps[0, 1], start[2] = np.nan, T
    e = eps if eps_per_game else eps[:, 0].copy()
    ref = SPM.analyse(tabs, probs, pol, e, start=start if use_start else None, tol=1e-12, max_iters=max_iters)
    kind = np.zeros(8, np.int32)
    nact = np.zeros(8, np.int32)
    kind[:N] = [{"QTable": 0, "Reinforce": 1, "ActorCritic": 2}[k] for k in tabs["kinds"]]
    nact[:N] = tabs["n_actions"]
    e8 = np.zeros(8)
    if not eps_per_game:
        e8[:N] = e
    with open(path, "wb") as f:
        np.array([n_games, N, T, D, max_iters, int(use_start), int(eps_per_game), n_blocks], np.int32).tofile(f)
        kind.tofile(f), nact.tofile(f), e8.tofile(f), np.array([1e-12]).tofile(f)
        if eps_per_game:
            np.ascontiguousarray(eps).tofile(f)
        start.tofile(f)
        for i in range(N):
            if i in probs:
                np.ascontiguousarray(probs[i], np.float32).tofile(f)
        np.ascontiguousarray(pol, np.uint16).tofile(f)
        for name, dt in (("grp_first", np.int32), ("grp_perm", np.int32), ("reward", np.float64), ("scaled", np.float64),
                         ("price", np.float64)):
            np.ascontiguousarray(tabs[name], dt).tofile(f)
        ref["iters"].astype(np.int32).tofile(f)
        for name in ("change", "mass", "samp_reward", "samp_action", "samp_price", "agree", "pi"):
            np.ascontiguousarray(ref[name], np.float64).tofile(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/sampled_host_check")
    ap.add_argument("--tsan", action="store_true", help="build with the thread sanitizer in place of address + undefined")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    exe = os.path.join(a.dir, "sampled_host_check_tsan" if a.tsan else "sampled_host_check")
    san = ["-fsanitize=thread"] if a.tsan else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off"] + san
                          + ["-DTHRL_SP_HOST_BUILD", "-I", os.path.join(ROOT, "th_rl_amd", "csrc"),
                             os.path.join(HERE, "sampled_host_check.cpp"), "-o", exe, "-lpthread"])
    big = {"agents": [dict(SPM.AG, actions=30), dict(SPM.RF, actions=32)], "environment": dict(SPM.ENV)}
    cases = [("T=4 uniform", SPM.QQ, 9, 40, 1, False, True, 2), ("T=4 tuples", SPM.QQ, 9, 40, 2, True, False, 3),
             ("T=12 three agents", SPM.QRA, 7, 24, 3, True, True, 2), ("T=960 uniform", big, 2, 3, 4, False, False, 1),
             ("T=960 tuples", big, 3, 3, 5, True, True, 2)]
    rc = 0
    for k, (what, config, g, it, seed, st, eg, nb) in enumerate(cases):
        path = os.path.join(a.dir, "case%d.bin" % k)
        write_case(path, config, g, it, seed, st, eg, nb)
        print(what)
        rc |= subprocess.call([exe, path])
    sys.exit(rc)


if __name__ == "__main__":
    main()
