"""k_spn_chain and k_spn_jump on the host under sanitizers: writes mirror-generated inputs and outputs
(tests/sampled_noise_mirror.py) for the smallest shape (2 x 2 QTable, T = 4, three nodes) from every start, three agents of
mixed kinds (T = 12, the variant for more than two agents), two networks with the node count on the tile's edges
(TILE, TILE + 1, 2 TILE - 1, 2 TILE + 1 nodes, the node rows moved 0 to 3 floats off a 16-byte boundary) and the heaviest
working set thrl_sampled_noise_chain accepts at the default resolution (QTable 27 x Reinforce 32, T = 864, 1,121 nodes);
compiles profiles/sampled_noise_host_check.cpp, the kernels' own source as 256 host threads with barriers, with
-fsanitize=address,undefined (with --tsan: -fsanitize=thread, which watches the barriers for a race between the block's
threads) and runs it on each as a program of its own.  No GPU.

    python profiles/sampled_noise_host_check.py [--tsan] [--dir /tmp/sampled_noise_host_check]
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

import sampled_noise_mirror as SNM                                # noqa: E402
from th_rl_amd import sampled_play as sp                          # noqa: E402

START = {"uniform": 0, "tuples": 1, "reset": 2}


def write_case(path, config, resolution, n_games, max_iters, seed, start, per_game, n_blocks, shift):
    x = SNM.make_inputs(config, resolution, n_games, seed)
    tabs = x["tabs"]
    N, T, D, Jn, W = len(tabs["kinds"]), tabs["n_tuples"], tabs["n_prices"], tabs["n_nodes"], tabs["band_w"]
    eps, p, st = x["eps"], x["noise_prob"], x["start"]
    if n_games > 3:
        eps[0, 1], st[2], p[3] = np.nan, T, 1.5
        p[0] = 0.0
    e = eps if per_game else eps[:, 0].copy()
    pp = p if per_game else float(p[n_games - 1])
    ref = SNM.analyse(tabs, x["probs"], x["dpolicy"], x["nprobs"], x["npolicy"], e, pp,
                      start={"uniform": None, "tuples": st, "reset": SNM.RESET}[start], tol=1e-12, max_iters=max_iters)
    kind = np.zeros(8, np.int32)
    nact = np.zeros(8, np.int32)
    kind[:N] = [{"QTable": 0, "Reinforce": 1, "ActorCritic": 2}[k] for k in tabs["kinds"]]
    nact[:N] = tabs["n_actions"]
    e8 = np.zeros(8)
    if not per_game:
        e8[:N] = e
    with open(path, "wb") as f:
        np.array([n_games, N, T, D, Jn, W, max_iters, START[start], int(per_game), int(per_game), n_blocks, shift],
                 np.int32).tofile(f)
        kind.tofile(f), nact.tofile(f), e8.tofile(f), np.array([1e-12, 0.0 if per_game else pp]).tofile(f)
        if per_game:
            np.ascontiguousarray(eps).tofile(f)
            np.ascontiguousarray(p).tofile(f)
        st.tofile(f)
        for src in (x["probs"], x["nprobs"]):
            for i in range(N):
                if i in src:
                    np.ascontiguousarray(src[i], np.float32).tofile(f)
        np.ascontiguousarray(x["dpolicy"], np.uint16).tofile(f)
        np.ascontiguousarray(x["npolicy"], np.uint16).tofile(f)
        for name, dt in (("grp_first", np.int32), ("grp_perm", np.int32), ("reward", np.float64), ("scaled", np.float64),
                         ("price", np.float64), ("band_lo", np.int32), ("band", np.float64), ("noise_price", np.float64),
                         ("noise_reward", np.float64), ("node_w", np.float64)):
            np.ascontiguousarray(tabs[name], dt).tofile(f)
        ref["iters"].astype(np.int32).tofile(f)
        for name in ("change", "mass", "samp_reward", "samp_action", "samp_price", "agree", "pi", "max_jump"):
            np.ascontiguousarray(ref[name], np.float64).tofile(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/sampled_noise_host_check")
    ap.add_argument("--tsan", action="store_true", help="build with the thread sanitizer in place of address + undefined")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    exe = os.path.join(a.dir, "sampled_noise_host_check_tsan" if a.tsan else "sampled_noise_host_check")
    san = ["-fsanitize=thread"] if a.tsan else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off"] + san
                          + ["-DTHRL_SP_HOST_BUILD", "-I", os.path.join(ROOT, "th_rl_amd", "csrc"),
                             os.path.join(HERE, "sampled_noise_host_check.cpp"), "-o", exe, "-lpthread"])
    qq = SNM.two_agents("QTable", 2, "QTable", 2)
    rr = SNM.two_agents("Reinforce", 5, "Reinforce", 5)
    big = SNM.two_agents("QTable", 27, "Reinforce", 32)
    assert sp.working_set(big, resolution=1024)["fits"]
    assert not sp.working_set(SNM.two_agents("QTable", 28, "Reinforce", 32), resolution=1024)["fits"]
    tile = sp.TILE
    # (what, config, resolution, games, max_iters, seed, start, per-game eps and noise_prob, blocks, shift)
    cases = [("T=4 uniform", qq, 0, 9, 40, 1, "uniform", True, 2, 0), ("T=4 tuples", qq, 0, 9, 40, 2, "tuples", False, 3, 0),
             ("T=4 reset", qq, 0, 9, 40, 3, "reset", True, 2, 0),
             ("T=12 three agents, tuples", SNM.three_agents(), 8, 7, 24, 4, "tuples", True, 2, 1),
             ("T=12 three agents, reset, no atom", SNM.three_agents([0.0, 0.2]), 8, 7, 24, 5, "reset", False, 2, 3)]
    for k, jn in enumerate((tile, tile + 1, 2 * tile - 1, 2 * tile + 1)):
        cases.append(("T=25 two networks, %d nodes" % jn, rr, jn - 1, 5, 6, 10 + k, ("uniform", "tuples", "reset", "reset")[k],
                      k % 2 == 0, 2, k))
    cases += [("T=864 uniform", big, 1024, 2, 2, 20, "uniform", False, 1, 2), ("T=864 reset", big, 1024, 3, 2, 21, "reset", True, 2, 0)]
    rc = 0
    for k, (what, config, res, g, it, seed, st, pg, nb, shift) in enumerate(cases):
        path = os.path.join(a.dir, "case%d.bin" % k)
        write_case(path, config, res, g, it, seed, st, pg, nb, shift)
        print(what, flush=True)
        rc |= subprocess.call([exe, path])
    sys.exit(rc)


if __name__ == "__main__":
    main()
