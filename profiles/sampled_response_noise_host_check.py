"""k_srn_response on the host under sanitizers: writes mirror-generated inputs and outputs
(tests/sampled_response_noise_mirror.host_cases: the smallest shape with per-game epsilon, gamma and noise and an
unsolved game of each kind, a capped agent, three agents of mixed kinds with a subset solved, scalars, D < T, and the
shipped shape T = D = 441 at resolution 16 and gamma 0.5), compiles tests/sampled_response_noise_check.cpp, the kernel's
own source as 256 host threads with barriers, with -fsanitize=address,undefined (with --tsan: -fsanitize=thread, which watches the barriers
for a race between the block's threads) and runs it on each.  No GPU.

    python profiles/sampled_response_noise_host_check.py [--tsan] [--dir /tmp/sampled_response_noise_host_check]
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sampled_response_noise_mirror as SRNM                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/sampled_response_noise_host_check")
    ap.add_argument("--tsan", action="store_true", help="build with the thread sanitizer in place of address + undefined")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    exe = os.path.join(a.dir, "sampled_response_noise_check_tsan" if a.tsan else "sampled_response_noise_check")
    san = ["-fsanitize=thread"] if a.tsan else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-ffp-contract=off",
                           "-DTHRL_SP_HOST_BUILD", "-fno-omit-frame-pointer"] + san
                          + [os.path.join(ROOT, "tests", "sampled_response_noise_check.cpp"), "-o", exe, "-lpthread"])
    rc = 0
    for k, (what, kw, blocks) in enumerate(SRNM.host_cases()):
        path = os.path.join(a.dir, "case%d.bin" % k)
        SRNM.write_case(path, kw, SRNM.analyse(**kw), blocks)
        print(what, flush=True)
        rc |= subprocess.call([exe, path], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    sys.exit(rc)


if __name__ == "__main__":
    main()
