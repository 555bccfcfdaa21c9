"""The cycle search the four greedy-walk kernels share (th_rl_amd/csrc/thrl_walk_dev.h) under host sanitizers:
tests/walk_dev_check.cpp runs it against a plain first-repeat search over every map on 1 .. 5 states, every start, every
horizon from 1 to n + 2 and both values of want_s, with the state as one int and as a row tuple (N = 2 of MAXN = 2,
N = 3 of MAXN = 8).  It is built here as a stand-alone host program with -fsanitize=address,undefined and run as a
process of its own; it makes no HIP call and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
def test_cycle_search_against_first_repeat_under_address_and_undefined_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "walk_dev_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "walk_dev_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "walk dev ok: 3413 maps" in p.stdout, p.stdout[-4000:]
