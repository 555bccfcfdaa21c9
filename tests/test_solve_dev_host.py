"""The host-callable pieces the six state-graph kernels share (th_rl_amd/csrc/thrl_solve_dev.h) under host sanitizers:
tests/solve_dev_check.cpp runs the first-visit walk against find_cycle and the doubling steps against step-by-step walks
over every map on 1 .. 5 states, the band range against a count (both ends of int32 included), the round count D against
its definition, and the relative loss, margin, blend, first maximum and attractor key on chosen values.  It is built here
as a stand-alone host program with -fsanitize=address,undefined and run as a process of its own; it makes no HIP call and
needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
def test_shared_solve_pieces_against_brute_force_under_address_and_undefined_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "solve_dev_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "solve_dev_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "solve dev ok: 3413 maps" in p.stdout, p.stdout[-4000:]
