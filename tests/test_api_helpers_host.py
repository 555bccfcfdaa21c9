"""The shared planning code of the analysis entry points under host sanitizers: tests/api_helpers_check.cpp calls the
LDS layout functions of the analysis headers and the pure helpers of thrl_api_analysis.hip (tuple strides, table rows,
the staged window, the reach tables, grid_for, the check helpers) on shapes up to the limits of include/thrl.h and
asserts alignment, bounds and budgets.  It is built here as a stand-alone host program with
-fsanitize=address,undefined and run as a process of its own; it makes no HIP call and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "th_rl_amd")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on hosts without a GPU")
def test_layouts_and_helpers_under_address_and_undefined_sanitizers(tmp_path):
    from th_rl_amd import build
    build.build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "api_helpers_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "api_helpers_check.cpp"), "-o", exe,
                           "-L" + PKG, "-lthrl_hip", "-Wl,-rpath," + PKG])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "api helpers ok" in p.stdout, p.stdout[-4000:]
