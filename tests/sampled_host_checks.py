"""What the host tests of the four newer calls on sampled play (test_sampled_response_host, test_sampled_response_noise_host,
test_sampled_deviation_host, test_sampled_deviation_noise_host) had word for word: the build of a kernel's stand-alone check
program, and the comparison of a ctypes args struct with the public header as the C compiler lays it out."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(source, path, sanitizer):
    """tests/<source>, a kernel's .hip compiled as host code with its own main, into the program at path."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-ffp-contract=off",
                           "-DTHRL_SP_HOST_BUILD", "-fno-omit-frame-pointer"] + sanitizer
                          + [os.path.join(ROOT, "tests", source), "-o", path, "-lpthread"])


def assert_struct_matches_header(struct, cname, header, constants):
    """sizeof(cname), the header's value of every (name, value) of constants and the offset of every field of struct, as gcc
    sees include/<header>, against ctypes' and the values given."""
    fields = [n for n, _ in struct._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu%s",sizeof(%s)%s);\n'
           % (header, " %d" * len(constants), cname, "".join("," + n for n, _ in constants)))
    for f in fields:
        src += 'printf(" %%zu",offsetof(%s,%s));\n' % (cname, f)
    src += 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [ctypes.sizeof(struct)] + [v for _, v in constants] + [getattr(struct, f).offset for f in fields]
