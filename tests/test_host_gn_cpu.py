"""CPU: the host Gauss-Newton kit of the small factors (csrc/ccal_host_gn.hpp: chol_factor / chol_solve, huber_weight, gn_decide)
through a plain C++ program (tests/cpp/test_host_gn.cpp) under the host's address and undefined-behaviour sanitizers: exact integer
Cholesky cases for n = 1, 6, 9, the pivots that must be refused, convert's fixed mask, the Huber weight on both sides of delta^2, and
the stop rule over a hand-worked table against a verbatim copy of the ladder the two loops carried before."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_host_gn_kit(tmp_path):
    exe = str(tmp_path / "test_host_gn")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_host_gn.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "GN-OK 28" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
