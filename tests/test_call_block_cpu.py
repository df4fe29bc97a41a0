"""CPU: the slice plan of the one-shot calls' device block (csrc/ccal_call.hpp: CallPlan) through a plain C++ program
(tests/cpp/test_call_plan.cpp) under the host's address and undefined-behaviour sanitizers: every slice on a 256-byte boundary, in
declaration order, none overlapping, an absent optional slice of zero bytes, the total the sum of the rounded sizes - and the layout of
ccal_refine_poses_batch for 5 problems with 195 points as large as the byte formulas of that entry point say, worked out here.  The
same program holds the guarded layout of the tests' CCAL_TEST_GUARD_SLICES mode (tests/test_gpu_guard.py): a guard in front, slices
on 256-byte boundaries and in order, a guard of at least 256 bytes from every present slice's exact end, none for an absent slice, the
total the sum - and with gap 0 the numbers above."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _up256(b):
    return (b + 255) & ~255


def _refine_block_bytes(n_prob, n_tot, err_out):
    # offsets | points | image points | poses, cost0, cost | errors | status, iterations, counts
    b_off, b_xyz, b_uv = _up256((n_prob + 1) * 8), _up256((n_tot + 1) * 24), _up256((n_tot + 1) * 16)
    b_res, b_err, b_int = _up256(n_prob * 8 * 8), (_up256((n_tot + 1) * 8) if err_out else 0), _up256(n_prob * 3 * 4)
    return b_off + b_xyz + b_uv + b_res + b_err + b_int


def test_call_plan_layout(tmp_path):
    exe = str(tmp_path / "test_call_plan")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_call_plan.cpp"), "-o", exe])
    with_err, without = _refine_block_bytes(5, 195, True), _refine_block_bytes(5, 195, False)
    assert (with_err, without) == (11008, 9216)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe, str(with_err), str(without)], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and f"PLAN-OK {with_err} {without}" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
