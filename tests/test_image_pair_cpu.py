"""CPU: the argument check that ccal_photo_apply_dev and ccal_normalize_dev share for their source / destination pair of image batches
(csrc/ccal_image_plan.hpp: image_pair_check; grey_batch_bad, which GreyBatch::bad of the other image stages calls), through a plain
C++ program (tests/cpp/test_image_pair.cpp) under the host's address and undefined-behaviour sanitizers: every message and their
order, n_img == 0 with NULL pointers, blocks that touch against blocks that share a byte for all four u8 / u16 pairs, and an image
of more than 2^31 - 1 pixels.  tests/test_gpu_photo.py and tests/test_gpu_normalize.py hold the entry points to the same messages."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_the_pair_check_gives_each_message_in_its_order(tmp_path):
    exe = str(tmp_path / "test_image_pair")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_image_pair.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    # the program counts what it checked: 4 good calls, 11 single messages, 5 on the pixel count, 12 on the order, 8 on n_img == 0,
    # 48 + 6 on overlap, 2 on the single-batch check
    assert out.stdout.strip() == "OK 96", out.stdout[-2000:]
