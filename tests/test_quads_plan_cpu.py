"""CPU: how ccal_propose_quads_* and ccal_decode_tags_* cut a batch into chunks of whole images (csrc/ccal_image_plan.hpp: one planner,
each stage's byte figures), through a plain C++ program (tests/cpp/test_quads_plan.cpp) under the host's address and
undefined-behaviour sanitizers - and, with it, that the limits tests/test_gpu_quads.py::test_a_batch_cut_into_chunks and
tests/test_gpu_tags.py::test_a_batch_cut_into_chunks set really cut their batches the way those tests say: for the host call and for
the _dev call a chunk of several images (for the quads, one that is not the first)."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quad_ref as ref  # noqa: E402
import tag_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quads_plan") / "test_quads_plan")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_quads_plan.cpp"), "-o", exe])

    def run(on_device, img_bytes, limit, counts, stage="quads"):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        out = subprocess.run([exe, stage, str(int(on_device)), str(img_bytes), str(limit)] + [str(c) for c in counts], env=env,
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
        lines = out.stdout.split("\n")
        # quads: 16 of coordinates, 32 of out-edges, degree, count, base; tags: 64 of corners in, 64 out, margin, code, four int32
        assert lines[0] == ("PER-POINT 60" if stage == "quads" else "PER-QUAD 160")
        cut = [int(c) for c in lines[1].split()[1:]]
        # the block of the call is sized for the chunk of the most images and for the chunk of the most rows
        ends = [sum(counts[:k]) for k in cut]
        assert lines[2] == "MOST %d %d" % (max(b - a for a, b in zip(cut, cut[1:])), max(b - a for a, b in zip(ends, ends[1:])))
        return cut
    return run


def model(on_device, img_bytes, limit, counts, per_image=16, per_row=60):
    """The rule restated: a chunk takes images while its bytes - 16 per image, the pixels in the host call, 60 per point (the tag
    decoder: 8 per image, 160 per quad) - stay within the limit, and one image at least."""
    cut, k = [0], 0
    while k < len(counts):
        size = 0
        while k < len(counts) and (size == 0 or size + (0 if on_device else img_bytes) + per_image + per_row * counts[k] <= limit):
            size += (0 if on_device else img_bytes) + per_image + per_row * counts[k]
            k += 1
        cut.append(k)
    return cut


def test_the_planner_follows_its_rule(planner):
    for counts in ([5], [0, 0, 0], [130, 0, 65, 4, 130], [1000, 1, 1, 1, 1000, 2000, 3]):
        for on_device in (False, True):
            for limit in (0, 1, 76, 77, 4000, 33000, 64032, 64033, 10 ** 6, 2 ** 40):
                got = planner(on_device, 32000, limit, counts)
                assert got == model(on_device, 32000, limit, counts), (counts, on_device, limit)
                assert got[0] == 0 and got[-1] == len(counts) and all(b > a for a, b in zip(got, got[1:]))
    # 76 bytes for the image with a point, 16 for each of the others: the limit is inclusive
    assert planner(True, 32000, 92, [1, 0, 0]) == [0, 2, 3] and planner(True, 32000, 91, [1, 0, 0]) == [0, 1, 3]


def test_the_limits_of_the_gpu_chunk_test_cut_its_batch_as_it_says(planner):
    case = ref.batch_case()
    n, H, W = case["images"].shape
    counts = [len(x) for x in case["xy_list"]]
    assert counts == [130, 0, 65, 4, 130] and case["images"].dtype.itemsize * H * W == 32000
    for on_device, limits in ((False, ref.CHUNK_LIMITS_HOST), (True, ref.CHUNK_LIMITS_DEV)):
        assert planner(on_device, 32000, limits[0], counts) == [0, 1, 2, 3, 4, 5]
        assert planner(on_device, 32000, limits[1], counts) == list(ref.CHUNK_GROUPS)
        assert planner(on_device, 32000, 256 << 20, counts) == [0, 5]                       # the product's limit: one chunk
    # a chunk of more than one image that is not the first: images 2 and 3, both with points
    assert ref.CHUNK_GROUPS[1:3] == (2, 4) and counts[2] > 0 and counts[3] > 0


def test_the_planner_follows_its_rule_with_the_tag_decoders_figures(planner):
    for counts in ([5], [0, 0, 0], [130, 0, 65, 4, 130], [1000, 1, 1, 1, 1000, 2000, 3]):
        for on_device in (False, True):
            for limit in (0, 1, 76, 77, 4000, 33000, 64032, 64033, 10 ** 6, 2 ** 40):
                got = planner(on_device, 32000, limit, counts, "tags")
                assert got == model(on_device, 32000, limit, counts, 8, 160), (counts, on_device, limit)
                assert got[0] == 0 and got[-1] == len(counts) and all(b > a for a, b in zip(got, got[1:]))
    # 168 bytes for the image with a quad, 8 for each of the others: the limit is inclusive
    assert planner(True, 32000, 176, [1, 0, 0], "tags") == [0, 2, 3] and planner(True, 32000, 175, [1, 0, 0], "tags") == [0, 1, 3]


def test_the_limits_of_the_gpu_tags_chunk_test_cut_its_batch_as_it_says(planner):
    case = tag_ref.batch_case()
    n, H, W = case["images"].shape
    counts = [len(q) for q in case["quads_list"]]
    assert counts == [60, 0, 140] and case["images"].dtype.itemsize * H * W == 76800
    for on_device, limits in ((False, tag_ref.CHUNK_LIMITS_HOST), (True, tag_ref.CHUNK_LIMITS_DEV)):
        for limit in limits + (256 << 20,):
            assert planner(on_device, 76800, limit, counts, "tags") == model(on_device, 76800, limit, counts, 8, 160)
        assert planner(on_device, 76800, limits[0], counts, "tags") == [0, 1, 2, 3]          # every image on its own
        assert planner(on_device, 76800, limits[1], counts, "tags") == list(tag_ref.CHUNK_GROUPS)
        assert planner(on_device, 76800, 256 << 20, counts, "tags") == [0, 3]                 # the product's limit: one chunk
    # the limits the GPU test's parameters name are the host call's: first two images together, third alone
    assert tag_ref.CHUNK_LIMITS_HOST == (1, 200000) and tag_ref.CHUNK_GROUPS == (0, 2, 3)
    # the host call's second limit does not cut the _dev call's batch at all, which is why that call has a limit of its own
    assert planner(True, 76800, tag_ref.CHUNK_LIMITS_HOST[1], counts, "tags") == [0, 3]
