"""CPU: ccal_detect_tags_* without a device - the exported symbols, the binding's struct against the header, the links of the rule as
tests/tagchain_ref.py restates them (merge, select, and chain() over the four stage yardsticks on the montage fixture), and the chunk
planner of both image chains (csrc/ccal_tagchain_plan.hpp) through a plain C++ program under the host's address and
undefined-behaviour sanitizers.  No GPU, nothing outside the repository."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tag_ref  # noqa: E402
import tagchain_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_exported_and_refuse_a_null_context():
    lib = _ffi.load()
    o = _ffi.DetectTagsOpts()
    cnt = np.zeros(1, dtype=np.int32)
    for fn in (lib.ccal_detect_tags_batch, lib.ccal_detect_tags_dev):
        assert fn(None, 0, 8, 8, 0, None, 6, None, 1, ctypes.byref(o), None, None, None, None, None, None, None, None) == _ffi.ERR_INVALID_ARG
        assert fn(None, 0, 8, 8, 1, None, 6, None, 1, ctypes.byref(o), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, None,
                  None, None, None, None) == _ffi.ERR_INVALID_ARG
    for name in ("ccal_detect_tags_batch", "ccal_detect_tags_dev"):
        assert [s for s in _ffi.SYMBOLS if s[0] == name]
    legacy = _ffi.load_legacy()                            # the hooks are the second library's alone
    assert hasattr(legacy, "ccal_test_merge_points") and hasattr(legacy, "ccal_test_select_tags")
    assert not hasattr(lib, "ccal_test_merge_points") and not hasattr(lib, "ccal_test_select_tags")


def test_the_bindings_struct_is_the_headers():
    src = open(os.path.join(ROOT, "include", "ccal.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ccal_detect_tags_opts;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[ctype]) for n in names.split(",")]
    assert fields == list(_ffi.DetectTagsOpts._fields_)
    assert ctypes.sizeof(_ffi.DetectTagsOpts) == sum(ctypes.sizeof(t) for _, t in fields) == 128          # no padding anywhere
    assert set(ref.OPTS) | {"reserved_"} == {n for n, _ in fields}
    text = re.search(r"AprilGrid tags from images in one call.*?ccal_detect_tags_opts;", src, flags=re.S).group(0)
    assert "CCAL_ERR_INVALID_ARG, nothing launched or written" in text and "32768" in text
    assert (_ffi.TAGS_FLAG_CUT, _ffi.TAGS_FLAG_CAND_CAP, _ffi.TAGS_FLAG_QUAD_CAP, _ffi.TAGS_FLAG_TAG_CAP) == \
        (ref.FLAG_CUT, ref.FLAG_CAND_CAP, ref.FLAG_QUAD_CAP, ref.FLAG_TAG_CAP) == (1, 2, 4, 8)


# ---- the links --------------------------------------------------------------------------------------------------------------------------
def test_merge_keeps_the_end_of_a_chain():
    """a - b - c with b within the radius of a, c within the radius of b but not of a: b is dropped and screens nothing, c is kept."""
    pts = np.array([[10.0, 10.0], [11.0, 10.5], [12.0, 11.0], [10.0, 11.0], [30.0, 30.0], [30.0, 30.0], [31.0, 29.0], [31.5, 29.0]])
    got = ref.merge(pts, 1.0)
    assert got.tolist() == [[10.0, 10.0], [12.0, 11.0], [30.0, 30.0], [31.5, 29.0]]          # a distance exactly equal to the radius merges
    assert np.array_equal(got, api.merge_points(pts, 1.0))
    assert ref.merge(np.zeros((0, 2)), 1.0).shape == (0, 2) and len(ref.merge(pts, 0.0)) == 7          # radius 0: exact duplicates only


def test_select_keeps_the_best_quad_of_each_id():
    OK, NO = tag_ref.OK, tag_ref.NO_CODE
    reason = [OK, NO, OK, OK, OK, OK, tag_ref.BORDER, OK]
    tag_id = [5, 5, 2, 5, 2, 5, 2, 9]
    hamming = [1, 0, 0, 0, 0, 0, 0, 2]
    margin = [9.0, 50.0, 3.0, 4.0, 3.0, 7.0, 99.0, 1.0]
    # id 2: rows 2 and 4 tie exactly - the earlier row; id 5: hamming 0 beats 1, then the larger margin (row 5); non-OK rows never win
    assert ref.select(reason, tag_id, hamming, margin) == [2, 5, 7]
    assert ref.select([], [], [], []) == [] and ref.select([NO], [0], [0], [1.0]) == []


# ---- the chain on the montage: every id twice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nms_radius", [5, 3])
def test_the_chain_on_a_montage_keeps_one_quad_of_each_pair(nms_radius):
    img = ref.montage(0)
    assert img.shape == (240, 640)
    codes = tag_ref.grid_family().codes
    o = ref.opts(np.uint8, 640, 240, nms_radius=nms_radius)
    got = ref.chain(img, tag_ref.GRID_D, codes, o)
    dec = got["decoded"]
    ok = [j for j, x in enumerate(dec) if x["reason"] == tag_ref.OK]
    assert sorted(dec[j]["id"] for j in ok) == sorted(list(range(6)) * 2) and got["stats"][3] == 12
    assert len({dec[j]["margin"] for j in ok}) == 12                                           # no tie: the margins decide
    assert got["count"] == 6 and got["id"].tolist() == list(range(6)) and got["flags"] == 0
    for row, t in enumerate(got["id"]):
        pair = [j for j in ok if dec[j]["id"] == t]
        best = min(pair, key=lambda j: (dec[j]["hamming"], -dec[j]["margin"]))
        assert got["margin"][row] == dec[best]["margin"] and np.array_equal(got["corners"][row], dec[best]["corners"])
    if nms_radius == 3:                                                                        # candidates that refine onto one saddle
        assert (len(got["refined"]), len(got["points"])) == (221, 215) and got["stats"][1] == 215
    else:
        assert len(got["points"]) <= len(got["refined"])
    print(f"nms_radius {nms_radius}: stats {got['stats']}, refined {len(got['refined'])}")


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tagchain_plan") / "test_tagchain_plan")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_tagchain_plan.cpp"), "-o", exe])

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        out = subprocess.run([exe] + [str(int(a)) for a in args], env=env, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
        return out.stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def planner(planner_lines):
    def run(*args):
        lines = planner_lines(*args)
        assert lines[0].startswith("ROWS ") and lines[1].startswith("PER-IMAGE ") and lines[2].startswith("CHUNK ")
        return int(lines[1].split()[1]), int(lines[2].split()[1])
    return run


@pytest.fixture(scope="module")
def board_planner(planner_lines):
    """(bytes per image, images per chunk) of ccal_detect_checkerboards_*; the tag chain's caps do not enter (the library passes 1)."""
    def run(on_device, width, height, itemsize, step, r, cand_cap, corners, limit, n_img):
        lines = planner_lines(on_device, width, height, itemsize, step, r, cand_cap, 1, 1, 1, limit, n_img, corners)
        assert lines[3].startswith("BOARD-PER-IMAGE ") and lines[4].startswith("BOARD-CHUNK ")
        return int(lines[3].split()[1]), int(lines[4].split()[1])
    return run


def test_the_planner_follows_its_rule(planner):
    shapes = ((320, 240, 1), (752, 480, 2), (67, 45, 1), (6, 240, 1), (320, 7, 2))           # the last two: no domain at step 1 / 2
    for width, height, itemsize in shapes:
        for on_device in (False, True):
            for step, r, cand_cap, quad_cap, tag_cap, n_codes in ((1, 5, 4096, 1024, 40, 40), (2, 3, 7, 1, 2, 587), (4, 15, 32768, 10 ** 6, 10 ** 6, 3)):
                for limit, n_img in ((0, 5), (1, 1), (10 ** 6, 1024), (256 << 20, 1024), (2 ** 40, 10 ** 5)):
                    args = (on_device, width, height, itemsize, step, r, cand_cap, quad_cap, tag_cap, n_codes, limit, n_img)
                    assert planner(*args) == ref.plan_model(*args), args
    per, _ = ref.plan_model(True, 320, 240, 1, 1, 5, 4096, 1024, 40, 40, 0, 1)
    assert planner(True, 320, 240, 1, 1, 5, 4096, 1024, 40, 40, 3 * per, 10)[1] == 3              # the limit is inclusive
    assert planner(True, 320, 240, 1, 1, 5, 4096, 1024, 40, 40, 3 * per - 1, 10)[1] == 2


def test_the_limits_of_the_gpu_chunk_test_cut_its_batch_as_it_says(planner):
    """tests/test_gpu_detect_tags.py::test_a_batch_cut_into_chunks runs the four fixture frames one image per chunk and two per chunk,
    through the host call and the _dev call, with limits from tagchain_ref.chunk_limit: the library's planner cuts them exactly so,
    and the product's 256 MB takes the four images in one chunk."""
    o = ref.opts(nms_radius=3)                             # that test's options
    for on_device in (False, True):
        for per_chunk in (1, 2):
            limit = ref.chunk_limit(on_device, (tag_ref.GRID_H, tag_ref.GRID_W), 1, o, 40, per_chunk)
            args = (on_device, tag_ref.GRID_W, tag_ref.GRID_H, 1, o["step"], o["nms_radius"], o["cand_cap"], o["quad_cap"], o["tag_cap"], 40)
            assert planner(*args, limit, 4)[1] == per_chunk
        assert planner(*args, 256 << 20, 4)[1] == 4


def test_the_board_chains_planner_follows_its_rule(board_planner):
    rng = np.random.default_rng(20)
    shapes = [(320, 240, 1, 1, 5, 4096, 35), (752, 480, 2, 2, 3, 7, 4), (6, 240, 1, 1, 5, 4096, 35)]           # the last: no domain
    for _ in range(8):
        shapes.append((int(rng.integers(7, 1500)), int(rng.integers(7, 1100)), int(rng.integers(1, 3)), int(rng.integers(1, 5)),
                       int(rng.integers(1, 16)), int(rng.integers(1, 4097)), int(rng.integers(2, 21)) * int(rng.integers(2, 21))))
    for width, height, itemsize, step, r, cand_cap, corners in shapes:
        for on_device in (False, True):
            for limit, n_img in ((0, 5), (1, 1), (10 ** 6, 1024), (256 << 20, 1024), (2 ** 40, 10 ** 5)):
                args = (on_device, width, height, itemsize, step, r, cand_cap, corners, limit, n_img)
                assert board_planner(*args) == ref.board_plan_model(*args), args


def test_the_limits_of_the_board_chunk_test_cut_its_batch_as_it_says(board_planner):
    """tests/test_gpu_board.py::test_a_batch_cut_into_chunks runs 320 x 240 u8 images at step 1, radius 5, cand_cap 4096 for a 7 x 5
    board through ccal_detect_checkerboards_* with limits of 1 and 800 000 bytes.  The domain is 314 x 234: 53 x 39 = 2067 slots, as
    many candidate rows, 512 kept slots.  Per image 2067 * 24 + 234 * 4 + 2067 * 84 + 512 * 108 + 35 * 16 + 64 = 280 092 bytes, and
    76 800 more when the call stages the image: two images per chunk at 800 000 either way, one at a limit of 1."""
    shape = (320, 240, 1, 1, 5, 4096, 35)
    assert 2067 * 24 + 234 * 4 + 2067 * (28 + 56) + 512 * 108 + 35 * 16 + 64 == 280092
    assert board_planner(True, *shape, 800000, 6) == (280092, 2)
    assert board_planner(False, *shape, 800000, 6) == (356892, 2)
    assert board_planner(True, *shape, 1, 6)[1] == 1 and board_planner(False, *shape, 1, 6)[1] == 1
    assert board_planner(True, *shape, 3 * 280092, 6)[1] == 3 and board_planner(True, *shape, 3 * 280092 - 1, 6)[1] == 2       # inclusive
    assert board_planner(False, *shape, 256 << 20, 6)[1] == 6                                  # the product's limit: one chunk
