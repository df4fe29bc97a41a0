"""GPU: the quad proposer (ccal_kernels_quads.hip, ccal_propose_quads_batch / _dev, Context.propose_quads_batch, api.propose_quads,
api.detect_aprilgrid) against tests/quad_ref.py, the numpy f64 yardstick of the rule stated in include/ccal.h.

Bounds.  Counts, indices and flags are decisions and integers, and quads_out holds copies of input points: everything is compared
with ==, bit for bit, for every image of every case, no exclusions.  Every fixture keeps its edge decisions at least 1e-3 grey
levels and its geometric comparisons at least 1e-6 relative from equality (tests/test_quads_cpu.py holds that on the CPU), and the
unit is compiled without fused multiply-adds, so no decision rides on the last bits of a sum.  Images are at most 320 x 240 with at
most 130 points; every case takes well under a second."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quad_ref as ref  # noqa: E402
import tag_ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, -3.25


IP, LP, DP = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def raw_propose(ctx, case, fn=None, ptr=None, want_quads=True, **change):
    """The C entry point on a case, every output prefilled with a sentinel: {"rc", "count", "flags", "idx", "quads"}.  change:
    arguments replaced (tests of invalid ones); "null": names of pointers passed as NULL."""
    imgs = case["images"]
    n_img, H, W = imgs.shape
    offs = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([len(x) for x in case["xy_list"]], out=offs[1:])
    xy = np.ascontiguousarray(np.concatenate(case["xy_list"]) if n_img else np.zeros((0, 2)))
    a = dict(dtype=_code(imgs.dtype), w=W, h=H, n=n_img, offs=offs, null=(), **{k: case[k] for k in ref.DEFAULTS})
    a.update(change)
    offs = None if a["offs"] is None else np.ascontiguousarray(a["offs"], dtype=np.int64)
    m, rows = max(n_img, 1), max(int(a["cap"]), 1)
    out = {"count": np.full(m, SENT_I, dtype=np.int32), "flags": np.full(m, SENT_I, dtype=np.int32),
           "idx": np.full((m, rows, 4), SENT_I, dtype=np.int32), "quads": np.full((m, rows, 4, 2), SENT_F)}
    p = lambda name, arr, t: None if name in a["null"] else arr.ctypes.data_as(t)      # noqa: E731
    fn = fn or ctx.lib.ccal_propose_quads_batch
    img_ptr = None if "images" in a["null"] else C.c_void_p(imgs.ctypes.data if ptr is None else ptr)
    out["rc"] = fn(ctx.handle, a["dtype"], a["w"], a["h"], a["n"], img_ptr, None if offs is None else offs.ctypes.data_as(LP),
                   p("xy", xy, DP), a["min_side"], a["max_side"], a["max_side_ratio"], a["offset"], a["samples"], a["min_contrast"],
                   a["cap"], p("count", out["count"], IP), p("flags", out["flags"], IP),
                   p("idx", out["idx"], IP), p("quads", out["quads"], DP) if want_quads else None)
    return out


def untouched(out):
    return bool((out["count"] == SENT_I).all() and (out["flags"] == SENT_I).all() and (out["idx"] == SENT_I).all()
                and (out["quads"] == SENT_F).all())


def check_against_yardstick(got, case, want_quads=True):
    """Exact: counts, flags, indices, the coordinates' bits, and the sentinel in every row past min(count, cap)."""
    assert got["rc"] == _ffi.OK
    rows = got["idx"].shape[1]
    for k, r in enumerate(ref.yardstick(case)):
        where = (case["name"], k)
        assert (int(got["count"][k]), int(got["flags"][k])) == (r["count"], r["flags"]), where
        m = min(r["count"], case["cap"])
        assert m == len(r["idx"]) and m <= rows, where
        assert np.array_equal(got["idx"][k, :m], r["idx"][:m]), where
        assert (got["idx"][k, m:] == SENT_I).all(), where
        if want_quads:
            assert got["quads"][k, :m].tobytes() == np.ascontiguousarray(r["quads"][:m]).tobytes(), where
            assert (got["quads"][k, m:] == SENT_F).all(), where
        else:
            assert (got["quads"] == SENT_F).all()


def cropped_frame(dtype):
    imgs, truth = tag_ref.grid_frames(dtype)
    cut_x = int(round(np.concatenate([truth[0][2][:, 0], truth[0][5][:, 0]]).mean()))
    return np.ascontiguousarray(imgs[0][:, :cut_x])


def bits(out):
    return b"".join(out[k].tobytes() for k in ("count", "flags", "idx", "quads"))


# ---- 1. parity: the fixture frames, point counts around the 64-lane stride, K, dtype, overflow, bounds, cap ---------------------------------
@pytest.mark.parametrize("name", ref.parity_case_names())
def test_parity(gpu_ctx, name):
    case = ref.parity_case(name)
    got = raw_propose(gpu_ctx, case)
    check_against_yardstick(got, case)
    print(f"{name}: points {[len(x) for x in case['xy_list']]}, quads {got['count'][:len(case['xy_list'])].tolist()}, "
          f"flags {got['flags'][:len(case['xy_list'])].tolist()}")
    again = raw_propose(gpu_ctx, case)
    assert bits(again) == bits(got)                                      # two runs: the same bits


def test_the_cases_cover_what_they_are_for():
    ys = {c["name"]: ref.yardstick(c) for c in ref.parity_cases()}
    assert [r["count"] for r in ys["fixture uint8 min_side 20"]] == [6] * 4 and [r["count"] for r in ys["fixture uint8 min_side 6"]] == [18] * 4
    assert ys["out-edge overflow"][0]["flags"] == ref.FLAG_CUT and ys["out-edge overflow"][0]["count"] == 0
    assert ys["cap 1"][0]["count"] > 1 and len(ys["cap 1"][0]["idx"]) == 1
    assert any(r["flags"] and r["count"] for c in ref.sheet_cases() if c["samples"] == 1 for r in ref.yardstick(c))     # cut lists with quads
    assert sorted({len(x) for c in ref.sheet_cases() for x in c["xy_list"]}) == [0, 1, 3, 4, 63, 64, 65, 130]


# ---- 2. batch shape -----------------------------------------------------------------------------------------------------------------
def test_an_images_outputs_do_not_depend_on_its_place_in_the_batch(gpu_ctx):
    case = ref.batch_case()
    whole = raw_propose(gpu_ctx, case)
    check_against_yardstick(whole, case)
    assert len(case["xy_list"][1]) == 0 and ref.yardstick(case)[2]["count"] > 0
    for k in (0, 2, 3):
        one = dict(case, name=f"image {k} alone", images=case["images"][k:k + 1], xy_list=case["xy_list"][k:k + 1])
        alone = raw_propose(gpu_ctx, one)
        assert alone["rc"] == _ffi.OK
        for key in ("count", "flags", "idx", "quads"):
            assert alone[key][0].tobytes() == whole[key][k].tobytes(), (k, key)
    swapped = dict(case, name="five images, reversed", images=np.ascontiguousarray(case["images"][::-1]), xy_list=case["xy_list"][::-1])
    back = raw_propose(gpu_ctx, swapped)
    for key in ("count", "flags", "idx", "quads"):
        assert np.ascontiguousarray(back[key][::-1]).tobytes() == whole[key].tobytes(), key


def test_no_images_and_images_without_points_are_valid(gpu_ctx):
    for fn in (gpu_ctx.lib.ccal_propose_quads_batch, gpu_ctx.lib.ccal_propose_quads_dev):
        assert fn(gpu_ctx.handle, _ffi.PIX_U8, 64, 48, 0, None, None, None, 20.0, 120.0, 2.0, 1.0 / 16.0, 8, 40.0, 16,
                  None, None, None, None) == _ffi.OK
    assert gpu_ctx.propose_quads_dev(0, _ffi.PIX_U8, 64, 48, 0, []) == []
    case = dict(ref.batch_case(), name="no points", xy_list=[np.zeros((0, 2))] * 5)
    got = raw_propose(gpu_ctx, case, null=("xy",))
    assert got["rc"] == _ffi.OK and (got["count"] == 0).all() and (got["flags"] == 0).all()
    assert (got["idx"] == SENT_I).all() and (got["quads"] == SENT_F).all()


def test_quads_out_may_be_null(gpu_ctx):
    case = ref.batch_case()
    lean = raw_propose(gpu_ctx, case, want_quads=False)
    check_against_yardstick(lean, case, want_quads=False)


@pytest.mark.parametrize("which", [0, 1], ids=["an image per chunk", "groups of images"])
def test_a_batch_cut_into_chunks(dev_ctx, gpu_ctx, monkeypatch, which):
    """The library runs a batch whose block would exceed 256 MB in chunks of whole images.  The second library reads the limit from
    CCAL_TEST_QUADS_CHUNK_BYTES (tests only).  The five 32 000-byte images of batch_case() carry 130, 0, 65, 4 and 130 points, and a
    chunk counts 16 bytes per image, the pixels in the host call only, and 60 bytes per point: so the host call and the _dev call
    get limits of their own (quad_ref.CHUNK_LIMITS_HOST / _DEV).  1 byte: every image a chunk of its own, the one without points
    skipped.  80 000 / 8 000 bytes: the images (0, 1), (2, 3), (4) - the second chunk holds two images with points and starts
    at image 2 and point 130, which is what a batch beyond 256 MB looks like to the kernels.  That the library's planner cuts
    exactly so is held on the CPU (tests/test_quads_plan_cpu.py).  Host and device entry: the product's bits."""
    import torch
    case = ref.batch_case()
    assert [len(x) for x in case["xy_list"]] == [130, 0, 65, 4, 130] and case["images"][0].nbytes == 32000
    assert ref.CHUNK_GROUPS == (0, 2, 4, 5) and (ref.CHUNK_LIMITS_HOST[which], ref.CHUNK_LIMITS_DEV[which]) == ((1, 1), (80000, 8000))[which]
    whole = raw_propose(gpu_ctx, case)
    check_against_yardstick(whole, case)
    assert all(ref.yardstick(case)[k]["count"] > 0 for k in (2, 3))          # both images of the middle chunk store rows
    raw = torch.from_numpy(case["images"].copy()).cuda()
    torch.cuda.synchronize()
    monkeypatch.setenv("CCAL_TEST_QUADS_CHUNK_BYTES", str(ref.CHUNK_LIMITS_HOST[which]))
    got = raw_propose(dev_ctx, case)
    assert got["rc"] == _ffi.OK and bits(got) == bits(whole)
    monkeypatch.setenv("CCAL_TEST_QUADS_CHUNK_BYTES", str(ref.CHUNK_LIMITS_DEV[which]))
    got = raw_propose(dev_ctx, case, fn=dev_ctx.lib.ccal_propose_quads_dev, ptr=raw.data_ptr())
    assert got["rc"] == _ffi.OK and bits(got) == bits(whole)


# ---- 3. the _dev entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_dev_entry_point_on_a_block_written_by_remap_dev(gpu_ctx, dtype):
    """The images go through ccal_remap_dev with an identity map (every output pixel reads its own source pixel: the same bytes)
    into a torch-allocated block; ccal_propose_quads_dev follows on the context's stream without a synchronise in between."""
    import torch
    case = ref.parity_case(f"fixture {np.dtype(dtype).name} min_side 20")
    imgs = case["images"]
    n, H, W = imgs.shape
    host = raw_propose(gpu_ctx, case)
    check_against_yardstick(host, case)
    xm, ym = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    m = gpu_ctx.undistort_map_from_arrays(np.ascontiguousarray(xm), np.ascontiguousarray(ym))
    try:
        src = torch.from_numpy(imgs.view(np.uint8).copy()).cuda()
        dst = torch.zeros_like(src)
        torch.cuda.synchronize()
        m.remap_dev(src.data_ptr(), dst.data_ptr(), _code(dtype), 1, W, H, n)
        dev = raw_propose(gpu_ctx, case, fn=gpu_ctx.lib.ccal_propose_quads_dev, ptr=dst.data_ptr())
        assert dst.cpu().numpy().tobytes() == imgs.tobytes()
    finally:
        m.close()
    assert dev["rc"] == _ffi.OK and bits(dev) == bits(host)
    wrapped = gpu_ctx.propose_quads_dev(dst.data_ptr(), _code(dtype), W, H, n, case["xy_list"], min_contrast=case["min_contrast"])
    for k, (idx, quads, count, flags) in enumerate(wrapped):
        r = ref.yardstick(case)[k]
        assert (count, flags) == (r["count"], r["flags"]) and np.array_equal(idx, r["idx"]) and np.array_equal(quads, r["quads"])


# ---- 4. the allocation poison -----------------------------------------------------------------------------------------------------------
def test_parity_on_poisoned_workspace(dev_ctx, monkeypatch):
    """The second library with CCAL_TEST_POISON_ALLOC=1 (tests/test_gpu_poison.py): the stored coordinates start as NaN bytes in
    every call; the kernel writes every stored row before the copy back."""
    monkeypatch.setenv("CCAL_TEST_POISON_ALLOC", "1")
    for name in ("fixture uint16 min_side 20", "sheets 200 x 160 K 1 uint8", "cap 1", "five images", "out-edge overflow"):
        check_against_yardstick(raw_propose(dev_ctx, ref.parity_case(name)), ref.parity_case(name))


# ---- 5. invalid arguments ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(gpu_ctx):
    case = ref.batch_case()
    nan, inf = float("nan"), float("inf")
    bad = [dict(min_side=0.5), dict(min_side=nan), dict(max_side=19.0), dict(max_side=nan), dict(max_side_ratio=0.9),
           dict(max_side_ratio=nan), dict(offset=0.0), dict(offset=-0.1), dict(offset=0.26), dict(offset=nan), dict(samples=0),
           dict(samples=17), dict(min_contrast=-1.0), dict(min_contrast=nan), dict(min_contrast=inf), dict(cap=0), dict(cap=-3),
           dict(dtype=2), dict(dtype=-1), dict(w=0), dict(h=-1), dict(n=-1), dict(w=65536, h=32768),
           dict(offs=[1, 1, 1, 2, 2, 2]), dict(offs=[0, 2, 1, 3, 3, 3]), dict(offs=[0, 0, 0, 0, 0, 2 ** 31]),
           dict(offs=[0, 32769, 32769, 32769, 32769, 32769]), dict(offs=None),
           dict(null=("images",)), dict(null=("xy",)), dict(null=("count",)), dict(null=("flags",)), dict(null=("idx",))]
    for fn in (gpu_ctx.lib.ccal_propose_quads_batch, gpu_ctx.lib.ccal_propose_quads_dev):
        for change in bad:
            got = raw_propose(gpu_ctx, case, fn=fn, **change)
            assert got["rc"] == _ffi.ERR_INVALID_ARG, change
            assert untouched(got), change
            assert gpu_ctx.last_error()
    with pytest.raises(ValueError):
        gpu_ctx.propose_quads_batch(np.zeros((1, 45, 67, 3), dtype=np.uint8), [np.zeros((0, 2))])                       # colour
    with pytest.raises(ValueError):
        gpu_ctx.propose_quads_batch(np.zeros((2, 45, 67), dtype=np.uint8), [np.zeros((0, 2))])
    with pytest.raises(ValueError):
        gpu_ctx.propose_quads_batch(np.zeros((1, 45, 67), dtype=np.float32), [np.zeros((0, 2))])


# ---- 6. the engine and api layers -----------------------------------------------------------------------------------------------------------
def test_context_and_api_wrappers(gpu_ctx):
    case = ref.parity_case("fixture uint8 min_side 20")
    got = gpu_ctx.propose_quads_batch(case["images"], case["xy_list"])                   # max_side None: half of 320
    for k, (idx, quads, count, flags) in enumerate(got):
        r = ref.yardstick(case)[k]
        assert (count, flags) == (r["count"], r["flags"]) and idx.dtype == np.int32
        assert np.array_equal(idx, r["idx"]) and np.array_equal(quads, r["quads"])
    one = gpu_ctx.propose_quads_batch(case["images"], case["xy_list"], max_per_image=1)
    assert all(len(q[0]) == 1 and q[2] == 6 and np.array_equal(q[0], g[0][:1]) for q, g in zip(one, got))
    # the api layer merges first: the refined points with their duplicates give the same quads
    fam = api.TagFamily("toy", 36, tag_ref.grid_family().codes)
    refined = [r for r, _ in ref.fixture_points(np.uint8)]
    for k, (quads, count, flags) in enumerate(api.propose_quads(list(case["images"]), refined, fam, ctx=gpu_ctx)):
        assert (count, flags) == (6, 0) and np.array_equal(quads, ref.yardstick(case)[k]["quads"])
    assert api.propose_quads([], [], fam, ctx=gpu_ctx) == []


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_detect_aprilgrid_from_images_alone(gpu_ctx, dtype):
    """The rendered 3 x 2 AprilGrid of tests/tag_ref.py from pixels to FrameFeatures in one call: every frame complete, every
    corner named and within 0.2 px of the projected truth (the CPU chain's worst is 0.105 px; 0.2 is the bound the end-to-end tag
    test holds the same refinement to).  A frame cropped to four tags has 16 < 24 corners: None."""
    imgs, truth = tag_ref.grid_frames(dtype)
    scale = 257 if dtype == np.uint16 else 1
    fam = api.TagFamily("toy", 36, tag_ref.grid_family().codes)
    board = api.AprilGridBoard(tag_ref.GRID.tag_size_meter, tag_ref.GRID.tag_spacing, tag_ref.GRID.tag_rows, tag_ref.GRID.tag_cols)
    frames = api.detect_aprilgrid(list(imgs), fam, board, min_contrast=40.0 * scale, times=[100 + k for k in range(len(imgs))], ctx=gpu_ctx)
    worst = 0.0
    assert len(frames) == len(imgs)
    for k, f in enumerate(frames):
        assert f is not None and f.time_ns == 100 + k and f.img_w_h == (tag_ref.GRID_W, tag_ref.GRID_H) and sorted(f.features) == list(range(24))
        for i in range(24):
            assert f.features[i].p3d == board.id_to_3d[i]
            e = float(np.hypot(*(np.array(f.features[i].p2d) - truth[k].reshape(-1, 2)[i])))
            worst = max(worst, e)
            assert e <= 0.2, (k, i, e)
    print(f"{np.dtype(dtype).name}: worst distance of a p2d to the projected truth {worst:.4f} px")
    # frame 0 cropped through the middle of its right tag column: four whole tags (tests/test_quads_cpu.py runs the same crop on the CPU)
    part = cropped_frame(dtype)
    got = api.detect_aprilgrid([part], fam, board, min_contrast=40.0 * scale, ctx=gpu_ctx)
    assert got == [None]
    low = api.detect_aprilgrid([part], fam, board, min_contrast=40.0 * scale, min_corners=16, ctx=gpu_ctx)[0]
    assert low is not None and sorted(low.features) == [4 * m + i for m in (0, 1, 3, 4) for i in range(4)]
    assert api.detect_aprilgrid([], fam, board, ctx=gpu_ctx) == []
