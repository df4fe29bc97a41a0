"""GPU: the tag decoder (ccal_kernels_tags.hip, ccal_decode_tags_batch / _dev, api.decode_tags, api.frames_from_tags) against
tests/tag_ref.py, the numpy f64 yardstick of the rule stated in include/ccal.h.

Bounds.  reason, id, rot, hamming and code are decisions and integers: compared with ==, for every quad of every case, no
exclusions.  corners are copies of input corners and margin is a minimum of |value - t| over cell means the kernel forms in the
yardstick's order without fused multiply-adds: held to 1e-9 max(1, |value|), the suite's bound for f64 against f64.  Every fixture
keeps its cells at least 0.5 grey levels from the threshold (tests/test_tags_cpu.py holds that on the CPU), so no decision rides on
the last bits of a sum.  Images are at most 320 x 240, calls hold at most a few hundred quads; every case takes well under a second."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402
import tag_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_I, SENT_F, SENT_U = -77, -3.25, 0xABCDEF0123456789
CASES = {c["name"]: c for c in ref.parity_cases()}
IP, LP, DP, UP = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def raw_decode(ctx, case, fn=None, ptr=None, optional=True, **change):
    """The C entry point on a case, every output prefilled with a sentinel: {"rc", "reason", "id", "rot", "hamming", "corners",
    "code", "margin"} over all quads of the call in order.  change: arguments replaced (tests of invalid ones); "null": names of
    pointers passed as NULL."""
    imgs = case["images"]
    n_img, H, W = imgs.shape
    offs = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([len(q) for q in case["quads_list"]], out=offs[1:])
    quads = np.ascontiguousarray(np.concatenate(case["quads_list"]) if n_img else np.zeros((0, 4, 2)))
    codes = np.array(case["codes"], dtype=np.uint64)
    a = dict(dtype=_code(imgs.dtype), w=W, h=H, n=n_img, offs=offs, d=case["d"], border=case["border"], n_codes=len(codes),
             samples=case["samples"], min_contrast=case["min_contrast"], max_border=case["max_border_errors"], max_hamming=case["max_hamming"],
             null=())
    a.update(change)
    offs = None if a["offs"] is None else np.ascontiguousarray(a["offs"], dtype=np.int64)
    m = max(len(quads), 1)
    out = {"reason": np.full(m, SENT_I, dtype=np.int32), "id": np.full(m, SENT_I, dtype=np.int32), "rot": np.full(m, SENT_I, dtype=np.int32),
           "hamming": np.full(m, SENT_I, dtype=np.int32), "corners": np.full((m, 4, 2), SENT_F), "code": np.full(m, SENT_U, dtype=np.uint64),
           "margin": np.full(m, SENT_F)}
    p = lambda name, arr, t: None if name in a["null"] else arr.ctypes.data_as(t)      # noqa: E731
    fn = fn or ctx.lib.ccal_decode_tags_batch
    img_ptr = None if "images" in a["null"] else C.c_void_p(imgs.ctypes.data if ptr is None else ptr)
    out["rc"] = fn(ctx.handle, a["dtype"], a["w"], a["h"], a["n"], img_ptr, None if offs is None else offs.ctypes.data_as(LP),
                   p("quads", quads, DP), a["d"], a["border"], p("codes", codes, UP), a["n_codes"], a["samples"], a["min_contrast"],
                   a["max_border"], a["max_hamming"], p("reason", out["reason"], IP), p("id", out["id"], IP), p("rot", out["rot"], IP),
                   p("hamming", out["hamming"], IP), p("corners", out["corners"], DP) if optional else None,
                   p("code", out["code"], UP) if optional else None, p("margin", out["margin"], DP) if optional else None)
    return out


def untouched(out):
    return ((out["reason"] == SENT_I).all() and (out["id"] == SENT_I).all() and (out["rot"] == SENT_I).all() and (out["hamming"] == SENT_I).all()
            and (out["corners"] == SENT_F).all() and (out["code"] == SENT_U).all() and (out["margin"] == SENT_F).all())


def close(got, want):
    """1e-9 max(1, |value|), NaN where the yardstick has NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.isnan(got) == np.isnan(want)).all() and (np.abs(got - want)[~np.isnan(want)] <= 1e-9 * np.maximum(1.0, np.abs(want[~np.isnan(want)]))).all())


def check_against_yardstick(got, case):
    assert got["rc"] == _ffi.OK
    flat = [r for per_image in ref.yardstick(case) for r in per_image]
    assert len(flat) == sum(len(q) for q in case["quads_list"])
    worst = 0.0
    for j, r in enumerate(flat):
        where = (case["name"], j, ref.REASONS[r["reason"]])
        assert (got["reason"][j], got["id"][j], got["rot"][j], got["hamming"][j]) == (r["reason"], r["id"], r["rot"], r["hamming"]), where
        assert int(got["code"][j]) == r["code"], where
        assert close(got["corners"][j], r["corners"]), where
        assert close(got["margin"][j], r["margin"]), where
        if not np.isnan(r["margin"]):
            worst = max(worst, abs(got["margin"][j] - r["margin"]) / max(1.0, abs(r["margin"])))
    return worst


def bits(out):
    return b"".join(out[k].tobytes() for k in ("reason", "id", "rot", "hamming", "corners", "code", "margin"))


# ---- 1. parity: cell chunks, table strides, sampling, dtype, bounds, degenerate corners, thresholds, ties, rendered frames ---------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity(gpu_ctx, name):
    case = CASES[name]
    got = raw_decode(gpu_ctx, case)
    worst = check_against_yardstick(got, case)
    reasons = np.bincount(got["reason"][:sum(len(q) for q in case["quads_list"])], minlength=5)
    print(f"{name}: {dict(zip(ref.REASONS, reasons.tolist()))}, worst |d margin| / max(1, |margin|) {worst:.3e}")
    if "want_reasons" in case:
        assert got["reason"].tolist() == case["want_reasons"]
    if "must_be_outside" in case:
        assert all(got["reason"][i] == ref.OUTSIDE for i in case["must_be_outside"])
    if name.startswith("table"):
        assert got["id"].tolist() == case["want"] + [-1] and got["hamming"].tolist() == [1, 1, 1, -1]
        assert got["reason"][3] == ref.NO_CODE
    if name in ("equal codes", "symmetric code"):
        assert (got["id"][0], got["rot"][0], got["hamming"][0]) == case["want"]
    if name.startswith(("sheet", "rendered")):
        assert reasons[ref.OK] >= len(got["reason"]) // 2
    again = raw_decode(gpu_ctx, case)
    assert bits(again) == bits(got)                                      # two runs: the same bits


def test_the_shapes_cover_every_cell_chunk_count():
    assert sorted({(c["d"] + 2 * c["border"]) ** 2 for c in ref.sheet_cases()}) == [25, 64, 100, 144]
    assert {c["d"] for c in ref.sheet_cases()} == {3, 6, 8} and {c["samples"] for c in ref.sheet_cases()} == {1, 4}
    assert [len(c["codes"]) for c in ref.table_cases()] == [1, 63, 64, 65, 587]


# ---- 2. batch shape -----------------------------------------------------------------------------------------------------------------
def test_a_quads_outputs_do_not_depend_on_its_place_in_the_batch(gpu_ctx):
    case = ref.batch_case()
    whole = raw_decode(gpu_ctx, case)
    check_against_yardstick(whole, case)
    assert len(case["quads_list"][1]) == 0 and len(case["quads_list"][2]) > 130
    at = len(case["quads_list"][0]) + 130                                 # quad 130 of image 2
    one = dict(case, name="one quad", images=case["images"][2:3], quads_list=[case["quads_list"][2][130:131]])
    alone = raw_decode(gpu_ctx, one)
    assert alone["rc"] == _ffi.OK and alone["reason"][0] == ref.OK
    for k in ("reason", "id", "rot", "hamming", "corners", "code", "margin"):
        assert alone[k][0].tobytes() == whole[k][at].tobytes(), k


def test_no_images_is_valid(gpu_ctx):
    codes = np.array([1, 2], dtype=np.uint64)
    for fn in (gpu_ctx.lib.ccal_decode_tags_batch, gpu_ctx.lib.ccal_decode_tags_dev):
        assert fn(gpu_ctx.handle, _ffi.PIX_U8, 64, 48, 0, None, None, None, 6, 1, codes.ctypes.data_as(UP), 2, 3, 20.0, 0, 2,
                  None, None, None, None, None, None, None) == _ffi.OK
        assert fn(gpu_ctx.handle, _ffi.PIX_U8, 64, 48, 0, None, None, None, 6, 1, None, 2, 3, 20.0, 0, 2,
                  None, None, None, None, None, None, None) == _ffi.OK
    assert gpu_ctx.decode_tags_dev(0, _ffi.PIX_U8, 64, 48, 0, [], 36, [1, 2]) == ([], [], [], [], [], [], [])
    # images without quads: valid, nothing written
    case = dict(ref.batch_case(), quads_list=[np.zeros((0, 4, 2))] * 3)
    got = raw_decode(gpu_ctx, case, null=("quads",))
    assert got["rc"] == _ffi.OK and untouched(got)


def test_optional_outputs_may_be_null(gpu_ctx):
    case = CASES["sheet d 6 border 2 S 4 uint8"]
    full = raw_decode(gpu_ctx, case)
    lean = raw_decode(gpu_ctx, case, optional=False)
    assert lean["rc"] == _ffi.OK
    for k in ("reason", "id", "rot", "hamming"):
        assert np.array_equal(lean[k], full[k])
    assert (lean["corners"] == SENT_F).all() and (lean["code"] == SENT_U).all() and (lean["margin"] == SENT_F).all()


@pytest.mark.parametrize("limit", [1, 200000])
def test_a_batch_cut_into_chunks(dev_ctx, gpu_ctx, monkeypatch, limit):
    """The library runs a batch whose block would exceed 256 MB in chunks of whole images.  The second library reads the limit from
    CCAL_TEST_TAGS_CHUNK_BYTES (tests only): 1 byte - every image a chunk of its own, the one without quads skipped -, and 200 000
    bytes - the first two 77 KB images together, the third alone.  The _dev call's chunks do not hold the pixels: at 200 000 bytes it
    would take the three images at once, so it gets the limit that cuts it the same way (20 000 bytes: tag_ref.CHUNK_LIMITS_DEV).
    That the limits cut the batch exactly so is held on the CPU (tests/test_quads_plan_cpu.py).  Host and device entry: the
    product's bits."""
    import torch
    case = ref.batch_case()
    whole = raw_decode(gpu_ctx, case)
    check_against_yardstick(whole, case)
    which = ref.CHUNK_LIMITS_HOST.index(limit)
    raw = torch.from_numpy(case["images"].copy()).cuda()
    torch.cuda.synchronize()
    monkeypatch.setenv("CCAL_TEST_TAGS_CHUNK_BYTES", str(ref.CHUNK_LIMITS_HOST[which]))
    got = raw_decode(dev_ctx, case)
    assert got["rc"] == _ffi.OK and bits(got) == bits(whole)
    monkeypatch.setenv("CCAL_TEST_TAGS_CHUNK_BYTES", str(ref.CHUNK_LIMITS_DEV[which]))
    got = raw_decode(dev_ctx, case, fn=dev_ctx.lib.ccal_decode_tags_dev, ptr=raw.data_ptr())
    assert got["rc"] == _ffi.OK and bits(got) == bits(whole)


# ---- 3. the _dev entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_dev_entry_point_on_a_block_written_by_remap_dev(gpu_ctx, dtype):
    """The images go through ccal_remap_dev with an identity map (every output pixel reads its own source pixel: the same bytes)
    into a torch-allocated block; ccal_decode_tags_dev follows on the context's stream without a synchronise in between."""
    import torch
    case = CASES[f"rendered grid S 3 {np.dtype(dtype).name}"]
    imgs = case["images"]
    n, H, W = imgs.shape
    host = raw_decode(gpu_ctx, case)
    check_against_yardstick(host, case)
    xm, ym = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    m = gpu_ctx.undistort_map_from_arrays(np.ascontiguousarray(xm), np.ascontiguousarray(ym))
    try:
        src = torch.from_numpy(imgs.view(np.uint8).copy()).cuda()
        dst = torch.zeros_like(src)
        torch.cuda.synchronize()
        m.remap_dev(src.data_ptr(), dst.data_ptr(), _code(dtype), 1, W, H, n)
        dev = raw_decode(gpu_ctx, case, fn=gpu_ctx.lib.ccal_decode_tags_dev, ptr=dst.data_ptr())
        assert dst.cpu().numpy().tobytes() == imgs.tobytes()
    finally:
        m.close()
    assert dev["rc"] == _ffi.OK and bits(dev) == bits(host)
    wrapped = gpu_ctx.decode_tags_dev(dst.data_ptr(), _code(dtype), W, H, n, case["quads_list"], 36, case["codes"], case["border"],
                                      case["samples"], case["min_contrast"], case["max_border_errors"], case["max_hamming"])
    assert np.array_equal(np.concatenate(wrapped[1]), host["id"]) and np.array_equal(np.concatenate(wrapped[5]), host["code"])


# ---- 4. the allocation poison -----------------------------------------------------------------------------------------------------------
def test_parity_on_poisoned_workspace(dev_ctx, monkeypatch):
    """The second library with CCAL_TEST_POISON_ALLOC=1 (tests/test_gpu_poison.py): corners and margins start as NaN bytes in
    every call; the kernel writes every one of them before the copy back."""
    monkeypatch.setenv("CCAL_TEST_POISON_ALLOC", "1")
    for name in ("sheet d 8 border 2 S 4 uint16", "sheet d 3 border 1 S 1 uint8", "table of 587", "degenerate corners", "three images"):
        check_against_yardstick(raw_decode(dev_ctx, CASES[name]), CASES[name])


# ---- 5. invalid arguments ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(gpu_ctx):
    case = ref.batch_case()
    bad = [dict(d=2), dict(d=9), dict(border=0), dict(border=3), dict(n_codes=0), dict(n_codes=-1), dict(samples=0), dict(samples=5),
           dict(min_contrast=-1.0), dict(min_contrast=float("nan")), dict(min_contrast=float("inf")), dict(max_border=-1),
           dict(max_hamming=-1), dict(max_hamming=37), dict(dtype=2), dict(dtype=-1), dict(w=0), dict(h=-1), dict(n=-1),
           dict(w=65536, h=32768), dict(offs=[1, 1, 1, 2]), dict(offs=[0, 2, 1, 3]), dict(offs=[0, 0, 0, 2 ** 31]), dict(offs=None),
           dict(null=("images",)), dict(null=("codes",)), dict(null=("quads",)), dict(null=("reason",)), dict(null=("id",)),
           dict(null=("rot",)), dict(null=("hamming",))]
    for fn in (gpu_ctx.lib.ccal_decode_tags_batch, gpu_ctx.lib.ccal_decode_tags_dev):
        for change in bad:
            got = raw_decode(gpu_ctx, case, fn=fn, **change)
            assert got["rc"] == _ffi.ERR_INVALID_ARG, change
            assert untouched(got), change
            assert gpu_ctx.last_error()
        # a code of more than d * d bits; at d = 8 every uint64 is a code
        over = dict(case, codes=case["codes"][:3] + (1 << 36,))
        got = raw_decode(gpu_ctx, over, fn=fn)
        assert got["rc"] == _ffi.ERR_INVALID_ARG and untouched(got)
    full = dict(CASES["sheet d 8 border 1 S 1 uint8"])
    full["codes"] = full["codes"] + (2 ** 64 - 1,)
    assert raw_decode(gpu_ctx, full)["rc"] == _ffi.OK
    with pytest.raises(ValueError):
        gpu_ctx.decode_tags_batch(np.zeros((1, 45, 67, 3), dtype=np.uint8), [np.zeros((0, 4, 2))], 36, [1])            # colour
    with pytest.raises(ValueError):
        gpu_ctx.decode_tags_batch(np.zeros((1, 45, 67), dtype=np.uint8), [np.zeros((0, 4, 2))], 35, [1])
    with pytest.raises(ValueError):
        gpu_ctx.decode_tags_batch(np.zeros((2, 45, 67), dtype=np.uint8), [np.zeros((0, 4, 2))], 36, [1])


# ---- 6. the api layer --------------------------------------------------------------------------------------------------------------------
def test_decode_tags_keeps_the_better_of_two_quads_with_one_id(gpu_ctx):
    case = ref.batch_case()                                              # every tag of the sheets is outlined by several quads
    fam = api.TagFamily("toy", 36, case["codes"])
    got = api.decode_tags(list(case["images"]), case["quads_list"], fam, case["border"], case["samples"], case["min_contrast"],
                          case["max_border_errors"], case["max_hamming"], ctx=gpu_ctx)
    assert len(got) == 3 and got[1] == []
    for k in (0, 2):
        best = {}
        for j, r in enumerate(ref.yardstick(case)[k]):
            if r["reason"] == ref.OK and (r["id"] not in best or (r["hamming"], -r["margin"]) < (best[r["id"]]["hamming"], -best[r["id"]]["margin"])):
                best[r["id"]] = r
        assert [t[0] for t in got[k]] == sorted(best) and len(best) < sum(r["reason"] == ref.OK for r in ref.yardstick(case)[k])
        for tag_id, rot, ham, corners in got[k]:
            assert (rot, ham) == (best[tag_id]["rot"], best[tag_id]["hamming"]) and close(corners, best[tag_id]["corners"])
    assert api.decode_tags([], [], fam, ctx=gpu_ctx) == []


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_rendered_aprilgrid_to_frame_features(gpu_ctx, dtype):
    """A rendered 3 x 2 AprilGrid (d = 6, a 40-code family, tags of about 45 px in 320 x 240), division camera at lambda 0 and
    -0.35, tilted 10 and 30 degrees, turned 15 and 100 degrees: the true outlines moved onto the saddles by api.refine_corners,
    decoded, named and looked up on the board."""
    imgs, truth = ref.grid_frames(dtype)
    assert {(f[0], f[1], f[2]) for f in ref.GRID_FRAMES} == {(0.0, 15.0, 10.0), (-0.35, 100.0, 30.0), (-0.35, 15.0, 30.0), (0.0, 100.0, 10.0)}
    fam = api.TagFamily("toy", 36, ref.grid_family().codes)
    board = api.AprilGridBoard(ref.GRID.tag_size_meter, ref.GRID.tag_spacing, ref.GRID.tag_rows, ref.GRID.tag_cols)
    start = [api.FrameFeature(k, (ref.GRID_W, ref.GRID_H), {i: api.FeaturePoint((float(x), float(y)), (0.0, 0.0, 0.0))
                                                             for i, (x, y) in enumerate(truth[k].reshape(-1, 2))}) for k in range(len(imgs))]
    refined = api.refine_corners(list(imgs), start, half_win=ref.GRID_HALF_WIN, ctx=gpu_ctx)
    quads = []
    for f in refined:
        assert f is not None and sorted(f.features) == list(range(24))
        quads.append(np.array([f.features[i].p2d for i in range(24)]).reshape(6, 4, 2))
    contrast = 20.0 * (257 if dtype == np.uint16 else 1)
    results = []
    for shift in (0, 1):
        decoded = api.decode_tags(list(imgs), [np.roll(q, -shift, axis=1) for q in quads], fam, min_contrast=contrast, ctx=gpu_ctx)
        for k, tags in enumerate(decoded):
            assert [(t[0], t[1], t[2]) for t in tags] == [(m, shift, 0) for m in range(6)], (k, shift)
        frames = api.frames_from_tags(decoded, board, (ref.GRID_W, ref.GRID_H), times=[100 + k for k in range(len(imgs))])
        worst = 0.0
        for k, f in enumerate(frames):
            assert f is not None and f.time_ns == 100 + k and f.img_w_h == (ref.GRID_W, ref.GRID_H) and sorted(f.features) == list(range(24))
            for i in range(24):
                assert f.features[i].p3d == board.id_to_3d[i]
                e = float(np.hypot(*(np.array(f.features[i].p2d) - truth[k].reshape(-1, 2)[i])))
                worst = max(worst, e)
                assert e <= 0.2, (k, i, e)
        print(f"shift {shift}: worst distance of a p2d to the projected truth {worst:.4f} px")
        results.append(decoded)
    for a, b in zip(*results):                                           # shifted quads: the same ids and the same corners_out
        assert [t[0] for t in a] == [t[0] for t in b]
        assert all(np.array_equal(x[3], y[3]) for x, y in zip(a, b))
    # a partial view: four tags decode, sixteen corners are below the reference's MIN_CORNERS
    part = api.frames_from_tags([results[0][0][:4]], board, (ref.GRID_W, ref.GRID_H))
    assert part == [None]
