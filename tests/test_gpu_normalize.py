"""GPU: local contrast normalisation (ccal_normalize_dev; ccal_kernels_normalize.hip) against tests/normalize_ref.py, the numpy
statement of the rule in include/ccal.h.

Every comparison with the yardstick is exact equality, between torch blocks with 64 guard bytes on each side under two fill values.
Round trips: the eight degraded frames of normalize_ref are made on the host and uploaded; detect_checkerboards_dev / detect_tags_dev
on the plain block find no board and fewer than six tags, after normalize_dev into a second block they find every board and all six
tags at Hamming distance 0, every corner within 1.5 x the worst error the numpy chains reach on the yardstick's normalised frames
(normalize_ref.RT_NORM_*_WORST)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as dr  # noqa: E402
import normalize_ref as nr  # noqa: E402
import tag_ref as tr  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in nr.parity_cases()}
GUARD = 64


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def _norm(o):
    return api.NormalizeOpts(**o)


def _normalize_dev(ctx, src, dst_dtype, o, fill):
    """normalize_dev between two torch blocks with 64 guard bytes on each side, every byte of the destination block and of the
    source's guards set to `fill` beforehand: (images, all four guards and the source intact)."""
    import torch
    n, H, W = src.shape
    dt = np.dtype(dst_dtype)
    raw = np.full(src.nbytes + 2 * GUARD, fill, dtype=np.uint8)
    raw[GUARD:GUARD + src.nbytes] = src.reshape(-1).view(np.uint8)
    s_block = torch.from_numpy(raw).cuda()
    d_block = torch.full((n * H * W * dt.itemsize + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.normalize_dev(s_block.data_ptr() + GUARD, d_block.data_ptr() + GUARD, _code(src.dtype), _code(dt), W, H, n, _norm(o))
    ctx.sync()
    host = d_block.cpu().numpy()
    intact = bool((host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all() and np.array_equal(s_block.cpu().numpy(), raw))
    return host[GUARD:-GUARD].copy().view(dt).reshape(n, H, W), intact


# ---- normalize_dev against the yardstick -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_normalize_dev_equals_the_yardstick(gpu_ctx, name):
    case = CASES[name]
    src = nr.source(case)
    want = nr.normalize(src, case["dst"], case["opts"])
    for fill in (0x5A, 0xA5):
        got, intact = _normalize_dev(gpu_ctx, src, case["dst"], case["opts"], fill)
        assert intact, "bytes outside the destination were written, or the source was"
        bad = got != want
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


def test_the_cases_cover_what_they_claim():
    cases = nr.parity_cases()
    assert {(c["src"].name, c["dst"].name) for c in cases} == {(a, b) for a in ("uint8", "uint16") for b in ("uint8", "uint16")}
    for shape in ((1, 1), (67, 45), (130, 67)):
        assert {c["opts"]["radius"] for c in cases if (c["width"], c["height"]) == shape} >= ({1, 16} if shape == (1, 1) else {1, 5, 16, 32})
    assert {c["opts"]["min_sigma"] for c in cases} >= {0.0, 4.0, 255.0} and {c["opts"]["amp"] for c in cases} >= {0.0, 64.0, 1000.0}
    assert any(c["n"] > 65535 for c in cases) and any(c["width"] == 1 and c["height"] > 1 for c in cases)
    halves = CASES["halves r 32"]
    src = nr.source(halves).astype(np.int64)
    mid = src[0, :, halves["width"] // 2 - 1:halves["width"] // 2 + 1]
    assert mid.min() == 0 and mid.max() == 65535
    d, s = nr.terms(nr.source(halves), 32, 0.0)
    assert int(s.max()) ** 2 > 2 ** 53                                   # v beyond what an f64 holds exactly
    sat = nr.normalize(nr.source(CASES["67 x 45 amp 1000"]), np.uint16, CASES["67 x 45 amp 1000"]["opts"])
    assert (sat == 0).mean() > 0.2 and (sat == 65535).mean() > 0.2         # the clamp is exercised at both ends
    assert (nr.normalize(nr.source(CASES["67 x 45 amp 0"]), np.uint8, CASES["67 x 45 amp 0"]["opts"]) == 128).all()


def test_a_constant_image_gives_128(gpu_ctx):
    for name, level in (("constant u8", 128), ("constant u16", 32896)):
        got, intact = _normalize_dev(gpu_ctx, nr.source(CASES[name]), CASES[name]["dst"], CASES[name]["opts"], 0x5A)
        assert intact and (got == level).all()


def test_u8_and_257_times_u16_sources_give_equal_output(gpu_ctx):
    case = CASES["67 x 45 r 5"]
    src = nr.source(case)
    wide = src.astype(np.uint16) * np.uint16(257)
    for dst in (np.uint8, np.uint16):
        a, ia = _normalize_dev(gpu_ctx, src, dst, case["opts"], 0x5A)
        b, ib = _normalize_dev(gpu_ctx, wide, dst, case["opts"], 0x5A)
        assert ia and ib and np.array_equal(a, b)


def test_two_runs_are_equal_and_an_image_does_not_depend_on_its_batch(gpu_ctx):
    case = CASES["65 images 9 x 5"]
    src = nr.source(case)
    a, _ = _normalize_dev(gpu_ctx, src, case["dst"], case["opts"], 0x5A)
    b, _ = _normalize_dev(gpu_ctx, src, case["dst"], case["opts"], 0xA5)
    assert np.array_equal(a, b)
    for k in (0, 1, 31, 63, 64):
        alone, intact = _normalize_dev(gpu_ctx, src[k:k + 1], case["dst"], case["opts"], 0x5A)
        assert intact and np.array_equal(alone[0], a[k]), k


def test_zero_images_and_the_default_options(gpu_ctx):
    gpu_ctx.normalize_dev(0, 0, _ffi.PIX_U8, _ffi.PIX_U8, 8, 8, 0)          # a successful no-op
    import torch
    case = CASES["67 x 45 r 16 u8 to u16"]
    src = nr.source(case)
    s_block = torch.from_numpy(src.copy()).cuda()
    d_block = torch.zeros(src.shape, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.normalize_dev(s_block.data_ptr(), d_block.data_ptr(), _ffi.PIX_U8, _ffi.PIX_U16, case["width"], case["height"], case["n"])
    gpu_ctx.sync()
    assert np.array_equal(d_block.cpu().numpy().view(np.uint16), nr.normalize(src, np.uint16, nr.opts()))


# ---- round trips: frames the plain chains lose ----------------------------------------------------------------------------------------------
def _upload(img):
    import torch
    block = torch.from_numpy(np.ascontiguousarray(img)[None].copy()).cuda()
    out = torch.zeros_like(block)
    torch.cuda.synchronize()
    return block, out


@pytest.mark.parametrize("k", range(len(nr.RT_BOARD_CASES)))
def test_round_trip_checkerboard(gpu_ctx, k):
    img, truth = nr.rt_board(k)
    H, W = img.shape
    block, out = _upload(img)
    detect = lambda ptr: gpu_ctx.detect_checkerboards_dev(ptr, _ffi.PIX_U8, W, H, 1, dr.BOARD_COLS, dr.BOARD_ROWS, half_win=dr.BOARD_HALF_WIN)[0]
    assert not detect(block.data_ptr())[0], "the plain frame gave a board: the degraded frame is not the one the figures were recorded on"
    gpu_ctx.normalize_dev(block.data_ptr(), out.data_ptr(), _ffi.PIX_U8, _ffi.PIX_U8, W, H, 1, api.NormalizeOpts())
    found, xy, _, _ = detect(out.data_ptr())
    assert found, k
    err = nr.board_error(xy, truth)
    print(f"board case {k}: worst corner error {err:.5f} px, bound {nr.rt_bound(nr.RT_NORM_BOARD_WORST[k]):.5f}")
    assert err <= nr.rt_bound(nr.RT_NORM_BOARD_WORST[k]), (k, err)


@pytest.mark.parametrize("k", range(len(nr.RT_GRID_CASES)))
def test_round_trip_aprilgrid(gpu_ctx, k):
    img, quads = nr.rt_grid(k)
    H, W = img.shape
    fam = tr.grid_family()
    block, out = _upload(img)
    detect = lambda ptr: gpu_ctx.detect_tags_dev(ptr, _ffi.PIX_U8, W, H, 1, fam.bits, fam.codes, half_win=tr.GRID_HALF_WIN)[0]
    assert len(detect(block.data_ptr())[0]) < 6
    gpu_ctx.normalize_dev(block.data_ptr(), out.data_ptr(), _ffi.PIX_U8, _ffi.PIX_U8, W, H, 1, api.NormalizeOpts())
    ids, rot, ham, corners, *_ = detect(out.data_ptr())
    assert [int(t) for t in ids] == list(range(6)) and not np.any(ham), (k, list(ids), list(ham))
    err = max(float(np.linalg.norm(c - quads[int(t)], axis=1).max()) for t, c in zip(ids, corners))
    print(f"grid case {k}: worst corner error {err:.5f} px, bound {nr.rt_bound(nr.RT_NORM_GRID_WORST[k]):.5f}")
    assert err <= nr.rt_bound(nr.RT_NORM_GRID_WORST[k]), (k, err)


# ---- error codes ----------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, src_dtype=_ffi.PIX_U8, dst_dtype=_ffi.PIX_U8, w=8, h=8, n=1, src=True, dst=True, norm=True, overlap=None, **o):
    """ccal_normalize_dev with one argument changed, on a block of 0x5A bytes: (status, the message, the block untouched)."""
    import torch
    block = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s_ptr = block.data_ptr() + 256
    d_ptr = block.data_ptr() + 2048 if overlap is None else s_ptr + overlap
    no = _ffi.NormalizeOpts(radius=o.get("radius", 16), min_sigma=o.get("min_sigma", 4.0), amp=o.get("amp", 64.0))
    rc = ctx.lib.ccal_normalize_dev(ctx.handle, src_dtype, dst_dtype, w, h, n, C.c_void_p(s_ptr) if src else None, C.c_void_p(d_ptr) if dst else None,
                                    C.byref(no) if norm else None)
    msg = ctx.last_error()
    ctx.sync()
    return rc, msg, bool((block.cpu().numpy() == 0x5A).all())


def test_error_codes(gpu_ctx):
    INV = _ffi.ERR_INVALID_ARG
    rc, _, untouched = _raw(gpu_ctx)
    assert rc == _ffi.OK and not untouched
    assert _raw(gpu_ctx, n=0, src=False, dst=False)[::2] == (_ffi.OK, True)
    for kw, word in ((dict(norm=False), "norm"), (dict(radius=0), "radius"), (dict(radius=33), "radius"), (dict(radius=-1), "radius"),
                     (dict(min_sigma=-0.1), "min_sigma"), (dict(min_sigma=255.5), "min_sigma"), (dict(min_sigma=float("nan")), "min_sigma"),
                     (dict(amp=-1.0), "amp"), (dict(amp=float("inf")), "amp"), (dict(amp=float("nan")), "amp"),
                     (dict(src_dtype=2), "src_dtype"), (dict(dst_dtype=-1), "dst_dtype"), (dict(w=0), "size"), (dict(h=-1), "size"),
                     (dict(n=-1), "size"), (dict(w=65536, h=32768), "2^31 - 1 pixels"), (dict(src=False), "src_dev"), (dict(dst=False), "dst_dev"),
                     (dict(overlap=0), "overlap"), (dict(overlap=63), "overlap"), (dict(overlap=-63), "overlap"),
                     (dict(src_dtype=_ffi.PIX_U16, overlap=127), "overlap"), (dict(dst_dtype=_ffi.PIX_U16, overlap=-127), "overlap")):
        rc, msg, untouched = _raw(gpu_ctx, **kw)
        assert rc == INV and word in msg and msg.startswith("ccal_normalize_dev: ") and untouched, (kw, rc, msg, untouched)
    assert _raw(gpu_ctx, overlap=64)[0] == _ffi.OK and _raw(gpu_ctx, overlap=-64)[0] == _ffi.OK       # blocks that touch
    assert _raw(gpu_ctx, radius=1)[0] == _ffi.OK and _raw(gpu_ctx, radius=32, min_sigma=255.0, amp=0.0)[0] == _ffi.OK
    assert _raw(gpu_ctx)[0] == _ffi.OK                                                      # the context is as good as before
