"""GPU: grey frames from colour and raw Bayer frames (ccal_grey_dev; ccal_kernels_grey.hip) against tests/grey_ref.py, the numpy
statement of the rule in include/ccal.h.

Every comparison with the yardstick is exact equality, between torch blocks with 64 guard bytes on each side under two fill values.
Round trips: the board fixture as a tinted RGB frame and as a mosaic, at bin 1 and - seen by a camera of twice the size - at bin 2,
through grey_dev into detect_checkerboards_dev: the board is found and every corner lies within 1.5 x the worst error the numpy
chain reaches on the yardstick's grey frame (grey_ref.RT_WORST)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref as dr  # noqa: E402
import grey_ref as gr  # noqa: E402
import normalize_ref as nr  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, engine  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in gr.parity_cases()}
GUARD = 64


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def _grey_dev(ctx, src, layout, dst_dtype, o, fill, skew=0):
    """grey_dev between two torch blocks with 64 guard bytes on each side, every byte of the destination block and of the source's
    guards set to `fill` beforehand; skew: both blocks start that many bytes off a dword boundary.  (images, all four guards and the
    source intact)."""
    import torch
    n, H, W = src.shape[:3]
    dt = np.dtype(dst_dtype)
    Wo, Ho = engine.grey_out_size(W, H, o["bin"])
    raw = np.full(src.nbytes + 2 * GUARD + skew, fill, dtype=np.uint8)
    raw[GUARD + skew:GUARD + skew + src.nbytes] = src.reshape(-1).view(np.uint8)
    s_block = torch.from_numpy(raw).cuda()
    d_block = torch.full((n * Ho * Wo * dt.itemsize + 2 * GUARD + skew,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert s_block.data_ptr() % 4 == 0 and d_block.data_ptr() % 4 == 0
    ctx.grey_dev(s_block.data_ptr() + GUARD + skew, d_block.data_ptr() + GUARD + skew, api.LAYOUTS[layout], _code(src.dtype), _code(dt), W, H, n,
                 api.GreyOpts(**o))
    ctx.sync()
    host = d_block.cpu().numpy()
    intact = bool((host[:GUARD + skew] == fill).all() and (host[-GUARD:] == fill).all() and np.array_equal(s_block.cpu().numpy(), raw))
    return host[GUARD + skew:-GUARD].copy().view(dt).reshape(n, Ho, Wo), intact


# ---- grey_dev against the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_grey_dev_equals_the_yardstick(gpu_ctx, name):
    case = CASES[name]
    src = gr.source(case)
    want = gr.grey(src, case["layout"], case["dst"], case["opts"])
    for fill in (0x5A, 0xA5):
        got, intact = _grey_dev(gpu_ctx, src, case["layout"], case["dst"], case["opts"], fill)
        assert intact, "bytes outside the destination were written, or the source was"
        bad = got != want
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


@pytest.mark.parametrize("name,skew", [("67 x 45 rgb u8 to u8 bin 1", 1), ("67 x 45 rgb u8 to u8 bin 2", 3), ("67 x 45 rgb u16 to u16 bin 1", 2),
                                       ("67 x 45 rgb u16 to u8 bin 4", 2), ("67 x 45 bayer_grbg u8 to u8 bin 1", 1),
                                       ("67 x 45 bayer_rggb u8 to u16 bin 2", 2), ("130 x 67 rgb u8 to u8 bin 1", 1)])
def test_blocks_off_a_dword_boundary(gpu_ctx, name, skew):
    case = CASES[name]
    src = gr.source(case)
    want = gr.grey(src, case["layout"], case["dst"], case["opts"])
    for fill in (0x5A, 0xA5):
        got, intact = _grey_dev(gpu_ctx, src, case["layout"], case["dst"], case["opts"], fill, skew=skew)
        assert intact, "bytes outside the destination were written, or the source was"
        assert np.array_equal(got, want), (name, skew, int((got != want).sum()))


# ---- the consequences, on the device --------------------------------------------------------------------------------------------------------
def test_grey_at_bin_1_with_equal_types_is_a_copy(gpu_ctx):
    for dtype in (np.uint8, np.uint16):
        src = gr.source(CASES["67 x 45 grey u8 to u8 bin 1" if dtype == np.uint8 else "67 x 45 grey u16 to u16 bin 1"])
        got, intact = _grey_dev(gpu_ctx, src, "grey", dtype, gr.opts(), 0x5A)
        assert intact and np.array_equal(got, src)


@pytest.mark.parametrize("layout", gr.LAYOUTS)
def test_u8_and_257_times_u16_sources_give_equal_output(gpu_ctx, layout):
    src = gr.source(CASES[f"67 x 45 {layout} u8 to u8 bin 1"])
    wide = src.astype(np.uint16) * np.uint16(257)
    for b in (1, 2, 4):
        for dst in (np.uint8, np.uint16):
            a, ia = _grey_dev(gpu_ctx, src, layout, dst, gr.opts(bin=b), 0x5A)
            w, iw = _grey_dev(gpu_ctx, wide, layout, dst, gr.opts(bin=b), 0x5A)
            assert ia and iw and np.array_equal(a, w), (b, dst)


def test_rgba_against_rgb_and_bgr_against_rgb(gpu_ctx):
    for dtype in (np.uint8, np.uint16):
        short = "u8" if dtype == np.uint8 else "u16"
        rgb = gr.source(CASES[f"67 x 45 rgb {short} to {short} bin 1"])
        alpha = gr.source(CASES[f"67 x 45 grey {short} to {short} bin 1"])
        for b in (1, 2, 4):
            o = gr.opts(bin=b)
            want, ok = _grey_dev(gpu_ctx, rgb, "rgb", dtype, o, 0x5A)
            assert ok
            for layout, block in (("bgr", rgb[..., ::-1]), ("rgba", np.concatenate([rgb, alpha[..., None]], axis=3)),
                                  ("rgba", np.concatenate([rgb, np.zeros_like(alpha)[..., None]], axis=3)),
                                  ("bgra", np.concatenate([rgb[..., ::-1], alpha[..., None]], axis=3))):
                got, ok = _grey_dev(gpu_ctx, np.ascontiguousarray(block), layout, dtype, o, 0x5A)
                assert ok and np.array_equal(got, want), (layout, short, b)


@pytest.mark.parametrize("name", ["65 images 9 x 5 rgb", "65 images 9 x 5 bayer_grbg"])
def test_two_runs_are_equal_and_an_image_does_not_depend_on_its_batch(gpu_ctx, name):
    case = CASES[name]
    src = gr.source(case)
    a, _ = _grey_dev(gpu_ctx, src, case["layout"], case["dst"], case["opts"], 0x5A)
    b, _ = _grey_dev(gpu_ctx, src, case["layout"], case["dst"], case["opts"], 0xA5)
    assert np.array_equal(a, b)
    for k in (0, 1, 31, 63, 64):
        alone, intact = _grey_dev(gpu_ctx, src[k:k + 1], case["layout"], case["dst"], case["opts"], 0x5A)
        assert intact and np.array_equal(alone[0], a[k]), k


def test_zero_images_and_the_default_options(gpu_ctx):
    gpu_ctx.grey_dev(0, 0, _ffi.LAYOUT_RGB, _ffi.PIX_U8, _ffi.PIX_U8, 8, 8, 0)          # a successful no-op
    import torch
    case = CASES["67 x 45 rgb u8 to u16 bin 1"]
    src = gr.source(case)
    s_block = torch.from_numpy(src.copy()).cuda()
    d_block = torch.zeros(src.shape[:3], dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.grey_dev(s_block.data_ptr(), d_block.data_ptr(), _ffi.LAYOUT_RGB, _ffi.PIX_U8, _ffi.PIX_U16, case["width"], case["height"], case["n"])
    gpu_ctx.sync()
    assert np.array_equal(d_block.cpu().numpy().view(np.uint16), gr.grey(src, "rgb", np.uint16, gr.opts()))


# ---- round trips: the board as a colour frame and as a mosaic ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(gr.RT_CASES)))
def test_round_trip_checkerboard(gpu_ctx, k):
    import torch
    src, layout, b, truth = gr.rt_source(k)
    H, W = src.shape[:2]
    Wo, Ho = engine.grey_out_size(W, H, b)
    block = torch.from_numpy(np.ascontiguousarray(src)[None].copy()).cuda()
    out = torch.zeros((1, Ho, Wo), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.grey_dev(block.data_ptr(), out.data_ptr(), api.LAYOUTS[layout], _ffi.PIX_U8, _ffi.PIX_U8, W, H, 1, api.GreyOpts(bin=b))
    found, xy, _, _ = gpu_ctx.detect_checkerboards_dev(out.data_ptr(), _ffi.PIX_U8, Wo, Ho, 1, dr.BOARD_COLS, dr.BOARD_ROWS, half_win=dr.BOARD_HALF_WIN)[0]
    assert np.array_equal(out.cpu().numpy()[0], gr.rt_grey(k)[0]), "the device's grey frame is not the yardstick's"
    assert found, gr.RT_CASES[k]
    err = nr.board_error(xy, truth)
    print(f"round trip {gr.RT_CASES[k]}: worst corner error {err:.5f} px, bound {gr.rt_bound(gr.RT_WORST[k]):.5f}")
    assert err <= gr.rt_bound(gr.RT_WORST[k]), (k, err)


# ---- error codes ----------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, layout=_ffi.LAYOUT_RGB, src_dtype=_ffi.PIX_U8, dst_dtype=_ffi.PIX_U8, w=8, h=8, n=1, src=True, dst=True, opts=True, overlap=None, **o):
    """ccal_grey_dev with one argument changed, on a block of 0x5A bytes whose bytes 256 .. 319 are 0x3C (the grey frame of a frame of
    0x5A bytes is 0x5A again: a call that ran shows on the 0x3C part alone): (status, the message, the block untouched).  The source
    is at byte 256 of the block, the destination at byte 2048 or `overlap` bytes from the source."""
    import torch
    before = np.full(4096, 0x5A, dtype=np.uint8)
    before[256:320] = 0x3C
    block = torch.from_numpy(before.copy()).cuda()
    torch.cuda.synchronize()
    s_ptr = block.data_ptr() + 256
    d_ptr = block.data_ptr() + 2048 if overlap is None else s_ptr + overlap
    go = _ffi.GreyOpts(bin=o.get("bin", 1), w_r=o.get("w_r", 19595), w_g=o.get("w_g", 38470), w_b=o.get("w_b", 7471))
    rc = ctx.lib.ccal_grey_dev(ctx.handle, layout, src_dtype, dst_dtype, w, h, n, C.c_void_p(s_ptr) if src else None, C.c_void_p(d_ptr) if dst else None,
                               C.byref(go) if opts else None)
    msg = ctx.last_error()
    ctx.sync()
    return rc, msg, bool(np.array_equal(block.cpu().numpy(), before))


def test_error_codes(gpu_ctx):
    INV = _ffi.ERR_INVALID_ARG
    rc, _, untouched = _raw(gpu_ctx)
    assert rc == _ffi.OK and not untouched
    assert _raw(gpu_ctx, n=0, src=False, dst=False)[::2] == (_ffi.OK, True)
    RGGB, U16 = _ffi.LAYOUT_BAYER_RGGB, _ffi.PIX_U16
    for kw, word in ((dict(opts=False), "opts"), (dict(layout=-1), "layout"), (dict(layout=9), "layout"),
                     (dict(bin=0), "bin"), (dict(bin=3), "bin"), (dict(bin=8), "bin"), (dict(bin=-2), "bin"),
                     (dict(w_r=-1, w_g=65537, w_b=0), "negative"), (dict(w_g=-1, w_r=65537, w_b=0), "negative"), (dict(w_b=-7471), "negative"),
                     (dict(w_b=7470), "sum"), (dict(w_r=19596), "sum"), (dict(w_r=0, w_g=0, w_b=0), "sum"),
                     (dict(w_r=2 ** 31 - 1, w_g=2 ** 31 - 1, w_b=65538), "sum"),
                     (dict(src_dtype=2), "src_dtype"), (dict(dst_dtype=-1), "dst_dtype"), (dict(w=0), "size"), (dict(h=-1), "size"),
                     (dict(n=-1), "size"), (dict(w=65536, h=32768), "2^31 - 1 pixels"), (dict(w=65536, h=32768, bin=4), "2^31 - 1 pixels"),
                     (dict(w=1, bin=2), "below bin"), (dict(h=3, bin=4), "below bin"),
                     (dict(layout=RGGB, w=1), "Bayer"), (dict(layout=_ffi.LAYOUT_BAYER_GBRG, h=1), "Bayer"),
                     (dict(src=False), "src_dev"), (dict(dst=False), "dst_dev"),
                     (dict(overlap=0), "overlap"), (dict(overlap=191), "overlap"), (dict(overlap=-63), "overlap"),
                     (dict(src_dtype=U16, overlap=383), "overlap"), (dict(dst_dtype=U16, overlap=-127), "overlap"),
                     (dict(bin=2, overlap=-15), "overlap"), (dict(layout=RGGB, overlap=63), "overlap"),
                     (dict(layout=_ffi.LAYOUT_BGRA, src_dtype=U16, overlap=511), "overlap")):
        rc, msg, untouched = _raw(gpu_ctx, **kw)
        assert rc == INV and word in msg and msg.startswith("ccal_grey_dev: ") and untouched, (kw, rc, msg, untouched)
    # blocks that touch: 8 x 8 RGB u8 is 192 bytes, its grey frame 64, at bin 2 16
    assert _raw(gpu_ctx, overlap=192)[0] == _ffi.OK and _raw(gpu_ctx, overlap=-64)[0] == _ffi.OK
    assert _raw(gpu_ctx, bin=2, overlap=-16)[0] == _ffi.OK and _raw(gpu_ctx, layout=RGGB, overlap=64)[0] == _ffi.OK
    assert _raw(gpu_ctx, w_r=65536, w_g=0, w_b=0)[0] == _ffi.OK and _raw(gpu_ctx, layout=RGGB, w=2, h=2)[0] == _ffi.OK
    assert _raw(gpu_ctx)[0] == _ffi.OK                                                      # the context is as good as before
