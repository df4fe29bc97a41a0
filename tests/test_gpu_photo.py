"""GPU: the photometric stage (ccal_photo_apply_dev, ccal_render_photo_targets / _dev; ccal_kernels_photo.hip) against
tests/photo_ref.py, the numpy statement of the rule in include/ccal.h.

Every comparison with the yardstick is exact equality, with the library's own tables (ccal_photo_tables; tests/test_photo_cpu.py
holds those to numpy).  The rendered cases put the device's own uint16 ideal render through the yardstick, so that the render rule's
near pixels do not enter.  Round trips at 512 x 512 under synth.GT_PARAMS: render_targets_dev(photo) feeds
detect_checkerboards_dev / detect_tags_dev without the images touching the host; every board and tag is found, every corner within
1.5 x the worst error the numpy chains reach on the yardstick's images of the same poses (photo_ref.RT_PHOTO_*_WORST)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import photo_ref as pr  # noqa: E402
import render_ref as rr  # noqa: E402
from test_gpu_render import _target  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, engine  # noqa: E402
from camera_intrinsic_calibration_rs_amd.engine import CcalError  # noqa: E402

pytestmark = pytest.mark.gpu

APPLY = {c["name"]: c for c in pr.apply_cases()}
RENDER = {c["name"]: c for c in rr.parity_cases()}
NAMES = {rr.UCM: "ucm", rr.EUCM: "eucm", rr.KB4: "kb4", rr.OPENCV5: "opencv5"}
NOISY = pr.opts(blur_sigma=0.8, vignette=0.3, gain=1.2, noise_read=2.5, noise_shot=0.08, seed=31, first_index=2)
GUARD = 64


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def _photo(o):
    return api.PhotoOpts(**o)


def _yard(src, dst_dtype, o):
    return pr.apply(src, dst_dtype, engine.photo_tables(_photo(o)), o)


def _apply_dev(ctx, src, dst_dtype, o, fill):
    """photo_apply_dev between two torch blocks with 64 guard bytes on each side, every byte of the destination block and of the
    source's guards set to `fill` beforehand: (images, all four guards and the source intact)."""
    import torch
    n, H, W = src.shape
    dt = np.dtype(dst_dtype)
    raw = np.full(src.nbytes + 2 * GUARD, fill, dtype=np.uint8)
    raw[GUARD:GUARD + src.nbytes] = src.reshape(-1).view(np.uint8)
    s_block = torch.from_numpy(raw).cuda()
    d_block = torch.full((n * H * W * dt.itemsize + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.photo_apply_dev(s_block.data_ptr() + GUARD, d_block.data_ptr() + GUARD, _code(src.dtype), _code(dt), W, H, n, _photo(o))
    ctx.sync()
    host = d_block.cpu().numpy()
    intact = bool((host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all() and np.array_equal(s_block.cpu().numpy(), raw))
    return host[GUARD:-GUARD].copy().view(dt).reshape(n, H, W), intact


def _render(ctx, case, photo=None, dtype=None, poses=None):
    return ctx.render_targets_batch(case["model"], case["params"], case["width"], case["height"], case["poses"] if poses is None else poses,
                                    _target(case["target"]), case["dtype"] if dtype is None else dtype, case["ss"],
                                    margin=case["target"]["margin"], photo=None if photo is None else _photo(photo), **case["opts"])


# ---- photo_apply_dev on random blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(APPLY))
def test_apply_dev_equals_the_yardstick(gpu_ctx, name):
    case = APPLY[name]
    src = pr.source(case)
    want = _yard(src, case["dst"], case["opts"])
    for fill in (0x5A, 0xA5):
        got, intact = _apply_dev(gpu_ctx, src, case["dst"], case["opts"], fill)
        assert intact, "bytes outside the destination were written, or the source was"
        bad = got != want
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


def test_the_cases_cover_what_they_claim():
    cases = pr.apply_cases()
    assert {(c["src"].name, c["dst"].name) for c in cases} == {(a, b) for a in ("uint8", "uint16") for b in ("uint8", "uint16")}
    on = lambda c: tuple(k for k in ("blur_sigma", "vignette", "gain", "noise_read", "noise_shot") if c["opts"][k] != pr.OFF[k])
    alone = {on(c) for c in cases if len(on(c)) == 1}
    assert alone == {("blur_sigma",), ("vignette",), ("gain",), ("noise_read",), ("noise_shot",)}
    assert any(len(on(c)) == 5 for c in cases) and any(len(on(c)) == 0 for c in cases)
    assert {engine.photo_tables(_photo(c["opts"]))[0] for c in cases} >= {0, 4, 9, 16}
    sat = APPLY["67 x 45 gain 3"]
    assert (_yard(pr.source(sat), sat["dst"], sat["opts"]) == 65535).mean() > 0.5       # the clamp at saturation is exercised


def test_apply_dev_identity_and_zero_images(gpu_ctx):
    case = APPLY["67 x 45 off"]
    src = pr.source(case)
    got, intact = _apply_dev(gpu_ctx, src, np.uint16, case["opts"], 0x5A)
    assert intact and np.array_equal(got, src)
    gpu_ctx.photo_apply_dev(0, 0, _ffi.PIX_U8, _ffi.PIX_U8, 8, 8, 0, _photo(pr.opts()))   # a successful no-op


# ---- rendered ideals --------------------------------------------------------------------------------------------------------------------
def _odd_u16():
    return next(c for c in rr.parity_cases() if c["dtype"] == np.uint16 and c["width"] % 2 == 1 and c["width"] > 1)


@pytest.mark.parametrize("pick", ["board", "grid", "odd u16"])
def test_rendered_ideals_through_the_yardstick(gpu_ctx, pick):
    case = {"board": RENDER["board ucm 130 x 67 s 3"], "grid": RENDER["grid kb4"], "odd u16": _odd_u16()}[pick]
    ideal = _render(gpu_ctx, case, dtype=np.uint16)
    for o in (pr.opts(**pr.ALL), NOISY, pr.opts(blur_sigma=5.0, noise_shot=0.1, seed=3)):
        got = _render(gpu_ctx, case, photo=o)
        assert got.dtype == case["dtype"] and np.array_equal(got, _yard(ideal, case["dtype"], o)), (case["name"], o)


@pytest.mark.parametrize("name", ["board ucm", "grid opencv5 130 x 67 s 1 first_id 4", "board kb4 1 x 1"])
def test_identity_with_all_effects_off(gpu_ctx, name):
    case = RENDER[name]
    assert np.array_equal(_render(gpu_ctx, case, photo=pr.opts(), dtype=np.uint16), _render(gpu_ctx, case, dtype=np.uint16))


def test_the_api_wrappers_take_photo(gpu_ctx):
    case = RENDER["board eucm"]
    model = api.GenericModel("eucm", case["params"], case["width"], case["height"])
    got = api.render_checkerboard(model, case["poses"], rr.BOARD[:2], rr.BOARD[2], dtype=case["dtype"], ctx=gpu_ctx, photo=_photo(NOISY))
    assert np.array_equal(got, _render(gpu_ctx, case, photo=NOISY))
    case = RENDER["grid kb4"]
    model = api.GenericModel("kb4", case["params"], case["width"], case["height"])
    fam = api.TagFamily("seeded", rr.family().bits, rr.family().codes)
    got = api.render_aprilgrid(model, case["poses"], api.AprilGridBoard(0.03, 0.3, 2, 3), fam, dtype=case["dtype"], ctx=gpu_ctx, photo=_photo(NOISY))
    assert np.array_equal(got, _render(gpu_ctx, case, photo=NOISY))


# ---- batches, chunks, guards, the device form --------------------------------------------------------------------------------------------
def test_two_runs_are_equal_and_an_image_does_not_depend_on_its_batch(gpu_ctx):
    case = RENDER["grid eucm 65 images s 1"]
    a, b = _render(gpu_ctx, case, photo=NOISY), _render(gpu_ctx, case, photo=NOISY)
    assert np.array_equal(a, b)
    assert not np.array_equal(a[0], _render(gpu_ctx, case, photo=dict(NOISY, seed=32), poses=case["poses"][:1])[0])
    for k in (0, 1, 31, 63, 64):
        alone = _render(gpu_ctx, case, photo=dict(NOISY, first_index=NOISY["first_index"] + k), poses=case["poses"][k:k + 1])
        assert np.array_equal(alone[0], a[k]), k


def test_a_batch_cut_into_chunks(dev_ctx, gpu_ctx, monkeypatch):
    """The second library reads the chunk limit from CCAL_TEST_RENDER_CHUNK_BYTES (tests only); with the photometric stage it counts
    the bytes of the uint16 ideal images: one byte is an image per chunk, 7 x 2 x 67 x 45 bytes seven per chunk (the last of 2)."""
    case = RENDER["grid eucm 65 images s 1"]
    want = _render(gpu_ctx, case, photo=NOISY)
    assert np.array_equal(_render(dev_ctx, case, photo=NOISY), want)
    for limit in ("1", str(7 * 2 * 67 * 45)):
        monkeypatch.setenv("CCAL_TEST_RENDER_CHUNK_BYTES", limit)
        assert np.array_equal(_render(dev_ctx, case, photo=NOISY), want), limit


def test_under_the_slice_guards(dev_ctx, monkeypatch):
    """The call's block with a guard round every slice (tests/test_gpu_guard.py): CCAL_OK and equal bytes, whole and in chunks."""
    for case, limit in ((RENDER["grid eucm 65 images s 1"], str(7 * 2 * 67 * 45)), (_odd_u16(), None), (RENDER["board kb4 1 x 1"], None)):
        monkeypatch.delenv("CCAL_TEST_GUARD_SLICES", raising=False)
        monkeypatch.delenv("CCAL_TEST_RENDER_CHUNK_BYTES", raising=False)
        plain = _render(dev_ctx, case, photo=NOISY)
        monkeypatch.setenv("CCAL_TEST_GUARD_SLICES", "1")
        if limit:
            monkeypatch.setenv("CCAL_TEST_RENDER_CHUNK_BYTES", limit)
        assert np.array_equal(_render(dev_ctx, case, photo=NOISY), plain), case["name"]


def _render_dev(ctx, case, photo, fill):
    import torch
    n, H, W = len(case["poses"]), case["height"], case["width"]
    nbytes = n * H * W * case["dtype"].itemsize
    block = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_targets_dev(block.data_ptr() + GUARD, case["model"], case["params"], _code(case["dtype"]), W, H, case["poses"],
                           _target(case["target"]), case["ss"], margin=case["target"]["margin"], photo=_photo(photo), **case["opts"])
    ctx.sync()
    host = block.cpu().numpy()
    guards = bool((host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all())
    return host[GUARD:-GUARD].copy().view(case["dtype"]).reshape(n, H, W), guards


@pytest.mark.parametrize("name", ["board ucm", "grid kb4", "grid opencv5 130 x 67 s 1 first_id 4", "board kb4 1 x 1", "grid eucm 65 images s 1"])
def test_dev_form_writes_every_pixel_and_nothing_else(gpu_ctx, name):
    case = RENDER[name]
    host = _render(gpu_ctx, case, photo=NOISY)
    for fill in (0x5A, 0xA5):
        dev, guards = _render_dev(gpu_ctx, case, NOISY, fill)
        assert guards, "bytes outside the block were written"
        assert np.array_equal(dev, host)


# ---- round trips under the four GT lenses, degraded ---------------------------------------------------------------------------------------
def _block(n):
    import torch
    block = torch.zeros((n, rr.RT_SIZE, rr.RT_SIZE), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return block


@pytest.mark.parametrize("m", [rr.UCM, rr.EUCM, rr.KB4, rr.OPENCV5], ids=lambda m: NAMES[m])
def test_round_trip_checkerboard(gpu_ctx, oracle, m):
    p, poses, S = rr.gt_params(m), pr.rt_board_poses(m), rr.RT_SIZE
    block = _block(len(poses))
    gpu_ctx.render_targets_dev(block.data_ptr(), m, p, _ffi.PIX_U8, S, S, poses, engine.checkerboard_target(*rr.BOARD), photo=_photo(pr.RT_PHOTO))
    res = gpu_ctx.detect_checkerboards_dev(block.data_ptr(), _ffi.PIX_U8, S, S, len(poses), rr.BOARD[0], rr.BOARD[1], half_win=rr.RT_BOARD_HALF_WIN)
    for k, (found, xy, _, _) in enumerate(res):
        assert found, (NAMES[m], k)
        err = rr.board_error(xy, rr.board_truth(oracle, m, p, poses[k]))
        print(f"board {NAMES[m]} pose {k}: worst corner error {err:.5f} px, bound {rr.rt_bound(pr.RT_PHOTO_BOARD_WORST[m]):.5f}")
        assert err <= rr.rt_bound(pr.RT_PHOTO_BOARD_WORST[m]), (NAMES[m], k, err)


@pytest.mark.parametrize("m", [rr.UCM, rr.EUCM, rr.KB4, rr.OPENCV5], ids=lambda m: NAMES[m])
def test_round_trip_aprilgrid(gpu_ctx, oracle, m):
    p, poses, S = rr.gt_params(m), pr.rt_grid_poses(m), rr.RT_SIZE
    fam = rr.family()
    block = _block(len(poses))
    gpu_ctx.render_targets_dev(block.data_ptr(), m, p, _ffi.PIX_U8, S, S, poses,
                               engine.aprilgrid_target(0.03, 0.3, rr.GRID.tag_rows, rr.GRID.tag_cols, 0, fam.bits, fam.codes, 1),
                               photo=_photo(pr.RT_PHOTO))
    got = gpu_ctx.detect_tags_dev(block.data_ptr(), _ffi.PIX_U8, S, S, len(poses), fam.bits, fam.codes, half_win=rr.RT_GRID_HALF_WIN)
    for k, (ids, rot, ham, corners, *_) in enumerate(got):
        assert [int(t) for t in ids] == list(range(6)) and not np.any(ham), (NAMES[m], k, list(ids), list(ham))
        truth = rr.grid_truth(oracle, m, p, poses[k])
        err = max(float(np.linalg.norm(c - truth[int(t)], axis=1).max()) for t, c in zip(ids, corners))
        print(f"grid {NAMES[m]} pose {k}: worst corner error {err:.5f} px, bound {rr.rt_bound(pr.RT_PHOTO_GRID_WORST[m]):.5f}")
        assert err <= rr.rt_bound(pr.RT_PHOTO_GRID_WORST[m]), (NAMES[m], k, err)


# ---- error codes --------------------------------------------------------------------------------------------------------------------------
def _raw_apply(ctx, src_dtype=_ffi.PIX_U8, dst_dtype=_ffi.PIX_U8, w=8, h=8, n=1, src=True, dst=True, photo=True, overlap=None, **o):
    """ccal_photo_apply_dev with one argument changed, on a block of 0x5A bytes: (status, the message, the block untouched)."""
    import torch
    block = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s_ptr = block.data_ptr() + 256
    d_ptr = block.data_ptr() + 2048 if overlap is None else s_ptr + overlap
    po = _ffi.PhotoOpts(**pr.opts(**o))
    rc = ctx.lib.ccal_photo_apply_dev(ctx.handle, src_dtype, dst_dtype, w, h, n, C.c_void_p(s_ptr) if src else None, C.c_void_p(d_ptr) if dst else None,
                                      C.byref(po) if photo else None)
    msg = ctx.last_error()
    ctx.sync()
    return rc, msg, bool((block.cpu().numpy() == 0x5A).all())


def test_error_codes_of_apply_dev(gpu_ctx):
    INV = _ffi.ERR_INVALID_ARG
    rc, _, untouched = _raw_apply(gpu_ctx, gain=2.0)
    assert rc == _ffi.OK and not untouched
    assert _raw_apply(gpu_ctx, n=0, src=False, dst=False)[::2] == (_ffi.OK, True)
    for kw, word in ((dict(photo=False), "photo"), (dict(src_dtype=2), "src_dtype"), (dict(dst_dtype=-1), "dst_dtype"), (dict(w=0), "size"),
                     (dict(h=-1), "size"), (dict(n=-1), "size"), (dict(w=65536, h=32768), "2^31 - 1 pixels"), (dict(src=False), "src_dev"),
                     (dict(dst=False), "dst_dev"), (dict(overlap=0), "overlap"), (dict(overlap=63), "overlap"), (dict(overlap=-63), "overlap"),
                     (dict(src_dtype=_ffi.PIX_U16, overlap=127), "overlap"), (dict(dst_dtype=_ffi.PIX_U16, overlap=-127), "overlap"),
                     (dict(blur_sigma=5.34), "blur_sigma"), (dict(blur_sigma=float("nan")), "blur_sigma"), (dict(blur_sigma=-0.1), "blur_sigma"),
                     (dict(vignette=-1.0), "vignette"), (dict(vignette=float("inf")), "vignette"), (dict(gain=-1.0), "gain"),
                     (dict(gain=float("nan")), "gain"), (dict(noise_read=-2.0), "noise_read"), (dict(noise_read=float("inf")), "noise_read"),
                     (dict(noise_shot=-0.05), "noise_shot"), (dict(noise_shot=float("nan")), "noise_shot"), (dict(first_index=-1), "first_index")):
        rc, msg, untouched = _raw_apply(gpu_ctx, **kw)
        assert rc == INV and word in msg and msg.startswith("ccal_photo_apply_dev: ") and untouched, (kw, rc, msg, untouched)
    assert _raw_apply(gpu_ctx, overlap=64)[0] == _ffi.OK and _raw_apply(gpu_ctx, overlap=-64)[0] == _ffi.OK       # blocks that touch
    assert _raw_apply(gpu_ctx)[0] == _ffi.OK                                                # the context is as good as before


def test_error_codes_of_the_render_forms(gpu_ctx):
    INV = _ffi.ERR_INVALID_ARG
    target = engine.checkerboard_target(7, 5, 0.03)
    params = np.asarray(rr.SMALL[rr.UCM], dtype=np.float64)
    pose = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.3]])
    dp = C.POINTER(C.c_double)

    def raw(fn, photo=True, n=1, out=True, w=8, dtype=_ffi.PIX_U8, ss=None, **o):
        ro = engine.render_opts(target, supersample=ss, lib=gpu_ctx.lib)
        po = _ffi.PhotoOpts(**pr.opts(**o))
        buf = np.zeros(256, dtype=np.uint8)
        rc = fn(gpu_ctx.handle, rr.UCM, params.ctypes.data_as(dp), dtype, w, 8, n, pose.ctypes.data_as(dp), C.byref(target), C.byref(ro),
                C.byref(po) if photo else None, C.c_void_p(buf.ctypes.data) if out else None)
        return rc, gpu_ctx.last_error()

    host = gpu_ctx.lib.ccal_render_photo_targets
    assert raw(host)[0] == _ffi.OK
    assert raw(host, n=0, out=False)[0] == _ffi.OK
    for kw, word in ((dict(photo=False), "photo"), (dict(blur_sigma=6.0), "blur_sigma"), (dict(vignette=-1.0), "vignette"), (dict(gain=float("inf")), "gain"),
                     (dict(noise_read=-1.0), "noise_read"), (dict(noise_shot=float("nan")), "noise_shot"), (dict(first_index=-5), "first_index"),
                     (dict(w=0), "size"), (dict(dtype=3), "dtype"), (dict(ss=9), "supersample"), (dict(out=False), "output")):
        rc, msg = raw(host, **kw)
        assert rc == INV and word in msg and msg.startswith("ccal_render_photo_targets: "), (kw, rc, msg)
    rc, msg = raw(gpu_ctx.lib.ccal_render_photo_targets_dev, out=False)
    assert rc == INV and msg.startswith("ccal_render_photo_targets_dev: ")
    with pytest.raises(CcalError) as e:
        gpu_ctx.render_targets_dev(0, rr.UCM, params, _ffi.PIX_U8, 8, 8, pose, target, photo=_photo(pr.opts(gain=-1.0)))
    assert e.value.code == INV and "ccal_render_photo_targets_dev" in str(e.value) and "gain" in str(e.value)
    assert raw(host)[0] == _ffi.OK
