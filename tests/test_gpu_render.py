"""GPU: the target renderer (ccal_render_targets_batch / _dev, ccal_kernels_render.hip) against tests/render_ref.py, the numpy f64
statement of the rule in include/ccal.h.

Bounds.  Outside NEAR pixels - pixels with a sub-pixel ray whose class changes within 1e-8 px, ten times the round-trip bound the
suite holds `unproject` to - the device image equals the yardstick's exactly; a near pixel may differ by the contribution of its
near rays plus one level; tests/test_render_cpu.py caps the near pixels of every case at 0.1 % on the yardstick alone.
Round trips at 512 x 512 under synth.GT_PARAMS: render_targets_dev feeds detect_checkerboards_dev / detect_tags_dev without the
images touching the host; every corner within 1.5 x the worst error the numpy chains reach on the yardstick's images of the same
poses (render_ref.RT_*_WORST), against oracle.project of the posed corner."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as rr  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, engine  # noqa: E402
from camera_intrinsic_calibration_rs_amd.engine import CcalError  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in rr.parity_cases()}
NAMES = {rr.UCM: "ucm", rr.EUCM: "eucm", rr.KB4: "kb4", rr.OPENCV5: "opencv5"}


def _target(t):
    if t["kind"] == "board":
        return engine.checkerboard_target(t["cols"], t["rows"], t["square"])
    b = t["board"]
    return engine.aprilgrid_target(b.tag_size_meter, b.tag_spacing, b.tag_rows, b.tag_cols, b.first_id, t["bits"], t["codes"], t["border"])


def _render(ctx, case, poses=None, params=None):
    return ctx.render_targets_batch(case["model"], case["params"] if params is None else params, case["width"], case["height"],
                                    case["poses"] if poses is None else poses, _target(case["target"]), case["dtype"], case["ss"],
                                    margin=case["target"]["margin"], **case["opts"])


def _render_dev(ctx, case, fill):
    """The _dev form into a torch block with 64 guard bytes on each side, every byte set to `fill` beforehand: (images, guards intact)."""
    import torch
    n, H, W = len(case["poses"]), case["height"], case["width"]
    nbytes = n * H * W * case["dtype"].itemsize
    block = torch.full((nbytes + 128,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_targets_dev(block.data_ptr() + 64, case["model"], case["params"], _ffi.PIX_U8 if case["dtype"] == np.uint8 else _ffi.PIX_U16,
                           W, H, case["poses"], _target(case["target"]), case["ss"], margin=case["target"]["margin"], **case["opts"])
    ctx.sync()
    host = block.cpu().numpy()
    guards = bool((host[:64] == fill).all() and (host[-64:] == fill).all())
    return host[64:-64].copy().view(case["dtype"]).reshape(n, H, W), guards


def _hold(got, case, oracle):
    want, near = rr.yardstick(oracle, case)
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    allowed = np.where(near > 0, rr.allowed_difference(near, case["ss"], case["dtype"], **{k: v for k, v in case["opts"].items()}), 0.0)
    bad = diff > allowed
    print(f"{case['name']}: {int((diff > 0).sum())} of {diff.size} pixels differ, {int((near > 0).sum())} near, worst {int(diff.max())}")
    assert not bad.any(), (case["name"], int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


# ---- parity with the yardstick: both targets, four models, the sizes, supersamplings, dtypes and image contents of the cases -----------
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity(gpu_ctx, oracle, name):
    _hold(_render(gpu_ctx, CASES[name]), CASES[name], oracle)


# ---- memory and determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["board ucm", "grid kb4", "grid opencv5 130 x 67 s 1 first_id 4", "board kb4 1 x 1", "grid eucm 65 images s 1"])
def test_dev_form_writes_every_pixel_and_nothing_else(gpu_ctx, name):
    case = CASES[name]
    host = _render(gpu_ctx, case)
    for fill in (0x5A, 0xA5):
        dev, guards = _render_dev(gpu_ctx, case, fill)
        assert guards, "bytes outside the block were written"
        assert np.array_equal(dev, host)


def test_two_runs_are_equal_and_an_image_does_not_depend_on_its_batch(gpu_ctx):
    case = CASES["grid eucm 65 images s 1"]
    a, b = _render(gpu_ctx, case), _render(gpu_ctx, case)
    assert np.array_equal(a, b)
    for k in (0, 1, 31, 63, 64):
        assert np.array_equal(_render(gpu_ctx, case, poses=case["poses"][k:k + 1])[0], a[k]), k
    case = CASES["board kb4"]
    a = _render(gpu_ctx, case)
    assert np.array_equal(a, _render(gpu_ctx, case))
    for k in range(3):
        assert np.array_equal(_render(gpu_ctx, case, poses=case["poses"][k:k + 1])[0], a[k]), k


def test_a_batch_cut_into_chunks(dev_ctx, gpu_ctx, monkeypatch):
    """The host form stages its images chunk by chunk; the second library reads the chunk limit from CCAL_TEST_RENDER_CHUNK_BYTES
    (tests only): one byte is an image per chunk, 2 x 67 x 45 bytes two images per chunk - three images: (0, 1), (2)."""
    case = CASES["board ucm"]
    want = _render(gpu_ctx, case)
    for limit in ("1", str(2 * 67 * 45)):
        monkeypatch.setenv("CCAL_TEST_RENDER_CHUNK_BYTES", limit)
        assert np.array_equal(_render(dev_ctx, case), want), limit
    case = CASES["grid eucm 65 images s 1"]
    monkeypatch.setenv("CCAL_TEST_RENDER_CHUNK_BYTES", str(7 * 67 * 45))
    assert np.array_equal(_render(dev_ctx, case), _render(gpu_ctx, case))


@pytest.fixture()
def conventions(gpu_ctx):
    yield gpu_ctx.model_conventions()
    gpu_ctx.set_model_conventions(None)


def test_reads_ocv5_order(gpu_ctx, oracle, conventions):
    case = CASES["board opencv5"]
    order = [2, 0, 4, 1, 3]                                    # k1 sits at slot 2, k2 at 0, p1 at 4, p2 at 1, k3 at 3
    for i, o in enumerate(order):
        conventions.ocv5_order[i] = o
    gpu_ctx.set_model_conventions(conventions)
    q = case["params"].copy()
    for i, o in enumerate(order):
        q[4 + o] = case["params"][4 + i]
    assert not np.array_equal(q, case["params"])
    _hold(_render(gpu_ctx, case, params=q), case, oracle)


def test_the_api_wrappers(gpu_ctx, oracle):
    """api.render_checkerboard / render_aprilgrid: RvecTvec poses or an [n, 6] array, the image size from the model, the defaults
    (supersample 4, margins of one square / one tag pitch) - the cases' own."""
    case = CASES["board eucm"]
    model = api.GenericModel("eucm", case["params"], case["width"], case["height"])
    got = api.render_checkerboard(model, [api.RvecTvec.from6(p) for p in case["poses"]], rr.BOARD[:2], rr.BOARD[2], dtype=case["dtype"], ctx=gpu_ctx)
    _hold(got, case, oracle)
    case = CASES["grid kb4"]
    model = api.GenericModel("kb4", case["params"], case["width"], case["height"])
    fam = api.TagFamily("seeded", rr.family().bits, rr.family().codes)
    got = api.render_aprilgrid(model, case["poses"], api.AprilGridBoard(0.03, 0.3, 2, 3), fam, dtype=case["dtype"], ctx=gpu_ctx)
    _hold(got, case, oracle)
    assert api.render_checkerboard(model, np.zeros((0, 6)), (7, 5), 0.03, ctx=gpu_ctx).shape == (0, 45, 67)


# ---- round trips under the four GT lenses ---------------------------------------------------------------------------------------------
def _block(n):
    import torch
    block = torch.zeros((n, rr.RT_SIZE, rr.RT_SIZE), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return block


@pytest.mark.parametrize("m", [rr.UCM, rr.EUCM, rr.KB4, rr.OPENCV5], ids=lambda m: NAMES[m])
def test_round_trip_checkerboard(gpu_ctx, oracle, m):
    p, poses, S = rr.gt_params(m), rr.rt_board_poses(m), rr.RT_SIZE
    block = _block(len(poses))
    gpu_ctx.render_targets_dev(block.data_ptr(), m, p, _ffi.PIX_U8, S, S, poses, engine.checkerboard_target(*rr.BOARD))
    res = gpu_ctx.detect_checkerboards_dev(block.data_ptr(), _ffi.PIX_U8, S, S, len(poses), rr.BOARD[0], rr.BOARD[1], half_win=rr.RT_BOARD_HALF_WIN)
    for k, (found, xy, _, _) in enumerate(res):
        assert found, (NAMES[m], k)
        err = rr.board_error(xy, rr.board_truth(oracle, m, p, poses[k]))
        print(f"board {NAMES[m]} pose {k}: worst corner error {err:.5f} px, bound {rr.rt_bound(rr.RT_BOARD_WORST[m]):.5f}")
        assert err <= rr.rt_bound(rr.RT_BOARD_WORST[m]), (NAMES[m], k, err)


@pytest.mark.parametrize("m", [rr.UCM, rr.EUCM, rr.KB4, rr.OPENCV5], ids=lambda m: NAMES[m])
def test_round_trip_aprilgrid(gpu_ctx, oracle, m):
    p, poses, S = rr.gt_params(m), rr.rt_grid_poses(m), rr.RT_SIZE
    fam, board = rr.family(), api.AprilGridBoard(rr.GRID.tag_size_meter, rr.GRID.tag_spacing, rr.GRID.tag_rows, rr.GRID.tag_cols)
    block = _block(len(poses))
    gpu_ctx.render_targets_dev(block.data_ptr(), m, p, _ffi.PIX_U8, S, S, poses,
                               engine.aprilgrid_target(0.03, 0.3, rr.GRID.tag_rows, rr.GRID.tag_cols, 0, fam.bits, fam.codes, 1))
    got = gpu_ctx.detect_tags_dev(block.data_ptr(), _ffi.PIX_U8, S, S, len(poses), fam.bits, fam.codes, half_win=rr.RT_GRID_HALF_WIN)
    decoded = [[(int(t), int(r), int(h), c.copy()) for t, r, h, c in zip(ids, rot, ham, corners)] for ids, rot, ham, corners, *_ in got]
    frames = api.frames_from_tags(decoded, board, (S, S))
    for k, tags in enumerate(decoded):
        assert [t[0] for t in tags] == list(range(6)) and all(t[2] == 0 for t in tags), (NAMES[m], k, [(t[0], t[2]) for t in tags])
        assert frames[k] is not None and sorted(frames[k].features) == list(range(24))
        truth = rr.grid_truth(oracle, m, p, poses[k])
        err = max(float(np.linalg.norm(t[3] - truth[t[0]], axis=1).max()) for t in tags)
        print(f"grid {NAMES[m]} pose {k}: worst corner error {err:.5f} px, bound {rr.rt_bound(rr.RT_GRID_WORST[m]):.5f}")
        assert err <= rr.rt_bound(rr.RT_GRID_WORST[m]), (NAMES[m], k, err)


# ---- error codes ------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, model=rr.UCM, params=None, dtype=_ffi.PIX_U8, w=8, h=8, n=1, poses=True, target=None, out=True, **opt):
    """ccal_render_targets_batch with one argument changed: (status, the context's message)."""
    params = np.asarray(rr.SMALL[rr.UCM] + [0.0] * 5, dtype=np.float64) if params is None else params
    target = engine.checkerboard_target(7, 5, 0.03) if target is None else target
    o = engine.render_opts(target, lib=ctx.lib)
    for k, v in opt.items():
        setattr(o, k, v)
    pose = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.3]] * max(n, 1))
    buf = np.zeros(max(n, 1) * 64 * 2, dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    rc = ctx.lib.ccal_render_targets_batch(ctx.handle, model, params.ctypes.data_as(dp), dtype, w, h, n, pose.ctypes.data_as(dp) if poses else None,
                                           C.byref(target), C.byref(o), C.c_void_p(buf.ctypes.data) if out else None)
    return rc, ctx.last_error()


def _grid(**kw):
    fam = rr.family()
    a = dict(tag_size=0.03, tag_spacing=0.3, tag_rows=2, tag_cols=3, first_id=0, family_bits=fam.bits, codes=fam.codes, border=1)
    a.update(kw)
    return engine.aprilgrid_target(**a)


def test_error_codes(gpu_ctx):
    INV = _ffi.ERR_INVALID_ARG
    assert _raw(gpu_ctx)[0] == _ffi.OK
    assert _raw(gpu_ctx, n=0, poses=False, out=False)[0] == _ffi.OK                        # a successful no-op
    rc, msg = _raw(gpu_ctx, model=api.MODEL_EUCMT)
    assert rc == _ffi.ERR_UNSUPPORTED and "EUCMT" in msg
    for kw, word in ((dict(model=7), "model"), (dict(dtype=2), "dtype"), (dict(w=0), "size"), (dict(h=-1), "size"), (dict(n=-1), "size"),
                     (dict(w=65536, h=32768), "2^31 - 1 pixels"), (dict(supersample=0), "supersample"), (dict(supersample=9), "supersample"),
                     (dict(margin=-1e-9), "margin"), (dict(margin=float("nan")), "margin"), (dict(black=float("inf")), "black"),
                     (dict(target=engine.checkerboard_target(7, 5, 0.0)), "square"), (dict(target=engine.checkerboard_target(7, 5, float("inf"))), "square"),
                     (dict(target=engine.checkerboard_target(0, 5, 0.03)), "cols"), (dict(target=engine.checkerboard_target(7, 0, 0.03)), "rows"),
                     (dict(target=_grid(tag_size=-0.03)), "tag_size"), (dict(target=_grid(tag_spacing=0.0)), "tag_spacing"),
                     (dict(target=_grid(tag_spacing=float("nan"))), "tag_spacing"), (dict(target=_grid(tag_rows=0)), "tag_rows"),
                     (dict(target=_grid(tag_cols=0)), "tag_cols"), (dict(target=_grid(first_id=35)), "n_codes"),
                     (dict(target=_grid(family_bits=35)), "family_bits"), (dict(target=_grid(border=0)), "border"),
                     (dict(target=_grid(codes=())), "n_codes"), (dict(poses=False), "poses"), (dict(out=False), "output")):
        rc, msg = _raw(gpu_ctx, **kw)
        assert rc == INV and word in msg and msg.startswith("ccal_render_targets_batch: "), (kw, rc, msg)
    bad_kind = engine.checkerboard_target(7, 5, 0.03)
    bad_kind.kind = 2
    assert _raw(gpu_ctx, target=bad_kind)[0] == INV
    with pytest.raises(CcalError) as e:
        gpu_ctx.render_targets_dev(0, rr.UCM, rr.SMALL[rr.UCM], _ffi.PIX_U8, 8, 8, np.zeros((1, 6)), engine.checkerboard_target(7, 5, 0.03))
    assert e.value.code == INV and "ccal_render_targets_dev" in str(e.value)
    assert _raw(gpu_ctx)[0] == _ffi.OK                                                      # the context is as good as before
