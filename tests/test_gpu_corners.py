"""GPU: sub-pixel corner refinement (ccal_kernels_corners.hip, ccal_refine_corners_batch / _dev, api.refine_corners /
api.redetect_corners) against tests/corner_ref.py, the numpy f64 yardstick of the rule stated in include/ccal.h.

Bounds.  The kernel and the yardstick evaluate the same f64 formulas in different orders of summation (64 lane-private sums and a
butterfly against numpy's pairwise sums) and with different contractions, so a position agrees to rounding times the conditioning of
eight well-posed 2 x 2 solves: 1e-9 px and 1e-9 relative for lambda_min are the suite's bound for f64 against f64
(tests/test_gpu_undistort.py), orders of magnitude above that.  Statuses and iteration counts are DECISIONS: with eps = 0 no stop
test can be near its threshold; with eps = 1e-3 only corners whose yardstick margins exceed 1e-7 are compared (at most 2 % may be
left out; tests/test_corners_cpu.py holds the seeds to none).  Images are 67 x 45 up to 160 x 160; every case takes well under a second."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ref.parity_cases()


def _bits(arrays):
    return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in arrays]


def _compare(got, want, keep, where):
    """got: (xy, status, iters, lam) of one image from the device; want: the yardstick's dict; keep: the corners compared."""
    xy, status, iters, lam = got
    assert np.array_equal(status[keep], want["status"][keep]), (where, status, want["status"])
    assert np.array_equal(iters[keep], want["iters"][keep]), (where, iters, want["iters"])
    a, b = xy[keep], want["xy"][keep]
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), where
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True), where                  # a start that is not finite comes back as given
    d_xy = np.abs(a[fin] - b[fin]).max() if fin.any() else 0.0
    la, lb = lam[keep], want["lam"][keep]
    assert np.array_equal(np.isnan(la), np.isnan(lb)), where
    ok = ~np.isnan(lb)
    d_lam = (np.abs(la[ok] - lb[ok]) / np.where(lb[ok] != 0.0, np.abs(lb[ok]), 1.0)).max() if ok.any() else 0.0
    print(f"{where}: {int(keep.sum())} corners, statuses {np.bincount(want['status'][keep], minlength=9)}, max |d xy| {d_xy:.3e} px, "
          f"max rel |d lambda_min| {d_lam:.3e}")
    given = np.isin(want["status"][keep], (ref.NO_RESULT, ref.NOT_PD))
    assert d_xy <= 1e-9 and d_lam <= 1e-9
    return given


# ---- parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_fixed_iterations(gpu_ctx, name):
    """eps = 0, 8 iterations: positions, iteration counts, statuses and lambda_min of every corner."""
    img, starts, h = CASES[name]
    got = [o[0] for o in gpu_ctx.refine_corners_batch(img[None], [starts], h, 8, 0.0)]
    want = ref.refine(img, starts, h, 8, 0.0)
    given = _compare(got, want, np.ones(len(starts), dtype=bool), f"fixed {name}")
    assert _bits([got[0][given]]) == _bits([starts[given]])                         # NO_RESULT / NOT_PD: the position as given, bit for bit
    assert (want["status"] == ref.NO_CONVERGENCE).any() and (want["status"] == ref.NO_RESULT).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_stop_rule(gpu_ctx, name):
    """eps = 1e-3, 30 iterations: statuses, iteration counts and positions of every corner whose yardstick margins exceed 1e-7."""
    img, starts, h = CASES[name]
    got = [o[0] for o in gpu_ctx.refine_corners_batch(img[None], [starts], h, 30, 1e-3)]
    want = ref.refine(img, starts, h, 30, 1e-3)
    keep = (want["margin_e"] > 1e-7) & (want["margin_det"] > 1e-7)
    assert (~keep).sum() <= 0.02 * len(starts)
    _compare(got, want, keep, f"stop rule {name}")
    assert h == 1 or (want["status"] == ref.OK).sum() >= 8


# ---- batch shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_batch_shape_permutation_and_repeat(gpu_ctx, dtype):
    """0, 1, 63, 64 and 65 corners in the five images of one call: every image against the yardstick; a permutation of each image's
    corners permutes every output bit for bit; a second run is bit-identical."""
    imgs, xy = ref.batch_fixture(dtype=dtype)
    h = ref.BATCH_HALF_WIN
    first = gpu_ctx.refine_corners_batch(imgs, xy, h, 8, 0.0)
    assert [len(s) for s in first[1]] == list(ref.BATCH_COUNTS)
    seen = np.zeros(9, dtype=int)
    for k in range(len(imgs)):
        want = ref.refine(imgs[k], xy[k], h, 8, 0.0)
        seen += np.bincount(want["status"], minlength=9)
        _compare([o[k] for o in first], want, np.ones(len(xy[k]), dtype=bool), f"batch {np.dtype(dtype).name} image {k}")
    assert seen[ref.NO_RESULT] and seen[ref.NOT_PD] and seen[ref.NO_CONVERGENCE]
    again = gpu_ctx.refine_corners_batch(imgs, xy, h, 8, 0.0)
    for a, b in zip(first, again):
        assert _bits(a) == _bits(b)
    rng = np.random.default_rng(7)
    perms = [rng.permutation(len(p)) for p in xy]
    order = [4, 2, 0, 3, 1]                                                          # and the images in another order
    moved = gpu_ctx.refine_corners_batch(imgs[order], [xy[k][perms[k]] for k in order], h, 8, 0.0)
    for a, b in zip(first, moved):
        assert _bits([a[k][perms[k]] for k in order]) == _bits(b)


def test_no_images_and_no_corners(gpu_ctx):
    xy = np.full((1, 2), 7.0); status = np.full(1, -2, dtype=np.int32)
    img = np.zeros((45, 67), dtype=np.uint8)
    call = gpu_ctx.lib.ccal_refine_corners_batch
    args = (xy.ctypes.data_as(C.POINTER(C.c_double)), 3, 8, 0.0, status.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
    assert call(gpu_ctx.handle, _ffi.PIX_U8, 67, 45, 0, None, None, *args) == _ffi.OK                      # n_img == 0
    offs = np.zeros(3, dtype=np.int64)
    assert call(gpu_ctx.handle, _ffi.PIX_U8, 67, 45, 2, C.c_void_p(np.stack([img, img]).ctypes.data),
                offs.ctypes.data_as(C.POINTER(C.c_int64)), *args) == _ffi.OK                               # two images, no corner
    assert xy[0, 0] == 7.0 and status[0] == -2
    out = gpu_ctx.refine_corners_batch(img[None], [np.zeros((0, 2))])
    assert [len(o[0]) for o in out] == [0, 0, 0, 0]


# ---- status rules on the device ------------------------------------------------------------------------------------------------
def test_status_rules(gpu_ctx):
    """The cases of the CPU test: flat and single-edge images (NOT_PD), exactly h + 1 from a border (inside), one ulp nearer, NaN
    and infinite starts (NO_RESULT), starts 2.5 px off with h = 2 (the drift rule) - statuses equal to the yardstick's, positions
    returned as given, bit for bit, where the rule says so."""
    flat = np.full((45, 67), 77, dtype=np.uint8)
    edge = np.zeros((45, 67), dtype=np.uint8)
    edge[:, 30:] = 200
    pts = np.array([[30.0, 20.0], [29.7, 20.3]])
    xy, status, iters, lam = gpu_ctx.refine_corners_batch(np.stack([flat, edge]), [pts, pts], 3, 30, 1e-3)
    for k in range(2):
        assert (status[k] == ref.NOT_PD).all() and (iters[k] == 0).all() and (lam[k] == 0.0).all()
        assert _bits([xy[k]]) == _bits([pts])
    img, _, _ = ref.grid_fixture(ref.TRUTH_SEEDS[3])
    starts = ref.rule_starts(img.shape[1], img.shape[0], 3)
    got = [o[0] for o in gpu_ctx.refine_corners_batch(img[None], [starts], 3, 30, 1e-3)]
    want = ref.refine(img, starts, 3, 30, 1e-3)
    assert np.array_equal(got[1], want["status"]) and np.array_equal(got[2], want["iters"])
    assert (got[1][4:] == ref.NO_RESULT).all() and np.isnan(got[3][4:]).all() and not np.isnan(got[3][:4]).any()
    assert _bits([got[0][4:]]) == _bits([starts[4:]])
    img, _, starts = ref.drift_fixture()
    got = [o[0] for o in gpu_ctx.refine_corners_batch(img[None], [starts], 2, 30, 1e-3)]
    want = ref.refine(img, starts, 2, 30, 1e-3)
    keep = (want["margin_e"] > 1e-7) & (want["margin_det"] > 1e-7)
    assert keep.all()
    given = _compare(got, want, keep, "drift, h = 2")
    drifted = (want["status"] == ref.NO_RESULT) & (want["iters"] > 0)
    assert drifted.sum() >= 1 and _bits([got[0][given]]) == _bits([starts[given]])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_dev_entry_point_gives_the_host_calls_bits(gpu_ctx, dtype):
    import torch
    imgs, xy = ref.batch_fixture(dtype=dtype)
    host = gpu_ctx.refine_corners_batch(imgs, xy, ref.BATCH_HALF_WIN, 30, 1e-3)
    raw = torch.from_numpy(imgs.view(np.uint8).copy()).cuda()                        # the bytes of the image block, torch-allocated
    torch.cuda.synchronize()
    dev = gpu_ctx.refine_corners_dev(raw.data_ptr(), _ffi.PIX_U8 if dtype == np.uint8 else _ffi.PIX_U16, ref.BATCH_W, ref.BATCH_H,
                                     len(imgs), xy, ref.BATCH_HALF_WIN, 30, 1e-3)
    for a, b in zip(host, dev):
        assert _bits(a) == _bits(b)


# ---- invalid arguments ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(gpu_ctx):
    img = np.zeros((2, 45, 67), dtype=np.uint8)
    good = dict(dtype=_ffi.PIX_U8, w=67, h=45, n=2, img=C.c_void_p(img.ctypes.data), offs=[0, 1, 2], xy=True, half=3, it=8, eps=1e-3,
                status=True)
    bad = [dict(half=0), dict(half=16), dict(it=0), dict(eps=-1e-3), dict(eps=float("nan")), dict(eps=float("inf")), dict(dtype=2),
           dict(dtype=-1), dict(w=0), dict(h=-1), dict(n=-1), dict(w=65536, h=32768), dict(offs=[1, 1, 2]), dict(offs=[0, 2, 1]),
           dict(img=None), dict(offs=None), dict(xy=False), dict(status=False)]
    for fn in (gpu_ctx.lib.ccal_refine_corners_batch, gpu_ctx.lib.ccal_refine_corners_dev):
        for change in bad:
            a = dict(good, **change)
            xy = np.full((2, 2), 20.0); status = np.full(2, -2, dtype=np.int32); iters = np.full(2, -2, dtype=np.int32)
            lam = np.full(2, -3.0)
            offs = None if a["offs"] is None else np.asarray(a["offs"], dtype=np.int64)
            rc = fn(gpu_ctx.handle, a["dtype"], a["w"], a["h"], a["n"], a["img"],
                    None if offs is None else offs.ctypes.data_as(C.POINTER(C.c_int64)),
                    xy.ctypes.data_as(C.POINTER(C.c_double)) if a["xy"] else None, a["half"], a["it"], a["eps"],
                    status.ctypes.data_as(C.POINTER(C.c_int32)) if a["status"] else None,
                    iters.ctypes.data_as(C.POINTER(C.c_int32)), lam.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == _ffi.ERR_INVALID_ARG, change
            assert (xy == 20.0).all() and (status == -2).all() and (iters == -2).all() and (lam == -3.0).all(), change
            assert gpu_ctx.last_error()
    with pytest.raises(ValueError):
        gpu_ctx.refine_corners_batch(np.zeros((1, 45, 67, 3), dtype=np.uint8), [np.zeros((1, 2))])          # colour
    with pytest.raises(ValueError):
        gpu_ctx.refine_corners_batch(img, [np.zeros((1, 2))])                                               # one list for two images


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E_SIZE, E2E_HALF_WIN, E2E_RADIUS = 160, 3, 8


def _e2e_scene():
    """An EUCM camera (synth's parameters, the principal point moved into a 160 x 160 image), three of synth's board poses and a
    6 x 6 board of 0.1 m pitch: per frame the true projections, and an image with a saddle at every projection that lies at least
    E2E_RADIUS + 2 px inside the image, but every fifth of those - their spots stay flat."""
    m = synth.MODEL_EUCM
    params = np.array(synth.GT_PARAMS[m])
    params[2:4] = [79.6, 80.3]
    poses = synth.make_problem(8, "eucm").poses_gt[[0, 4, 5]]
    k = (np.arange(6) - 2.5) * 0.1
    board = np.concatenate([np.stack(np.meshgrid(0.33 + k, -0.33 + k), axis=-1).reshape(-1, 2), np.zeros((36, 1))], axis=1)
    board = board.astype(np.float32).astype(np.float64)
    truth, imgs, drawn = [], [], []
    for f, pose in enumerate(poses):
        uv = synth.project(m, params, board @ synth.rodrigues(pose[:3]).T + pose[3:])
        roomy = np.flatnonzero(((uv >= E2E_RADIUS + 2) & (uv <= E2E_SIZE - 3 - E2E_RADIUS)).all(axis=1))
        draw = np.delete(roomy, np.arange(0, len(roomy), 5))
        imgs.append(ref.render(E2E_SIZE, E2E_SIZE, uv[draw], 400 + f, radius=E2E_RADIUS))
        truth.append(uv); drawn.append(draw)
    return params, poses, board, truth, imgs, drawn


def test_redetect_corners_end_to_end(gpu_ctx):
    """api.redetect_corners from a calibration whose focal length is 1 % off: exactly the yardstick's kept set - every rendered
    saddle, none of the flat spots, none of the projections outside - at the yardstick's positions.  The positions are STORED as f32:
    half an ulp of an f32 coordinate in [128, 256) is 7.63e-6 px, so the 1e-6 px bound is held against the yardstick's position
    rounded to f32 in the same way (an f64 disagreement of 1e-9 flips that rounding for one coordinate in thousands; it would show
    as an ulp, 1.5e-5), and the raw f64 difference to that half ulp (coordinates lie below 160)."""
    params, poses, board, truth, imgs, drawn = _e2e_scene()
    h = E2E_HALF_WIN
    off = params.copy()
    off[:2] *= 1.01                                                                   # the first calibration: focal 1 % off
    model = api.GenericModel("eucm", off, E2E_SIZE, E2E_SIZE)
    rtvecs = {f: api.RvecTvec.from6(p) for f, p in enumerate(poses)}
    points = {10 + j: tuple(float(v) for v in board[j]) for j in range(36)}
    out = api.redetect_corners(imgs, model, rtvecs, points, half_win=h, ctx=gpu_ctx)
    assert len(out) == 3
    n_outside = n_blank = 0
    for f in range(3):
        R, t = rtvecs[f].matrix()
        start, valid = model.project(board @ R.T + t, ctx=gpu_ctx)
        inside = valid & ((start >= h + 1) & (start <= E2E_SIZE - 2 - h)).all(axis=1)
        want = ref.refine(imgs[f], start[inside], h, 30, 1e-3)
        assert ((want["margin_e"] > 1e-7) & (want["margin_det"] > 1e-7)).all()
        kept = want["status"] == ref.OK
        ids = [10 + j for j in np.flatnonzero(inside)[kept]]
        assert out[f] is not None and sorted(out[f].features) == ids, (f, sorted(out[f].features), ids)
        assert out[f].img_w_h == (E2E_SIZE, E2E_SIZE)
        got = np.array([out[f].features[i].p2d for i in ids])
        d64 = np.abs(got - want["xy"][kept]).max()
        d = np.abs(got - want["xy"][kept].astype(np.float32).astype(np.float64)).max()
        err = np.hypot(*(got - truth[f][np.flatnonzero(inside)[kept]]).T).max()
        print(f"frame {f}: {len(ids)} of 36 kept ({int(inside.sum())} inside, {len(drawn[f])} drawn), max |d| to the yardstick as f32 {d:.2e} px "
              f"(as f64 {d64:.2e}), worst error against the true saddle {err:.4f} px")
        assert d <= 1e-6 and d64 <= 7.63e-6
        assert all(out[f].features[i].p3d == points[i] for i in ids)
        blank = set(np.flatnonzero(inside)) - set(drawn[f])
        assert {i - 10 for i in ids} == set(drawn[f])                                 # every saddle, nothing on a flat spot, nothing outside
        n_outside += int((~inside).sum()); n_blank += len(blank)
    assert n_outside >= 5 and n_blank >= 5                                            # the scene has both kinds


@pytest.mark.parametrize("h", sorted(ref.TRUTH_SEEDS))
def test_refine_corners_reaches_the_true_saddle(gpu_ctx, h):
    """api.refine_corners on detections up to 1.5 px off: every corner comes back, within the bound of the CPU truth test."""
    img, centres, starts = ref.grid_fixture(ref.TRUTH_SEEDS[h])
    frame = api.FrameFeature(9, (160, 160), {k: api.FeaturePoint((float(x), float(y)), (0.01 * k, 0.0, 0.0)) for k, (x, y) in enumerate(starts)})
    out = api.refine_corners([None, img], [None, frame], half_win=h, ctx=gpu_ctx)
    assert out[0] is None and out[1] is not None and out[1].time_ns == 9 and out[1].img_w_h == (160, 160)
    assert sorted(out[1].features) == list(range(25))
    got = np.array([out[1].features[k].p2d for k in range(25)])
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))             # stored as f32
    err = np.hypot(*(got - centres).T).max()
    print(f"h = {h}: worst error against the true saddle {err:.5f} px, bound {ref.TRUTH_BOUND[h]:.5f}")
    assert err <= ref.TRUTH_BOUND[h]
    assert api.refine_corners([img], [frame], half_win=h, min_lambda=1e30, ctx=gpu_ctx) == [None]      # screened by strength: none left
