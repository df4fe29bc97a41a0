"""GPU: board poses refined under fixed intrinsics (ccal_refine_poses_batch, k_pose_refine in csrc/ccal_kernels_refine.hip) -
against ground truth on exact data, against the numpy yardstick tests/refine_ref.py on noisy data with outliers, for first-order
optimality with a gradient the kernel's Jacobian has no part in, on the shapes where the lane loop and the four-wavefront workgroup
can go wrong, for independence of the batch and determinism, the loss switch, the argument checks, held-out validation and on
poisoned memory."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth
from camera_intrinsic_calibration_rs_amd.engine import CcalError, Problem, default_opts

import refine_ref

pytestmark = pytest.mark.gpu

MODELS = ["ucm", "eucm", "kb4", "opencv5"]
OK_ = _ffi.OK


def _tight(rel=1e-12):
    """The stop rules far below the comparisons made here: the frame runs until the predicted decrease of a step is `rel` of
    the objective (or, on exact data, the objective or the predicted decrease is below 1e-24 px^2: the rounding of 144 residuals of
    ~500 px leaves ~1e-25)."""
    return default_opts(_ffi.METHOD_LM, min_error=1e-24, min_abs_error_decrease=1e-24, min_rel_error_decrease=rel)


# The comparisons with the yardstick on frames with outliers run the frame to the rounding of its objective: the reported cost
# sum rho'(s) s is not stationary where sum rho(s) is, so a pose error e shows in it at first order (|d cost / d pose| ~ 7 outliers x
# 300 px / rad against a cost of ~140 px^2: 1e-9 relative asks for e ~ 1e-10), and a last step whose predicted decrease is 1e-12 of
# the objective is still ~1e-7 long in the frame's weakest direction.  1e-16 of the objective is below the rounding of its sum.
_TO_ROUNDING = 1e-16


# The yardstick's own difference to the ground truth on the 4 x 12 exact frames of test_exact_data, run from the same perturbed start
# (a run from the truth stays there), measured on an MI355X machine (EXPERIMENTS.md): rotation-matrix entries 1.78e-15 (OPENCV5),
# translation 3.33e-16 m.  Asserted at 10 x that.
EXACT_DIFF_R = 10 * 1.78e-15
EXACT_DIFF_T = 10 * 3.33e-16
# The yardstick's resolution on the 2 x 40 noisy frames of test_noisy_against_the_yardstick: the difference between its run from
# the initial pose and its run from the ground truth, which end in the same minimum, measured the same way: rotation-matrix
# entries 1.35e-9, translation 6.08e-10 m (KB4; EUCM 2.09e-10 / 2.78e-11).  Asserted at 10 x that.
NOISY_DIFF_R = 10 * 1.35e-9
NOISY_DIFF_T = 10 * 6.08e-10
# The yardstick's own residual gradient on those frames, relative to the gradient at the start: 9.0e-9 (KB4; EUCM 2.6e-9).
# Asserted at 10 x that.
GRAD_REL = 10 * 9.0e-9
assert max(EXACT_DIFF_R, EXACT_DIFF_T, NOISY_DIFF_R, NOISY_DIFF_T) <= 1e-6


def _frames(sp):
    return [(int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])) for o in range(sp.n_obs)]


def _params(sp):
    m = int(sp.model[0])
    return m, sp.intr_gt[0, :synth.MODEL_NPARAMS[m]].copy()


@functools.lru_cache(maxsize=None)
def _exact(model):
    """12 frames, uv recomputed in f64 at the true pose; the start 0.05 rad / 0.02 m off."""
    sp = synth.make_problem(12, model, noise_px=0)
    m, par = _params(sp)
    X = [sp.p3d[a:b].astype(np.float64) for a, b in _frames(sp)]
    U = [synth.project(m, par, X[f] @ synth.rodrigues(sp.poses_gt[f, :3]).T + sp.poses_gt[f, 3:]) for f in range(12)]
    sgn = np.where(synth.uniform01(0xE7AC7, 12 * 6, stream=40).reshape(12, 6) < 0.5, -1.0, 1.0)
    start = sp.poses_gt + sgn * np.array([0.05, 0.05, 0.05, 0.02, 0.02, 0.02]) / np.sqrt(3.0)
    return m, par, X, U, start, sp.poses_gt


@functools.lru_cache(maxsize=None)
def _noisy(model):
    """40 ragged frames, 0.1 px noise, 5 % of the corners displaced by 20 px in a random direction."""
    sp = synth.make_problem(40, model, noise_px=0.1, ragged=True)
    n = sp.n_corners
    bad = synth.uniform01(0x0071E5, n, stream=31) < 0.05
    ang = 2.0 * np.pi * synth.uniform01(0x0071E5, n, stream=32)
    uv = sp.p2d.astype(np.float64)
    uv[bad] += 20.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
    return dataclasses.replace(sp, p2d=uv.astype(np.float32))


def _noisy_inputs(ctx, model):
    sp = _noisy(model)
    m, par = _params(sp)
    gp = Problem.from_synth(ctx, sp)
    poses0, used = gp.init_poses(sp.intr_gt)
    gp.close()
    assert (used > 0).all()
    X = [sp.p3d[a:b].astype(np.float64) for a, b in _frames(sp)]
    U = [sp.p2d[a:b].astype(np.float64) for a, b in _frames(sp)]
    return sp, m, par, X, U, poses0


@functools.lru_cache(maxsize=None)
def _yardstick_noisy(model, poses0_bytes):
    """The yardstick on the noisy frames: computed once, shared, never changed.  Per frame (pose, cost, pose of the run from the
    initial pose, pose of the run from the ground truth)."""
    sp = _noisy(model)
    m, par = _params(sp)
    poses0 = np.frombuffer(poses0_bytes).reshape(-1, 6)
    out = []
    for f, (a, b) in enumerate(_frames(sp)):
        X, uv = sp.p3d[a:b].astype(np.float64), sp.p2d[a:b].astype(np.float64)
        ra = refine_ref.refine(m, par, X, uv, poses0[f], 1.0)
        rb = refine_ref.refine(m, par, X, uv, sp.poses_gt[f], 1.0)
        best = ra if ra[1] <= rb[1] else rb
        out.append((best[0], best[1], ra[0], rb[0]))
    return out


def _dR(p, q):
    return float(np.abs(synth.rodrigues(np.asarray(p)[..., :3]) - synth.rodrigues(np.asarray(q)[..., :3])).max())


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_exact_data(gpu_ctx, model):
    m, par, X, U, start, gt = _exact(model)
    poses, status, iters, used, cost0, cost = gpu_ctx.refine_poses_batch(m, par, X, U, start, 1.0, 4, _tight())
    ref = [refine_ref.refine(m, par, X[f], U[f], start[f], 1.0)[0] for f in range(12)]      # (from the same start: a run from the truth stays there)
    ref_r = max(_dR(ref[f], gt[f]) for f in range(12)); ref_t = max(np.abs(ref[f][3:] - gt[f, 3:]).max() for f in range(12))
    dr = _dR(poses, gt); dt = float(np.abs(poses[:, 3:] - gt[:, 3:]).max())
    print(f"{model}: kernel dR {dr:.2e} dt {dt:.2e}; yardstick dR {ref_r:.2e} dt {ref_t:.2e}; iters {iters.min()}..{iters.max()} "
          f"cost0 {cost0.max():.3e} cost {cost.max():.3e}")
    assert (status == OK_).all(), status
    assert (used == [len(x) for x in X]).all()
    assert (cost <= cost0).all()
    assert dr <= EXACT_DIFF_R, dr
    assert dt <= EXACT_DIFF_T, dt


# ---- 2. noisy data with outliers, against the yardstick --------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["eucm", "kb4"])
def test_noisy_against_the_yardstick(gpu_ctx, model):
    sp, m, par, X, U, poses0 = _noisy_inputs(gpu_ctx, model)
    poses, status, iters, used, cost0, cost = gpu_ctx.refine_poses_batch(m, par, X, U, poses0, 1.0, 4, _tight(_TO_ROUNDING))
    ref = _yardstick_noisy(model, np.ascontiguousarray(poses0).tobytes())
    own_r = max(_dR(r[2], r[3]) for r in ref); own_t = max(np.abs(r[2][3:] - r[3][3:]).max() for r in ref)
    worst_r = max(_dR(poses[f], ref[f][0]) for f in range(40))
    worst_t = max(np.abs(poses[f, 3:] - ref[f][0][3:]).max() for f in range(40))
    worst_c = max(cost[f] / ref[f][1] - 1 for f in range(40))
    print(f"{model}: kernel - yardstick dR {worst_r:.2e} dt {worst_t:.2e}, cost / yardstick cost - 1 <= {worst_c:.2e}; "
          f"yardstick's two starts differ by dR {own_r:.2e} dt {own_t:.2e}; iters {iters.min()}..{iters.max()}")
    assert (status == OK_).all(), status                 # no frame is left out
    assert (used == [len(x) for x in X]).all()
    assert worst_r <= NOISY_DIFF_R, worst_r
    assert worst_t <= NOISY_DIFF_T, worst_t
    assert worst_c <= 1e-9, worst_c


# ---- 3. first-order optimality, independent of the kernel's Jacobian ---------------------------------------------------------------
@pytest.mark.parametrize("model", ["eucm", "kb4"])
def test_first_order_optimality(gpu_ctx, model):
    sp, m, par, X, U, poses0 = _noisy_inputs(gpu_ctx, model)
    poses, status, *_ = gpu_ctx.refine_poses_batch(m, par, X, U, poses0, 1.0, 4, _tight(_TO_ROUNDING))
    ref = _yardstick_noisy(model, np.ascontiguousarray(poses0).tobytes())
    worst = worst_ref = 0.0
    for f in range(40):
        g0 = np.linalg.norm(refine_ref.gradient(m, par, X[f], U[f], poses0[f], 1.0))
        worst = max(worst, np.linalg.norm(refine_ref.gradient(m, par, X[f], U[f], poses[f], 1.0)) / g0)
        worst_ref = max(worst_ref, np.linalg.norm(refine_ref.gradient(m, par, X[f], U[f], ref[f][0], 1.0)) / g0)
    print(f"{model}: |grad| / |grad at the start| kernel {worst:.2e}, yardstick {worst_ref:.2e}")
    assert worst <= GRAD_REL, worst


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------------
def _shape_frames(counts, seed=0x5A4E):
    """One EUCM frame per entry of counts (0: an empty problem): corners drawn from a 20 x 15 board, 0.1 px noise."""
    bx, by = np.meshgrid(np.arange(20) * 0.035, -np.arange(15) * 0.035)
    board = np.stack([bx.ravel(), by.ravel(), np.zeros(300)], axis=1).astype(np.float32)
    sp = synth.make_problem(len(counts), "eucm", noise_px=0.1, board=board, seed=seed, shuffle_corners=True)
    m, par = _params(sp)
    X, U = [], []
    for f, (a, b) in enumerate(_frames(sp)):
        X.append(sp.p3d[a:a + counts[f]].astype(np.float64)); U.append(sp.p2d[a:a + counts[f]].astype(np.float64))
    return m, par, X, U, sp.poses0.copy(), sp.poses_gt


COUNTS = [4, 5, 63, 64, 65, 128, 129, 300, 144]


@pytest.mark.parametrize("n_prob", [1, 3, 4, 5, 9])
def test_shapes_and_batch_sizes(gpu_ctx, n_prob):
    m, par, X, U, start, gt = _shape_frames(COUNTS)
    alone = [gpu_ctx.refine_poses_batch(m, par, [X[f]], [U[f]], start[f:f + 1], 1.0, 4, _tight(), with_errors=True) for f in range(9)]
    # the batch takes the frames from the far end, so that every count appears in some batch size
    sel = list(range(9))[::-1][:n_prob] if n_prob < 9 else list(range(9))
    out = gpu_ctx.refine_poses_batch(m, par, [X[f] for f in sel], [U[f] for f in sel], start[sel], 1.0, 4, _tight(), with_errors=True)
    for k, f in enumerate(sel):
        for i in range(6):
            assert np.asarray(out[i][k]).tobytes() == np.asarray(alone[f][i][0]).tobytes(), (f, i)
        assert out[6][k].tobytes() == alone[f][6][0].tobytes()
        assert out[1][k] == OK_ and out[3][k] == COUNTS[f]
        # the refined pose is the minimum of the numpy cost: no lower cost at the yardstick's result, to rounding
        ref = refine_ref.solve(m, par, X[f], U[f], start[f], gt[f], 1.0)
        assert out[5][k] <= ref[1] * (1 + 1e-9) + 1e-18, (f, out[5][k], ref[1])
        r = refine_ref.residuals(m, par, X[f], U[f], out[0][k])
        np.testing.assert_allclose(out[6][k], np.sqrt((r * r).sum(axis=1)), rtol=0, atol=1e-9)


def test_empty_problem_nan_rows_and_too_few_points(gpu_ctx):
    m, par, X, U, start, gt = _shape_frames([64, 0, 129, 144, 6, 65])
    U[3] = U[3].copy(); X[2] = X[2].copy()
    U[3][[0, 70, 143], 0] = np.nan; X[2][[5, 128], 2] = np.inf
    start[4] = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    poses, status, iters, used, cost0, cost, err = gpu_ctx.refine_poses_batch(m, par, X, U, start, 1.0, 7, _tight(), with_errors=True)
    assert status.tolist() == [OK_, _ffi.NO_RESULT, OK_, OK_, _ffi.NO_RESULT, OK_], status
    assert used.tolist() == [64, 0, 127, 141, 0, 65]
    for f in (1, 4):                                      # empty / below min_points: untouched
        assert poses[f].tobytes() == start[f].tobytes() and iters[f] == 0 and cost0[f] == 0.0 and cost[f] == 0.0
        assert np.isnan(err[f]).all()
    assert np.isnan(err[3][[0, 70, 143]]).all() and np.isfinite(np.delete(err[3], [0, 70, 143])).all()
    assert np.isnan(err[2][[5, 128]]).all() and np.isfinite(np.delete(err[2], [5, 128])).all()
    # the NaN rows are left out: the same result as the frame without them
    keep = np.ones(144, dtype=bool); keep[[0, 70, 143]] = False
    o = gpu_ctx.refine_poses_batch(m, par, [X[3][keep]], [U[3][keep]], start[3:4], 1.0, 7, _tight())
    np.testing.assert_allclose(poses[3], o[0][0], rtol=0, atol=1e-12)
    # a start that is not finite: no result either
    bad = start.copy(); bad[0, 2] = np.nan
    o = gpu_ctx.refine_poses_batch(m, par, X, U, bad, 1.0, 7, _tight())
    assert o[1][0] == _ffi.NO_RESULT and o[0][0].tobytes() == bad[0].tobytes()
    # n_prob == 0
    o = gpu_ctx.refine_poses_batch(m, par, [], [], np.zeros((0, 6)), 1.0, 4)
    assert all(len(v) == 0 for v in o)


# ---- 5. independence and determinism -----------------------------------------------------------------------------------------------
def test_independence_and_determinism(gpu_ctx):
    sp, m, par, X, U, poses0 = _noisy_inputs(gpu_ctx, "eucm")
    X, U, poses0 = X[:9], U[:9], poses0[:9].copy()
    probe = (X[4], U[4], poses0[4:5])
    alone = gpu_ctx.refine_poses_batch(m, par, [probe[0]], [probe[1]], probe[2], 1.0, 4, _tight(), with_errors=True)
    for pos in (0, 4, 8):
        Xb, Ub, pb = list(X), list(U), poses0.copy()
        Xb[pos], Ub[pos], pb[pos] = probe[0], probe[1], probe[2][0]
        out = gpu_ctx.refine_poses_batch(m, par, Xb, Ub, pb, 1.0, 4, _tight(), with_errors=True)
        for i in range(6):
            assert np.asarray(out[i][pos]).tobytes() == np.asarray(alone[i][0]).tobytes(), (pos, i)
        assert out[6][pos].tobytes() == alone[6][0].tobytes()
    a = gpu_ctx.refine_poses_batch(m, par, X, U, poses0, 1.0, 4, _tight(), with_errors=True)
    b = gpu_ctx.refine_poses_batch(m, par, X, U, poses0, 1.0, 4, _tight(), with_errors=True)
    for i in range(6):
        assert a[i].tobytes() == b[i].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[6], b[6]))
    # a frame that starts 0.4 rad off beside frames that start at the optimum: each stops by its own rule
    at_opt = a[0].copy()
    at_opt[3, :3] += 0.4 / np.sqrt(3.0)
    mixed = gpu_ctx.refine_poses_batch(m, par, X, U, at_opt, 1.0, 4, _tight())
    own = [gpu_ctx.refine_poses_batch(m, par, [X[f]], [U[f]], at_opt[f:f + 1], 1.0, 4, _tight())[2][0] for f in range(9)]
    print("iterations in the batch", mixed[2].tolist(), "alone", own)
    assert mixed[2].tolist() == own
    assert mixed[2][3] > np.delete(mixed[2], 3).max()


# ---- 6. loss switch ------------------------------------------------------------------------------------------------------------------
def test_no_loss_equals_a_huge_delta(gpu_ctx):
    sp = synth.make_problem(8, "kb4", noise_px=0.1, ragged=True)
    m, par = _params(sp)
    X = [sp.p3d[a:b].astype(np.float64) for a, b in _frames(sp)]
    U = [sp.p2d[a:b].astype(np.float64) for a, b in _frames(sp)]
    ref = gpu_ctx.refine_poses_batch(m, par, X, U, sp.poses0, 1e6, 4, _tight(), with_errors=True)
    for delta in (0.0, -1.0):
        out = gpu_ctx.refine_poses_batch(m, par, X, U, sp.poses0, delta, 4, _tight(), with_errors=True)
        for i in range(6):
            assert out[i].tobytes() == ref[i].tobytes(), (delta, i)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out[6], ref[6]))
    assert (ref[1] == OK_).all()


# ---- 7. arguments ------------------------------------------------------------------------------------------------------------------
def test_arguments(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    m, par, X, U, start, _ = _shape_frames([10, 12])
    par10 = np.zeros(synth.PMAX); par10[:len(par)] = par
    Xa, Ua = np.concatenate(X), np.concatenate(U)
    good = np.array([0, 10, 22], dtype=np.int64)
    poses = start.copy(); st = np.full(2, -7, dtype=np.int32); it = np.full(2, -7, dtype=np.int32); nu = np.full(2, -7, dtype=np.int32)
    c0 = np.full(2, -7.0); c1 = np.full(2, -7.0); err = np.full(22, -7.0)

    def call(model=m, offs=good, po=poses, status=st, params=par10, n=2):
        return lib.ccal_refine_poses_batch(h, model, dp(params) if params is not None else None, 1.0, n,
                                           lp(offs) if offs is not None else None, dp(Xa), dp(Ua), 4, None,
                                           dp(po) if po is not None else None, ip(status) if status is not None else None,
                                           ip(it), ip(nu), dp(c0), dp(c1), dp(err))
    assert call(offs=np.array([1, 10, 22], dtype=np.int64)) == _ffi.ERR_INVALID_ARG
    assert call(offs=np.array([0, 12, 10], dtype=np.int64)) == _ffi.ERR_INVALID_ARG
    assert call(offs=None) == _ffi.ERR_INVALID_ARG
    assert call(po=None) == _ffi.ERR_INVALID_ARG
    assert call(status=None) == _ffi.ERR_INVALID_ARG
    assert call(params=None) == _ffi.ERR_INVALID_ARG
    assert call(model=17) == _ffi.ERR_INVALID_ARG
    assert call(model=-1) == _ffi.ERR_INVALID_ARG
    assert call(n=-1) == _ffi.ERR_INVALID_ARG
    assert call(model=api.MODEL_EUCMT) == _ffi.ERR_UNSUPPORTED
    assert poses.tobytes() == start.tobytes()
    assert (st == -7).all() and (it == -7).all() and (nu == -7).all() and (c0 == -7).all() and (c1 == -7).all() and (err == -7).all()
    assert call() == _ffi.OK and (st == OK_).all() and (err >= 0).all()
    with pytest.raises(CcalError):
        api.refine_poses([None], api.GenericModel("eucmt", [1.0] * 8, 512, 512))


# ---- 8. held-out validation ----------------------------------------------------------------------------------------------------------
def test_validation_holdout(gpu_ctx):
    sp = synth.make_problem(40, "eucm", noise_px=0.1)
    frames = api.frames_from_synth(sp)
    cam0 = api.GenericModel("eucm", sp.intr0[0, :6], 512, 512)
    fit = api.calib_camera([f if i % 2 == 0 else None for i, f in enumerate(frames)], cam0, False, 0, False,
                           {i: api.RvecTvec.from6(sp.poses0[i]) for i in range(0, 40, 2)}, ctx=gpu_ctx)
    assert fit is not None
    held = [f if i % 2 == 1 else None for i, f in enumerate(frames)]
    refined = api.refine_poses(held, fit[0], ctx=gpu_ctx)
    assert sorted(refined) == list(range(1, 40, 2))
    assert api.validation_holdout(0, fit[0], held, ctx=gpu_ctx) == api.validation(0, fit[0], refined, held, ctx=gpu_ctx)
    # with the true intrinsics the refined poses fit the held-out frames no worse than the ground-truth poses do
    true_cam = api.GenericModel("eucm", sp.intr_gt[0, :6], 512, 512)
    avg, med = api.validation_holdout(0, true_cam, held, ctx=gpu_ctx)
    avg_gt, med_gt = api.validation(0, true_cam, {i: api.RvecTvec.from6(sp.poses_gt[i]) for i in range(1, 40, 2)}, held, ctx=gpu_ctx)
    print(f"held-out median {med:.4f} px (ground-truth poses {med_gt:.4f}), fitted model {api.validation_holdout(0, fit[0], held, ctx=gpu_ctx)}")
    assert med <= med_gt


# ---- 9. poisoned memory ------------------------------------------------------------------------------------------------------------
def _run_refine_noisy(ctx):
    sp, m, par, X, U, poses0 = _noisy_inputs(ctx, "eucm")
    out = ctx.refine_poses_batch(m, par, X, U, poses0, 1.0, 4, _tight(), with_errors=True)
    res = {k: out[i] for i, k in enumerate(["poses", "status", "iters", "used", "cost0", "cost"])}
    res["err"] = np.concatenate(out[6])
    return res


def test_poisoned_memory():
    """Case 2's EUCM half on a context of the second library with every block of doubles pre-filled with NaN, in a fresh process,
    against the same run without the hook (the harness of tests/test_gpu_poison.py, imported as it is)."""
    import test_gpu_poison as tp
    res = tp._poisoned_and_clean(_run_refine_noisy)
    assert (res["status"] == OK_).all()
