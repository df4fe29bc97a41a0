"""GPU: pose initialisation for targets that are not a z = 0 plane and the batched general PnP (ccal_pnp_batch, k_pose_pnp in
csrc/ccal_kernels_pnp.hip) - against ground truth, against the numpy yardstick tests/pnp_ref.py (same cost, 512 random starts, LM to
a stalled step), against the planar estimator on planar input, on the shapes where the lane loops and the four-wavefront workgroup
can go wrong, and for determinism."""
import ctypes as C
import functools

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth
from camera_intrinsic_calibration_rs_amd.engine import CcalError, Problem, default_opts, make_desc

import pnp_ref

pytestmark = pytest.mark.gpu

TARGETS = {"hinged": synth.hinged_boards, "offset": synth.offset_board, "cube": lambda: synth.cube_points(100)}

# Worst difference to the yardstick over the 3 x 40 noisy frames of test_pnp_batch_against_the_yardstick, measured on an MI355X
# (EXPERIMENTS.md): rotation-matrix entries 5.6e-9 (offset board), translation 1.42e-9 m - the
# yardstick's own resolution: comparing costs resolves a minimum of E to the square root of E's rounding, the kernel's last steps
# solve for the zero of the gradient.  Asserted at 10 x that (and never looser than 1e-6): the
# margin covers the summation order and the fixed iteration count.
POSE_DIFF_R = 10 * 5.6e-9
POSE_DIFF_T = 10 * 1.42e-9
assert POSE_DIFF_R <= 1e-6 and POSE_DIFF_T <= 1e-6


def _frames(sp):
    return [(int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])) for o in range(sp.n_obs)]


def _normalised(ctx, sp, cam=0):
    """x / z, y / z of the library's own unprojection of every detection (all valid at the true intrinsics)."""
    m = int(sp.model[cam])
    rays, valid = ctx.unproject_points(m, sp.intr_gt[cam, :synth.MODEL_NPARAMS[m]], sp.p2d.astype(np.float64))
    assert valid.all()
    return rays[:, :2] / rays[:, 2:3]


def _angle(R, Rg):
    """Rotation angle between R and Rg, from |R - Rg|_F = 2 sqrt 2 sin(angle / 2) (the arccos of the trace cannot see below 1e-8)."""
    return 2.0 * np.arcsin(np.clip(np.sqrt(((R - Rg) ** 2).sum(axis=(-2, -1)) / 8.0), 0.0, 1.0))


@functools.lru_cache(maxsize=None)
def _yardstick_noisy(target, xn_bytes, n_rows):
    """The yardstick's (R, t, E) for the 40 noisy frames of a target: computed once, shared, never changed."""
    sp = synth.make_problem(40, "eucm", board=TARGETS[target](), ragged=True)
    xn = np.frombuffer(xn_bytes).reshape(n_rows, 2)
    return [pnp_ref.solve(sp.p3d[a:b].astype(np.float64), xn[a:b]) for a, b in _frames(sp)]


# ---- 1. init_poses on a hinged target, every model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["ucm", "eucm", "kb4", "opencv5"])
def test_init_poses_hinged_boards_close_to_ground_truth(gpu_ctx, model):
    sp = synth.make_problem(30, model, board=synth.hinged_boards(), ragged=True)
    gp = Problem.from_synth(gpu_ctx, sp)
    poses, used = gp.init_poses(sp.intr_gt)
    gp.close()
    assert (used == np.diff(sp.obs_offsets)).all(), used
    ang = _angle(synth.rodrigues(poses[:, :3]), synth.rodrigues(sp.poses_gt[:, :3]))
    dt = np.abs(poses[:, 3:] - sp.poses_gt[:, 3:]).max()
    print(f"{model}: rotation {ang.max():.2e} rad, translation {dt:.2e} m")
    assert ang.max() < 0.02, ang.max()                  # the bounds of tests/test_gpu_init.py for the planar estimator, same noise
    assert dt < 0.01, dt


# ---- 2. calib_camera as the reference calls it ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["eucm", "kb4"])
@pytest.mark.parametrize("target", ["hinged", "offset"])
def test_calib_camera_without_initial_poses_nonplanar(gpu_ctx, target, model):
    sp = synth.make_problem(30, model, board=TARGETS[target]())
    P = synth.MODEL_NPARAMS[synth.MODEL_NAMES[model]]
    frames = api.frames_from_synth(sp)
    cam0 = api.GenericModel(model, sp.intr0[0, :P], 512, 512)
    tight = default_opts(0, min_abs_error_decrease=1e-10, min_rel_error_decrease=1e-12)
    a = api.calib_camera(frames, cam0, False, 0, False, None, ctx=gpu_ctx, opts=tight)
    b = api.calib_camera(frames, cam0, False, 0, False, {i: api.RvecTvec.from6(sp.poses0[i]) for i in range(30)},
                         ctx=gpu_ctx, opts=tight)
    assert a is not None and b is not None
    assert sorted(a[1]) == list(range(30))               # every frame got a starting pose
    assert np.abs(a[0].params() / b[0].params() - 1)[:4].max() < 1e-6
    pa = np.stack([a[1][i].as6() for i in range(30)]); pb = np.stack([b[1][i].as6() for i in range(30)])
    np.testing.assert_allclose(synth.rodrigues(pa[:, :3]), synth.rodrigues(pb[:, :3]), atol=1e-6)
    np.testing.assert_allclose(pa[:, 3:], pb[:, 3:], atol=1e-6)


# ---- 3. ccal_pnp_batch against the yardstick -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", sorted(TARGETS))
def test_pnp_batch_against_the_yardstick(gpu_ctx, target):
    """40 noisy frames (0.1 px).  Both sides claim the global minimum of the same E, which is flat to second order there: E recomputed
    in numpy from the returned pose may exceed the yardstick's by a relative 1e-6 at most.  cost_out is the quadratic form
    vec(R)^T Omega vec(R): entries of Omega ~ n x 0.1, E ~ 1e-5, so cancellation leaves it ~1e-10 relative - held to the same 1e-6."""
    sp = synth.make_problem(40, "eucm", board=TARGETS[target](), ragged=True)
    xn = _normalised(gpu_ctx, sp)
    fr = _frames(sp)
    X = [sp.p3d[a:b].astype(np.float64) for a, b in fr]
    poses, used, cost = gpu_ctx.pnp_batch(X, [xn[a:b] for a, b in fr], 4)
    ref = _yardstick_noisy(target, np.ascontiguousarray(xn).tobytes(), len(xn))
    assert (used == np.diff(sp.obs_offsets)).all()
    R = synth.rodrigues(poses[:, :3])
    worst_e = worst_c = worst_r = worst_t = 0.0
    for f, (a, b) in enumerate(fr):
        Rr, tr, Er = ref[f]
        Eg = pnp_ref.cost(X[f], xn[a:b], R[f], poses[f, 3:])
        worst_e = max(worst_e, Eg / Er - 1); worst_c = max(worst_c, abs(cost[f] / Eg - 1))
        worst_r = max(worst_r, np.abs(R[f] - Rr).max()); worst_t = max(worst_t, np.abs(poses[f, 3:] - tr).max())
    print(f"{target}: E/E_ref - 1 <= {worst_e:.2e}, |cost_out/E - 1| <= {worst_c:.2e}, dR {worst_r:.2e}, dt {worst_t:.2e}")
    assert worst_e <= 1e-6, worst_e
    assert worst_c <= 1e-6, worst_c
    assert worst_r <= POSE_DIFF_R, worst_r
    assert worst_t <= POSE_DIFF_T, worst_t
    # the estimate is as good as the noise allows (the planar estimator's bounds)
    assert _angle(R, synth.rodrigues(sp.poses_gt[:, :3])).max() < 0.02 and np.abs(poses[:, 3:] - sp.poses_gt[:, 3:]).max() < 0.01


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_pnp_batch_noise_free_against_ground_truth(gpu_ctx, target):
    """20 noise-free frames, true normalised points: the error against ground truth may be 10 x the yardstick's own on the same frames,
    and never more than 1e-3 rad / 1e-3 m - anything above that is a wrong basin, not rounding."""
    sp = synth.make_problem(20, "eucm", noise_px=0, board=TARGETS[target]())
    fr = _frames(sp)
    X = [sp.p3d[a:b].astype(np.float64) for a, b in fr]
    xn = [pnp_ref.true_normalised_points(X[f], sp.poses_gt[f]) for f in range(20)]
    poses, used, _ = gpu_ctx.pnp_batch(X, xn, 4)
    assert (used == np.diff(sp.obs_offsets)).all()
    Rg = synth.rodrigues(sp.poses_gt[:, :3])
    ref = [pnp_ref.solve(X[f], xn[f]) for f in range(20)]
    ref_ang = max(float(_angle(r[0], Rg[f])) for f, r in enumerate(ref))
    ref_dt = max(np.abs(r[1] - sp.poses_gt[f, 3:]).max() for f, r in enumerate(ref))
    ang = _angle(synth.rodrigues(poses[:, :3]), Rg).max()
    dt = np.abs(poses[:, 3:] - sp.poses_gt[:, 3:]).max()
    print(f"{target}: kernel {ang:.2e} rad {dt:.2e} m, yardstick {ref_ang:.2e} rad {ref_dt:.2e} m")
    assert ang <= min(10 * ref_ang, 1e-3), (ang, ref_ang)
    assert dt <= min(10 * ref_dt, 1e-3), (dt, ref_dt)


# ---- 4. the planar twin ----------------------------------------------------------------------------------------------------------------
def test_pnp_batch_on_the_planar_board_agrees_with_the_homography(gpu_ctx):
    sp = synth.make_problem(40, "eucm", ragged=True)
    gp = Problem.from_synth(gpu_ctx, sp)
    planar, used_planar = gp.init_poses(sp.intr_gt)
    gp.close()
    xn = _normalised(gpu_ctx, sp)
    fr = _frames(sp)
    poses, used, _ = gpu_ctx.pnp_batch([sp.p3d[a:b] for a, b in fr], [xn[a:b] for a, b in fr], 10)
    assert (used == used_planar).all() and (used > 0).all()
    assert np.abs(synth.rodrigues(poses[:, :3]) - synth.rodrigues(planar[:, :3])).max() < 5e-3      # two estimators: tests/test_gpu_init.py
    assert np.abs(poses[:, 3:] - planar[:, 3:]).max() < 5e-3
    R = synth.rodrigues(poses[:, :3])
    for f, (a, b) in enumerate(fr):                          # the mirror twin (same cost, behind the camera) lost everywhere
        z = sp.p3d[a:b].astype(np.float64) @ R[f, 2] + poses[f, 5]
        assert (z > 0).all(), f


# ---- 5. shapes where it can go wrong -----------------------------------------------------------------------------------------------------
def _one_pose_problem(counts, seed=0xABCD):
    """Frames of the given sizes, all of one noise-free pose of a 300-point cloud in a cube (EUCM ground truth)."""
    cloud = synth.cube_points(300, seed=seed).astype(np.float64)
    pose = synth.make_problem(1, "eucm", noise_px=0, board=cloud).poses_gt[0]
    X = [cloud[:n] for n in counts]
    return X, [pnp_ref.true_normalised_points(x, pose) for x in X], pose


def test_lane_loop_boundaries_and_workgroup_edges(gpu_ctx):
    counts = [4, 6, 63, 64, 65, 144, 300]
    X, xn, pose = _one_pose_problem(counts)
    Rg = synth.rodrigues(pose[:3])
    poses, used, cost = gpu_ctx.pnp_batch(X, xn, 4)
    assert used.tolist() == counts
    assert np.abs(synth.rodrigues(poses[:, :3]) - Rg).max() < 1e-6 and np.abs(poses[:, 3:] - pose[3:]).max() < 1e-6
    assert (cost >= 0).all() and (cost < 1e-12).all()
    for n_prob in (1, 3, 4, 5):                              # the four-wavefront workgroup's edge
        p, u, c = gpu_ctx.pnp_batch(X[2:2 + n_prob], xn[2:2 + n_prob], 4)
        assert p.shape == (n_prob, 6) and np.array_equal(p, poses[2:2 + n_prob]) and np.array_equal(u, used[2:2 + n_prob])
        assert np.array_equal(c, cost[2:2 + n_prob])
    p, u, c = gpu_ctx.pnp_batch([], [], 4)
    assert p.shape == (0, 6) and u.shape == (0,) and c.shape == (0,)


def test_invalid_arguments_launch_nothing(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    X = np.zeros((8, 3)); U = np.zeros((8, 2)); poses = np.full((2, 6), np.nan); used = np.full(2, -2, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = used.ctypes.data_as(C.POINTER(C.c_int32))
    good = np.array([0, 4, 8], dtype=np.int64)
    for offs in (np.array([1, 4, 8], dtype=np.int64), np.array([0, 6, 4], dtype=np.int64)):
        assert lib.ccal_pnp_batch(h, 2, lp(offs), dp(X), dp(U), 4, dp(poses), ip, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_pnp_batch(h, 2, None, dp(X), dp(U), 4, dp(poses), ip, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_pnp_batch(h, 2, lp(good), None, dp(U), 4, dp(poses), ip, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_pnp_batch(h, 2, lp(good), dp(X), None, 4, dp(poses), ip, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_pnp_batch(h, 2, lp(good), dp(X), dp(U), 4, None, ip, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_pnp_batch(h, 2, lp(good), dp(X), dp(U), 4, dp(poses), None, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_pnp_batch(h, -1, lp(good), dp(X), dp(U), 4, dp(poses), ip, None) == _ffi.ERR_INVALID_ARG
    assert np.isnan(poses).all() and (used == -2).all()      # nothing was written
    assert lib.ccal_pnp_batch(h, 0, None, None, None, 4, None, None, None) == _ffi.OK
    with pytest.raises(ValueError):
        gpu_ctx.pnp_batch([X], [U[:5]], 4)


def test_frames_without_a_pose_leave_their_neighbours_alone(gpu_ctx):
    """A three-point frame, a collinear frame, one image point for all, fewer than min_points: zeros and n_used 0; the good frames
    between them are bit-equal to a batch holding only them.  Nothing stays NaN."""
    X, xn, pose = _one_pose_problem([40, 40, 40, 40])
    good_p, good_u, good_c = gpu_ctx.pnp_batch(X[:3], xn[:3], 4)
    line = np.outer(np.linspace(-1.0, 1.0, 40), [0.3, 0.2, -0.1]) + [0.3, -0.3, -0.2]
    Xs = [X[0], X[0][:3], X[1], line, X[2], X[0], X[0][:9]]
    xs = [xn[0], xn[0][:3], xn[1], pnp_ref.true_normalised_points(line, pose), xn[2], np.tile(xn[0][:1], (40, 1)), xn[0][:9]]
    p, u, c = gpu_ctx.pnp_batch(Xs, xs, 4)
    assert not np.isnan(p).any() and not np.isnan(c).any() and (u >= 0).all()
    assert u.tolist() == [40, 0, 40, 0, 40, 0, 9]
    for k in (1, 3, 5):
        assert (p[k] == 0).all() and c[k] == 0
    assert np.array_equal(p[[0, 2, 4]], good_p) and np.array_equal(c[[0, 2, 4]], good_c)
    p10, u10, _ = gpu_ctx.pnp_batch(Xs, xs, 10)              # min_points 10: the nine-point frame goes too
    assert u10.tolist() == [40, 0, 40, 0, 40, 0, 0] and (p10[6] == 0).all()


def _behind_the_camera(cloud, pose):
    """The cloud mirrored in the camera's z = 0 plane and taken back to board coordinates: the given pose fits it exactly (E = 0),
    with every point at negative depth."""
    R = synth.rodrigues(pose[:3])
    pc = (cloud @ R.T + pose[3:]) * np.array([1.0, 1.0, -1.0])
    return (pc - pose[3:]) @ R, pc[:, :2] / pc[:, 2:3]


def test_a_behind_the_camera_frame_gives_no_pose(gpu_ctx):
    """A frame whose points lie behind the camera gives zeros and n_used 0, its neighbours unaffected.  The pose that generated it
    fits exactly (E = 0) at negative depth; E has other, poor local minima in front of the camera (E = 0.19 here - the yardstick,
    which only takes the lowest cost with positive summed depth, returns that one), and the library's rule for "no candidate in
    front" (ccal.h) sets them aside when a candidate behind the camera fits that much better."""
    X, xn, pose = _one_pose_problem([40, 40])
    Xb, xb = _behind_the_camera(X[0], pose)
    p, u, c = gpu_ctx.pnp_batch([X[0], Xb, X[1]], [xn[0], xb, xn[1]], 4)
    good = gpu_ctx.pnp_batch(X, xn, 4)
    print(f"behind the camera: n_used {u[1]}, E {c[1]:.3g}, yardstick {'no pose' if pnp_ref.solve(Xb, xb) is None else 'a pose'}")
    assert np.array_equal(p[[0, 2]], good[0]) and np.array_equal(u[[0, 2]], good[1])
    assert u[1] == 0 and (p[1] == 0).all() and c[1] == 0


def _raw_init_poses(gp, intr, min_points=10, division=None):
    """ccal_init_poses / ccal_init_poses_division into buffers the test filled with NaN and -2."""
    poses = np.full((gp.n_obs, 6), np.nan); used = np.full(gp.n_obs, -2, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = used.ctypes.data_as(C.POINTER(C.c_int32))
    if division is None:
        rc = gp.lib.ccal_init_poses(gp.handle, dp(np.ascontiguousarray(intr, dtype=np.float64)), min_points, dp(poses), ip)
    else:
        rc = gp.lib.ccal_init_poses_division(gp.handle, float(division), min_points, dp(poses), ip)
    assert rc == _ffi.OK
    return poses, used


def _concat(sps, order):
    """Frames of several single-camera problems interleaved into one description: order = [(problem index, frame)]."""
    offs, X, U = [0], [], []
    for k, f in order:
        a, b = sps[k].obs_offsets[f], sps[k].obs_offsets[f + 1]
        X.append(sps[k].p3d[a:b]); U.append(sps[k].p2d[a:b]); offs.append(offs[-1] + b - a)
    X = np.concatenate(X); U = np.concatenate(U)
    n = len(order)
    return make_desc(1, [1], [512.0], [512.0], False, n, [0] * n, list(range(n)), offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)


def test_planar_and_nonplanar_frames_in_one_call(gpu_ctx):
    flat = synth.make_problem(6, "eucm", ragged=True)
    hinged = synth.make_problem(5, "eucm", board=synth.hinged_boards(), ragged=True, seed=77)
    order = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 4), (1, 4), (0, 5)]
    d, keep = _concat([flat, hinged], order)
    gp = Problem(gpu_ctx, d, keep)
    poses, used = _raw_init_poses(gp, flat.intr_gt)
    gp.close()
    assert not np.isnan(poses).any() and (used > 0).all()
    gf = Problem.from_synth(gpu_ctx, flat)
    flat_poses, flat_used = gf.init_poses(flat.intr_gt)
    gf.close()
    gh = Problem.from_synth(gpu_ctx, hinged)
    hinged_poses, hinged_used = gh.init_poses(hinged.intr_gt)
    gh.close()
    for row, (k, f) in enumerate(order):                     # planar frames: the bits of a call on a problem holding only them
        want_p, want_u = (flat_poses, flat_used) if k == 0 else (hinged_poses, hinged_used)
        assert np.array_equal(poses[row], want_p[f]) and used[row] == want_u[f], (row, k, f)
    ang = _angle(synth.rodrigues(hinged_poses[:, :3]), synth.rodrigues(hinged.poses_gt[:, :3]))
    assert ang.max() < 0.02 and np.abs(hinged_poses[:, 3:] - hinged.poses_gt[:, 3:]).max() < 0.01


def test_second_camera_of_a_rig_and_the_sharded_call(gpu_ctx):
    sp = synth.make_problem(9, "eucm", n_cams=2, board=synth.hinged_boards())
    gp = Problem.from_synth(gpu_ctx, sp)
    poses, used = _raw_init_poses(gp, sp.intr_gt)
    gp.close()
    assert not np.isnan(poses).any() and (used == 288).all()
    # T_cam_board of camera c = T_c0 * T_0_board
    Rc = synth.rodrigues(sp.extr_gt[:, :3]); Rb = synth.rodrigues(sp.poses_gt[:, :3])
    for o in range(sp.n_obs):
        c, s = int(sp.obs_cam[o]), int(sp.obs_slot[o])
        Rg = Rc[c] @ Rb[s]; tg = Rc[c] @ sp.poses_gt[s, 3:] + sp.extr_gt[c, 3:]
        assert _angle(synth.rodrigues(poses[o, :3]), Rg) < 0.02 and np.abs(poses[o, 3:] - tg).max() < 0.01, o
    from camera_intrinsic_calibration_rs_amd.engine import MultiContext, MultiProblem
    mctx = MultiContext([0, 0])
    try:
        mp = MultiProblem.from_synth(mctx, sp)
        mposes, mused = mp.init_poses(sp.intr_gt)
        mp.close()
    finally:
        mctx.close()
    assert np.array_equal(mposes, poses) and np.array_equal(mused, used)


def test_init_poses_division_on_a_pinhole_exact_hinged_target(gpu_ctx):
    """lambda = 0: the division model is a pinhole with f = max(w, h) / 2 and the centre at (w / 2, h / 2)."""
    board = synth.hinged_boards().astype(np.float64)
    sp = synth.make_problem(7, "opencv5", noise_px=0, board=board)
    half = 256.0
    offs, X, U = [0], [], []
    for f in range(7):
        pc = board @ synth.rodrigues(sp.poses_gt[f, :3]).T + sp.poses_gt[f, 3:]
        X.append(board); U.append(half * pc[:, :2] / pc[:, 2:3] + half); offs.append(offs[-1] + len(board))
    X = np.concatenate(X).astype(np.float32); U = np.concatenate(U).astype(np.float32)
    d, keep = make_desc(1, [0], [512.0], [512.0], False, 7, [0] * 7, list(range(7)), offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    gp = Problem(gpu_ctx, d, keep)
    poses, used = _raw_init_poses(gp, None, 4, division=0.0)
    gp.close()
    assert not np.isnan(poses).any() and (used == 288).all()
    # f32 detections: ~3e-5 px / 256 per coordinate, far inside the planar estimator's bounds
    assert _angle(synth.rodrigues(poses[:, :3]), synth.rodrigues(sp.poses_gt[:, :3])).max() < 1e-4
    assert np.abs(poses[:, 3:] - sp.poses_gt[:, 3:]).max() < 1e-4


def test_solve_pnp_is_the_reference_shaped_call(gpu_ctx):
    X, xn, pose = _one_pose_problem([50])
    rt = api.solve_pnp(X[0], xn[0], ctx=gpu_ctx)
    assert rt is not None
    assert np.abs(synth.rodrigues(np.array(rt[0])) - synth.rodrigues(pose[:3])).max() < 1e-6 and np.abs(np.array(rt[1]) - pose[3:]).max() < 1e-6
    assert api.solve_pnp(X[0][:3], xn[0][:3], ctx=gpu_ctx) is None


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_whatever_else_is_in_the_batch(gpu_ctx):
    sp = synth.make_problem(12, "eucm", board=synth.hinged_boards(), ragged=True)
    xn = _normalised(gpu_ctx, sp)
    fr = _frames(sp)
    X = [sp.p3d[a:b] for a, b in fr]; U = [xn[a:b] for a, b in fr]
    a = gpu_ctx.pnp_batch(X, U, 4)
    b = gpu_ctx.pnp_batch(X, U, 4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    alone = gpu_ctx.pnp_batch(X[5:6], U[5:6], 4)
    rev = gpu_ctx.pnp_batch(X[::-1], U[::-1], 4)
    for k in range(3):
        assert np.array_equal(alone[k][0], a[k][5]) and np.array_equal(rev[k][::-1], a[k])
    gp = Problem.from_synth(gpu_ctx, sp)
    p1, u1 = gp.init_poses(sp.intr_gt); p2, u2 = gp.init_poses(sp.intr_gt)
    gp.close()
    assert np.array_equal(p1, p2) and np.array_equal(u1, u2)
