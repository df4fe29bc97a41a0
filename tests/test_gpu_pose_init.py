"""GPU: the planar pose initialiser k_pose_init (csrc/ccal_kernels_init.hip) held to its yardstick tests/pose_init_ref.py - the same
least-squares problem solved by Householder QR in long double from the same f32 inputs - through every entry point that launches
it: ccal_init_poses, ccal_init_poses_division, ccal_multi_init_poses, api.init_pose and api.calib_camera(..., None).  The frames
come from tests/pose_init_cases.py; tests/test_pose_init_cpu.py checks the yardstick and the frames on a CPU.

The comparison rule, per frame with a pose: max |R_dev - R_ref| <= F kappa^2 u and |t_dev - t_ref| <= F kappa^2 u |t_ref| with
u = 2^-53 and kappa the yardstick's condition number of the column-scaled design (normal equations square it); rotations are
compared as matrices, since rvecs near pi are two names for one rotation.  `used` must equal the yardstick's count of valid
corners; a frame without a pose has used == 0 and six zeros.

F: the f64 emulation of the kernel's arithmetic (pose_init_ref.emulate_f64) against the yardstick over the whole case list gave
a worst err / (kappa^2 u) of 0.694 (frame opencv5-n63-2); F = 4 x that, rounded up to a power of two = 4.  The margin is for the
device's summation order and contraction to fma.  test_pose_init_cpu.py::test_tolerance_factor_follows_its_rule re-measures it.

The invalid corners of case 3: a frame of 12 or 13 corners has no lane 63, so beside the frames of 12 (9 valid) and 13 (10 valid)
there are three of 130 corners whose invalid corners sit at 0, at 63, and at 64, 127 and 128."""
import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import api, synth
from camera_intrinsic_calibration_rs_amd.engine import MultiContext, MultiProblem, Problem, default_opts, make_desc

import pose_init_cases as cases
import pose_init_ref as ref

pytestmark = pytest.mark.gpu

MODELS = {"ucm": cases.UCM, "eucm": cases.EUCM, "kb4": cases.KB4, "opencv5": cases.OPENCV5}


def _desc(frames):
    """One description of the frames in order: cameras from f["cam"] (one camera without it), one slot per frame unless f["slot"]."""
    cams = sorted({f.get("cam", 0) for f in frames})
    model = [next(f["model"] for f in frames if f.get("cam", 0) == c) for c in cams]
    model = [cases.UCM if m == cases.DIVISION else m for m in model]        # the division model is no camera model: any will do
    slots = [f.get("slot", k) for k, f in enumerate(frames)]
    offs = np.concatenate([[0], np.cumsum([len(f["X"]) for f in frames])])
    X = np.concatenate([f["X"] for f in frames]); U = np.concatenate([f["uv"] for f in frames])
    return make_desc(len(cams), model, [cases.W] * len(cams), [cases.H] * len(cams), False, max(slots) + 1,
                     [f.get("cam", 0) for f in frames], slots, offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)


def _intr(frames):
    cams = sorted({f.get("cam", 0) for f in frames})
    intr = np.zeros((len(cams), synth.PMAX))
    for f in frames:
        if f["model"] != cases.DIVISION:
            intr[f.get("cam", 0), :len(f["params"])] = f["params"]
    return intr


def _run(ctx, frames, min_points=10):
    d, keep = _desc(frames)
    gp = Problem(ctx, d, keep)
    try:
        if frames[0]["model"] == cases.DIVISION:
            return gp.init_poses_division(cases.DIVISION_LAMBDA, min_points)
        return gp.init_poses(_intr(frames), min_points)
    finally:
        gp.close()


def _hold(frames, poses, used, min_points=10, label=""):
    """The comparison rule of the module docstring over every frame; prints the worst figures before it asserts."""
    assert poses.shape == (len(frames), 6) and not np.isnan(poses).any()
    worst_r = worst_t = 0.0
    bad = []
    for k, f in enumerate(frames):
        r = cases.reference(f, min_points)
        if r is None:
            if used[k] != 0 or poses[k].any():
                bad.append((f["name"], "a pose where the yardstick has none", int(used[k])))
            continue
        if used[k] != r["used"]:
            bad.append((f["name"], "used", int(used[k]), r["used"]))
            continue
        er, et = cases.pose_errors(synth.rodrigues(poses[k, :3]), poses[k, 3:], r)
        worst_r, worst_t = max(worst_r, er), max(worst_t, et)
        if er > cases.F or et > cases.F:
            bad.append((f["name"], er, et, r["kappa"]))
    print(f"{label}: worst rotation {worst_r:.3g}, translation {worst_t:.3g} x kappa^2 u (F = {cases.F})")
    assert not bad, bad


# ---- 1. lane and loop edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(MODELS))
def test_lane_and_loop_edges(gpu_ctx, model):
    """10 .. 257 corners, 13 frames (three workgroups and one wavefront); then the first 1, 4 and 5 of them as problems of their own
    (a last workgroup with three, no and three idle wavefronts): the same bits."""
    frames = cases.lane_frames(MODELS[model])
    poses, used = _run(gpu_ctx, frames)
    assert used.tolist() == [len(f["X"]) for f in frames]
    _hold(frames, poses, used, label=f"lanes {model}")
    for n in (1, 4, 5):
        p, u = _run(gpu_ctx, frames[:n])
        assert np.array_equal(p, poses[:n]) and np.array_equal(u, used[:n]), n


# ---- 8. position independence ----------------------------------------------------------------------------------------------------
def test_reversed_order_gives_the_same_bits(gpu_ctx):
    for model in (cases.EUCM, cases.KB4):
        frames = cases.lane_frames(model)
        poses, used = _run(gpu_ctx, frames)
        p, u = _run(gpu_ctx, frames[::-1])
        assert np.array_equal(p[::-1], poses) and np.array_equal(u[::-1], used)


# ---- 2. every rotation branch ----------------------------------------------------------------------------------------------------
def test_every_rotation_branch(gpu_ctx):
    """Angle 0, 1e-9, the four-way tie at 2 pi / 3 about (1, 1, 1), and pi - 1e-3 about +-x, +-y, +-z, +-(1, 1, 0): each of the four
    matrix -> quaternion branches with and without the qw < 0 flip (test_pose_init_cpu.py asserts which frame takes which)."""
    frames = cases.rotation_frames()
    poses, used = _run(gpu_ctx, frames)
    assert (used == 144).all()
    assert (np.linalg.norm(poses[:, :3], axis=1) <= np.pi + 1e-12).all()
    _hold(frames, poses, used, label="rotations")


# ---- 3. the count of valid corners -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["eucm", "division"])
def test_count_of_valid_corners(gpu_ctx, model):
    frames = cases.count_frames(cases.EUCM if model == "eucm" else cases.DIVISION)
    poses, used = _run(gpu_ctx, frames)
    assert used.tolist() == [0, 0, 0, 10, 10, 10, 129, 129, 127, 0], used
    _hold(frames, poses, used, label=f"counts {model}")
    poses4, used4 = _run(gpu_ctx, frames, 4)                  # min_points 4: the 9-corner frames and the exactly determined one
    assert used4.tolist() == [9, 9, 9, 10, 10, 10, 129, 129, 127, 4], used4
    _hold(frames, poses4, used4, 4, label=f"counts {model}, min_points 4")
    assert np.array_equal(poses4[3:9], poses[3:9])
    poses5, used5 = _run(gpu_ctx, frames, 5)
    assert used5[9] == 0 and not poses5[9].any()


def test_api_init_pose_is_the_same_estimate(gpu_ctx):
    """api.init_pose (min_points 4, the division model) on the 13-corner frame with 3 corners outside the domain."""
    f = cases.count_frames(cases.DIVISION)[4]
    ff = api.FrameFeature(0, (int(cases.W), int(cases.H)),
                          {k: api.FeaturePoint(tuple(f["uv"][k]), tuple(f["X"][k])) for k in range(len(f["X"]))})
    rvec, tvec = api.init_pose(ff, cases.DIVISION_LAMBDA, ctx=gpu_ctx)
    _hold([f], np.array([list(rvec) + list(tvec)]), np.array([10]), 4, label="api.init_pose")


# ---- 4. conditioning -------------------------------------------------------------------------------------------------------------
def test_conditioning(gpu_ctx):
    """Metres, millimetres, the board's origin 10 m and 100 m away in its own plane (kappa 1e4 and 3e5; at 100 m the origin lies
    behind the camera's plane while the corners are in front of it), 5 m away tilted 75 degrees."""
    frames = cases.conditioning_frames()
    poses, used = _run(gpu_ctx, frames)
    assert (used == 144).all()
    _hold(frames, poses, used, label="conditioning")
    for k, f in enumerate(frames):                              # the corners in front of the camera, whatever the origin's depth
        z = f["X"].astype(np.float64) @ synth.rodrigues(poses[k, :3])[2] + poses[k, 5]
        assert (z > 0).all(), f["name"]


# ---- 5. noise --------------------------------------------------------------------------------------------------------------------
def test_noisy_detections(gpu_ctx):
    """0.1 px: the yardstick solves the same noisy system, the rule is unchanged."""
    for model in (cases.UCM, cases.EUCM, cases.KB4, cases.OPENCV5):
        frames = [f for f in cases.noisy_frames() if f["model"] == model]
        poses, used = _run(gpu_ctx, frames)
        _hold(frames, poses, used, label=f"noisy {cases.MODEL_NAME[model]}")


# ---- 6. rank deficiency ----------------------------------------------------------------------------------------------------------
def test_corners_that_do_not_span_the_plane_give_no_pose(gpu_ctx):
    """One row, one column, one diagonal, one corner twelve times, two corners six times each - noise-free and at three seeds of
    0.1 px: used 0 and six zeros.  Between them two frames that barely span the plane and must match the yardstick."""
    bad, good = cases.degenerate_frames()
    frames = bad[:10] + [good[0]] + bad[10:] + [good[1]]
    poses, used = _run(gpu_ctx, frames)
    got = {f["name"]: int(used[k]) for k, f in enumerate(frames) if used[k]}
    print("frames with a pose:", got)
    assert got == {"two-rows": 24, "row-plus-two": 14}, got
    _hold(frames, poses, used, label="rank deficiency")
    p1, u1 = _run(gpu_ctx, [cases.row_plus_one()])            # rank 7 at exact detections, 1e-14 through their f32 rounding
    assert u1[0] == 0 and not p1.any()


# ---- 7. two cameras of different models ------------------------------------------------------------------------------------------
def test_two_cameras_of_different_models(gpu_ctx):
    frames = cases.two_camera_frames()
    d, keep = _desc(frames)
    gp = Problem(gpu_ctx, d, keep)
    poses, used = gp.init_poses(_intr(frames))
    gp.close()
    _hold(frames, poses, used, label="KB4 + EUCM")
    mctx = MultiContext([0, 0])
    try:
        d, keep = _desc(frames)
        mp = MultiProblem(mctx, d, keep)
        mposes, mused = mp.init_poses(_intr(frames))
        mp.close()
    finally:
        mctx.close()
    assert np.array_equal(mposes, poses) and np.array_equal(mused, used)


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------------
def test_calib_camera_drops_a_one_row_frame(gpu_ctx):
    """A 30-frame session plus one noisy one-row frame, no initial poses: the intrinsics and poses of the session without it."""
    sp = cases.e2e_session()
    frames = api.frames_from_synth(sp)
    f = cases.e2e_row_frame()
    row = api.FrameFeature(0, (512, 512), {k: api.FeaturePoint(tuple(f["uv"][k]), tuple(f["X"][k])) for k in range(len(f["X"]))})
    cam0 = api.GenericModel("eucm", sp.intr0[0, :6], 512, 512)
    tight = default_opts(0, min_abs_error_decrease=1e-10, min_rel_error_decrease=1e-12)
    a = api.calib_camera(frames + [row], cam0, False, 0, False, None, ctx=gpu_ctx, opts=tight)
    b = api.calib_camera(frames, cam0, False, 0, False, None, ctx=gpu_ctx, opts=tight)
    assert a is not None and b is not None
    assert sorted(a[1]) == list(range(30)) and sorted(b[1]) == list(range(30))
    assert np.abs(a[0].params() / b[0].params() - 1)[:4].max() < 1e-6
    pa = np.stack([a[1][i].as6() for i in range(30)]); pb = np.stack([b[1][i].as6() for i in range(30)])
    np.testing.assert_allclose(synth.rodrigues(pa[:, :3]), synth.rodrigues(pb[:, :3]), atol=1e-6)
    np.testing.assert_allclose(pa[:, 3:], pb[:, 3:], atol=1e-6)
