"""CPU: the numpy yardstick of the rig's pose refinement (tests/rig_refine_ref.py) holds on its own - with one camera and a zero
extrinsic it is tests/refine_ref.py, its gradient vanishes at the exact pose of exact data seen through several cameras, it converges
on every noisy slot of the GPU test and its figures there are the ones that test records -, api.refine_rig_poses sorts out the
frames it cannot use before anything reaches the library and starts every camera through its own T_c_0, and the kernel compiles for
gfx950 without scratch memory."""
import os
import re
import subprocess

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import api, synth

import refine_ref
import rig_refine_cases as cases
import rig_refine_ref


def test_one_camera_zero_extrinsic_is_the_single_camera_yardstick():
    sp = synth.make_problem(3, "kb4", noise_px=0.1, ragged=True, outlier_frac=0.05)
    m = int(sp.model[0])
    par = sp.intr_gt[0, :synth.MODEL_NPARAMS[m]]
    rig = ([m], [par], np.zeros((1, 6)))
    for f in range(3):
        a, b = int(sp.obs_offsets[f]), int(sp.obs_offsets[f + 1])
        X, uv = sp.p3d[a:b].astype(np.float64), sp.p2d[a:b].astype(np.float64)
        slot = [(0, X, uv)]
        p0 = sp.poses0[f]
        # compose() with the identity goes through a rotation matrix and back: the rounding of that round trip, nothing else
        np.testing.assert_allclose(rig_refine_ref.residuals(rig, slot, p0), refine_ref.residuals(m, par, X, uv, p0), rtol=0, atol=1e-10)
        assert abs(rig_refine_ref.cost(rig, slot, p0, 1.0) / refine_ref.cost(m, par, X, uv, p0, 1.0) - 1) < 1e-12
        assert abs(rig_refine_ref.objective(rig, slot, p0, 1.0) / refine_ref.objective(m, par, X, uv, p0, 1.0) - 1) < 1e-12
        pose, c = rig_refine_ref.refine(rig, slot, p0, 1.0)
        pose1, c1 = refine_ref.refine(m, par, X, uv, p0, 1.0)
        # both run to a stalled step at the same minimum: the resolution the yardstick has on such frames (1.35e-9, KB4)
        assert cases.dR(pose, pose1) < 1e-7 and np.abs(pose[3:] - pose1[3:]).max() < 1e-7
        assert abs(c / c1 - 1) < 1e-8


@pytest.mark.parametrize("name", ["A", "B"])
def test_gradient_vanishes_at_the_exact_pose_of_exact_data(name):
    rig, slots, start, gt = cases.exact(name)
    for s in (0, 2, 6):              # rig B: slots with 2, 3 and 1 segments
        assert rig_refine_ref.cost(rig, slots[s], gt[s], 1.0) < 1e-18
        g = np.linalg.norm(rig_refine_ref.gradient(rig, slots[s], gt[s], 1.0))
        g0 = np.linalg.norm(rig_refine_ref.gradient(rig, slots[s], start[s], 1.0))
        # residuals of ~1e-13 px at the truth: the difference quotient of their squares is rounding
        assert g0 > 1e3 and g < 1e-9 * g0, (g, g0)
        pose, c = rig_refine_ref.refine(rig, slots[s], start[s], 1.0)
        assert c < 1e-18 and cases.dR(pose, gt[s]) < 1e-10 and np.abs(pose[3:] - gt[s, 3:]).max() < 1e-10


def test_refine_rig_poses_unusable_frames_never_reach_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(api, "_ctx", boom)
    cams = [api.GenericModel("eucm", synth.GT_PARAMS[synth.MODEL_NAMES["eucm"]], 512, 512),
            api.GenericModel("kb4", synth.GT_PARAMS[synth.MODEL_NAMES["kb4"]], 512, 512)]
    eye = api.RvecTvec((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    pose = api.RvecTvec((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    ok = api.FrameFeature(0, (512, 512), {k: api.FeaturePoint((10.0 * k, 5.0), (0.1 * k, 0.01 * k * k, 0.0)) for k in range(6)})
    assert api.refine_rig_poses([[], []], cams, [eye, eye], {}) == {}
    assert api.refine_rig_poses([[None, None], [None, None]], cams, [eye, eye], {0: pose, 1: pose}) == {}
    # a frame that a camera saw but that has no starting pose in the map is left out
    assert api.refine_rig_poses([[ok, None], [None, None]], cams, [eye, eye], {1: pose}) == {}
    with pytest.raises(ValueError):
        api.refine_rig_poses([[ok]], cams, [eye, eye], {0: pose})


def test_recorded_yardstick_figures_and_convergence_on_every_noisy_slot():
    """The figures recorded in rig_refine_cases.py are what rig_refine_cases.measure() gives, to the digits recorded; on each of
    the 24 noisy slots the yardstick's runs from the start and from the ground truth end in the same minimum and its gradient
    there is rounding beside the one at the start (far below the 4e-3 that the results lie from the ground truth)."""
    m = cases.measure()
    for name in ("A", "B"):
        assert m["exact_r"][name] == pytest.approx(cases.YARD_EXACT_R[name], rel=1e-3), (name, m)
        assert m["exact_t"][name] == pytest.approx(cases.YARD_EXACT_T[name], rel=1e-3), (name, m)
    assert m["noisy_r"] == pytest.approx(cases.YARD_NOISY_R, rel=1e-3) and m["noisy_t"] == pytest.approx(cases.YARD_NOISY_T, rel=1e-3), m
    assert m["grad"] == pytest.approx(cases.YARD_GRAD_REL, rel=1e-3), m
    assert len(m["slot_diff"]) == 24 and max(m["slot_diff"]) < 1e-8 and max(m["slot_grad"]) < 1e-7, m


def test_default_start_goes_through_every_cameras_own_extrinsic(monkeypatch):
    """Without board_rtvecs the start of a frame is T_c_0^-1 o T_c_b of the first camera with an init_frame_poses result - for
    camera 0 too when its T_0_0 is not the identity."""
    cams = [api.GenericModel("eucm", synth.GT_PARAMS[synth.MODEL_NAMES["eucm"]], 512, 512),
            api.GenericModel("kb4", synth.GT_PARAMS[synth.MODEL_NAMES["kb4"]], 512, 512)]
    t = [api.RvecTvec((0.2, -0.1, 0.3), (0.05, 0.02, -0.01)), api.RvecTvec((-0.3, 0.25, 0.1), (0.1, 0.0, 0.03))]
    ok = api.FrameFeature(0, (512, 512), {k: api.FeaturePoint((10.0 * k, 5.0), (0.1 * k, 0.01 * k * k, 0.0)) for k in range(6)})
    cam_pose = [{0: api.RvecTvec((0.1, 0.2, -0.1), (0.0, 0.1, 1.0))}, {0: api.RvecTvec((0.3, 0.0, 0.1), (0.1, 0.0, 0.9)),
                                                                      1: api.RvecTvec((0.0, -0.2, 0.1), (0.0, 0.1, 1.1))}]
    frames = [[ok, None], [ok, ok]]
    monkeypatch.setattr(api, "init_frame_poses", lambda fr, model, ctx=None: cam_pose[0 if fr is frames[0] else 1])
    got = {}

    class Fake:
        def refine_rig_poses_batch(self, models, params, extr, slots, poses0, *a, **k):
            got["poses0"] = np.array(poses0); got["cams"] = [[c for c, _, _ in s] for s in slots]
            n = len(slots)
            return poses0, np.zeros(n, dtype=np.int32), None, None, None, None
    monkeypatch.setattr(api, "_ctx", lambda ctx: Fake())
    out = api.refine_rig_poses(frames, cams, t)
    assert sorted(out) == [0, 1] and got["cams"] == [[0, 1], [1]]
    for fi, c in ((0, 0), (1, 1)):
        back = t[c].compose(api.RvecTvec.from6(got["poses0"][fi]))       # T_c_0 o start = that camera's own pose
        np.testing.assert_allclose(back.as6(), cam_pose[c][fi].as6(), rtol=0, atol=1e-14)


def test_rig_refine_kernel_needs_no_scratch(tmp_path):
    """The compiler's resource remark for gfx950: ScratchSize 0 for k_rig_pose_refine (one instantiation, four model bodies, 462
    of the 512 registers of a lane live)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camera_intrinsic_calibration_rs_amd", "csrc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "ccal_kernels_rig_refine.hip"),
                        "-o", str(tmp_path / "rig_refine.out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_rig_pose_refine\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 1 and len(scratch) == 1, (names, scratch)
    assert scratch == [0], list(zip(names, scratch))
