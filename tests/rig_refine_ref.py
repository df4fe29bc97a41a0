"""numpy f64 yardstick for the board poses of a rig under fixed intrinsics and extrinsics (ccal_refine_rig_poses_batch,
csrc/ccal_kernels_rig_refine.hip), written independently of the kernel, in the style of tests/refine_ref.py, whose residuals()
and weights() it uses as they are.

A rig is (models [n_cams], params: one parameter vector per camera, extr [n_cams, 6]: rvec | tvec of T_c_0); a slot is a list of
segments (cam, X [n, 3], uv [n, 2]).  The residuals of a slot at the pose T_0_b are the concatenation over its segments of
    refine_ref.residuals(model_c, params_c, X, uv, compose(extr_c, pose)),      compose(e, p) = T_c_0 o T_0_b,
and cost(), objective(), gradient(), refine() and solve() are those of refine_ref.py over that concatenation: the reported
sum rho'(s) s, the judged sum rho(s), its central-difference gradient with respect to rvec | tvec of T_0_b (no analytic derivative
anywhere, the kernel's Jacobian has no part in it), Levenberg-Marquardt on the corrected system until the step stalls, and the
better of the runs from the given start and from the ground truth.
"""
from functools import partial

import numpy as np

from camera_intrinsic_calibration_rs_amd import synth

import refine_ref
from refine_ref import _H, _stencil           # (_stencil: tests reach it through this module too)


def compose(extr, pose):
    """T_c_0 o T_0_b as rvec | tvec; pose [6] or [k, 6]."""
    extr = np.asarray(extr, dtype=np.float64); pose = np.asarray(pose, dtype=np.float64)
    R1 = synth.rodrigues(extr[:3])
    R = R1 @ synth.rodrigues(pose[..., :3])
    t = pose[..., 3:] @ R1.T + extr[3:]
    return np.concatenate([synth.rotmat_to_rvec(R), t], axis=-1)


def residuals(rig, slot, pose):
    """pose [6] -> r [n, 2]; poses [k, 6] -> r [k, n, 2]; n = all the slot's points, segment after segment."""
    models, params, extr = rig
    pose = np.asarray(pose, dtype=np.float64)
    parts = [refine_ref.residuals(int(models[c]), params[c], X, uv, compose(extr[c], pose)) for c, X, uv in slot]
    if not parts:
        return np.zeros(pose.shape[:-1] + (0, 2))
    return np.concatenate(parts, axis=-2)


def pixel_errors(rig, slot, pose):
    r = residuals(rig, slot, pose)
    return np.sqrt((r * r).sum(axis=-1))


def cost(rig, slot, pose, delta):
    return refine_ref.cost_of(partial(residuals, rig, slot), pose, delta)


def objective(rig, slot, pose, delta):
    """sum rho(s) over every camera of the slot."""
    return refine_ref.objective_of(partial(residuals, rig, slot), pose, delta)


def gradient(rig, slot, pose, delta, h=_H):
    """Central-difference gradient of objective() with respect to rvec | tvec of T_0_b."""
    return refine_ref.gradient_of(partial(residuals, rig, slot), pose, delta, h)


def _corrected_system(rig, slot, pose, delta, h=_H):
    return refine_ref.corrected_system_of(partial(residuals, rig, slot), pose, delta, h)


def refine(rig, slot, pose0, delta, max_iter=300):
    """LM from pose0 until the step stalls: (pose, cost() there)."""
    return refine_ref.refine_of(partial(residuals, rig, slot), pose0, delta, max_iter)


def solve(rig, slot, pose_start, pose_gt, delta):
    """The yardstick's answer for one slot: of the runs from pose_start and from pose_gt the one with the lower objective."""
    return refine_ref.solve_of(partial(residuals, rig, slot), pose_start, pose_gt, delta)
