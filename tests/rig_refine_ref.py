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
import numpy as np

from camera_intrinsic_calibration_rs_amd import synth

import refine_ref
from refine_ref import _H, _stencil, weights


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
    r = residuals(rig, slot, pose)
    s = (r * r).sum(axis=-1)
    c = (weights(s, delta) * s).sum(axis=-1)
    return float(c) if c.ndim == 0 else c


def objective(rig, slot, pose, delta):
    """sum rho(s) over every camera of the slot: the function whose stationary point the corrected Gauss-Newton iteration finds."""
    r = residuals(rig, slot, pose)
    s = (r * r).sum(axis=-1)
    if delta > 0.0:
        s = np.where(s > delta * delta, 2.0 * delta * np.sqrt(s) - delta * delta, s)
    c = s.sum(axis=-1)
    return float(c) if c.ndim == 0 else c


def gradient(rig, slot, pose, delta, h=_H):
    """Central-difference gradient of objective() with respect to rvec | tvec of T_0_b."""
    c = objective(rig, slot, _stencil(pose, h), delta)
    return (c[:6] - c[6:]) / (2 * h)


def _corrected_system(rig, slot, pose, delta, h=_H):
    """(J, c): central-difference Jacobian of r and r itself, rows scaled by sqrt(rho')."""
    r = residuals(rig, slot, pose)
    sw = np.sqrt(weights((r * r).sum(axis=-1), delta))
    rs = residuals(rig, slot, _stencil(pose, h))
    J = (rs[:6] - rs[6:]) / (2 * h)                                   # [6, n, 2]
    return (J * sw[None, :, None]).reshape(6, -1).T, (r * sw[:, None]).ravel()


def refine(rig, slot, pose0, delta, max_iter=300):
    """LM from pose0 until the step stalls (the rounding of the objective): (pose, cost() there)."""
    x = np.asarray(pose0, dtype=np.float64).copy()
    F = objective(rig, slot, x, delta)
    lam = 1e-4
    for _ in range(max_iter):
        J, c = _corrected_system(rig, slot, x, delta)
        H = J.T @ J
        g = J.T @ c
        moved = False
        while lam < 1e12:
            d = -np.linalg.solve(H + lam * np.diag(np.maximum(np.diag(H), 1e-12)), g)
            Fn = objective(rig, slot, x + d, delta)
            if Fn < F:
                x = x + d; F = Fn; lam = max(lam * 0.1, 1e-15); moved = True
                break
            if np.abs(d).max() < 1e-15:
                break
            lam *= 10.0
        if not moved or np.abs(d).max() < 1e-14:
            break
    return x, cost(rig, slot, x, delta)


def solve(rig, slot, pose_start, pose_gt, delta):
    """The yardstick's answer for one slot: of the runs from pose_start and from pose_gt the one with the lower objective."""
    a = refine(rig, slot, pose_start, delta)
    b = refine(rig, slot, pose_gt, delta)
    return a if objective(rig, slot, a[0], delta) <= objective(rig, slot, b[0], delta) else b
