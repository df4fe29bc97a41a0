#!/usr/bin/env python3
"""Developer tool, an experiment and no pass criterion: render a dozen frames of the 7 x 5 board through a GT lens
(synth.GT_PARAMS, 512 x 512), detect the boards from the images alone (api.detect_checkerboard, fused), and calibrate from those
detections with api.calib_camera, starting from the GT parameters perturbed by --perturb (relative, focal lengths and distortion;
the principal point moved by 3 px).  The board's middle goes 0 to 40 degrees off the axis in twelve directions, facing the camera,
with an extra tilt.  Prints one JSON line: frames found, the fitted parameters against the GT, the worst and the RMS distance of the
detected corners from the fitted model's reprojection."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import render_ref as rr
from camera_intrinsic_calibration_rs_amd import api, synth
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="eucm")
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--perturb", type=float, default=0.05)
args = ap.parse_args()
ctx = Context(0)
m = synth.MODEL_NAMES[args.model]
gt = np.asarray(synth.GT_PARAMS[m], dtype=np.float64)
model = api.GenericModel(args.model, gt, rr.RT_SIZE, rr.RT_SIZE)
rng = 0.40 if m == rr.OPENCV5 else 0.18
poses = []
for k in range(args.frames):
    a, phi = np.deg2rad((20.0 if m == rr.OPENCV5 else 40.0) * k / max(args.frames - 1, 1)), np.deg2rad(360.0 * k / args.frames * 5.0)
    centre = (rng * np.sin(a) * np.cos(phi), rng * np.sin(a) * np.sin(phi), rng * np.cos(a))
    poses.append(rr._board_pose(30.0 * k, np.rad2deg(a) + 8.0, np.rad2deg(phi) + 90.0, centre))
images = api.render_checkerboard(model, np.stack(poses), rr.BOARD[:2], rr.BOARD[2], ctx=ctx)
frames = api.detect_checkerboard(list(images), rr.BOARD[:2], rr.BOARD[2], ctx=ctx, fused=True)
start = gt.copy()
start[:2] *= 1.0 + args.perturb
start[2:4] += 3.0
start[4:] *= 1.0 - args.perturb
res = api.calib_camera(frames, api.GenericModel(args.model, start, rr.RT_SIZE, rr.RT_SIZE), False, 0, False, ctx=ctx)
out = {"model": args.model, "frames": args.frames, "found": sum(f is not None for f in frames), "gt": gt.tolist(), "start": start.tolist()}
if res is None:
    out["fitted"] = None
else:
    fitted, rtvecs = res
    err = []
    for i, f in enumerate(frames):
        if f is None or i not in rtvecs:
            continue
        R, t = rtvecs[i].matrix()
        ids = sorted(f.features)
        X = np.array([f.features[j].p3d for j in ids]) @ R.T + t
        uv, ok = fitted.project(X, ctx)
        err.append(np.linalg.norm(uv - np.array([f.features[j].p2d for j in ids]), axis=1)[ok])
    err = np.concatenate(err)
    out.update(fitted=[round(float(x), 6) for x in fitted.params()], fitted_minus_gt=[round(float(x), 6) for x in fitted.params() - gt],
               reprojection_rms_px=round(float(np.sqrt((err ** 2).mean())), 4), reprojection_worst_px=round(float(err.max()), 4))
print(json.dumps(out))
