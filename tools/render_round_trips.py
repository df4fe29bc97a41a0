#!/usr/bin/env python3
"""Developer tool: what the two image chains do under the library's own lenses.  For each model (synth.GT_PARAMS, 512 x 512) the
target's middle is moved off the optical axis in steps of --step degrees at a fixed range (0.18 m for the 7 x 5 board of 30 mm
squares, 0.12 m for the 3 x 2 grid of 30 mm tags; 0.40 m and 0.25 m under OPENCV5), in two attitudes:
  facing    the target's normal along the line of sight (tilted by the off-axis angle)
  parallel  the target parallel to the image plane (only moved sideways: the fisheye foreshortens it)
All poses of a model are rendered in ONE render_targets_dev call per target and go through detect_checkerboards_dev /
detect_tags_dev on the device.  Per pose, one JSON line: whether every corner of the target projects into the image, whether the
chain found the whole target (all 35 corners / all six tags at Hamming distance 0), the worst corner distance from oracle.project of
the posed corner, and the smallest and largest distance between neighbouring corners (board) or tag side (grid) in pixels."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import render_ref as rr
from oracle import binding as oracle
from camera_intrinsic_calibration_rs_amd import _ffi, engine, synth
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--step", type=float, default=5.0)
ap.add_argument("--max-angle", type=float, default=85.0)
ap.add_argument("--models", default="ucm,eucm,kb4,opencv5")
args = ap.parse_args()
oracle.load()
ctx = Context(0)
S = rr.RT_SIZE
angles = np.arange(0.0, args.max_angle + 1e-9, args.step)
fam = rr.family()


def centre(angle, rng):
    a = np.deg2rad(angle)
    return (rng * np.sin(a), 0.004, rng * np.cos(a))


def inside(uv):
    return bool(np.isfinite(uv).all() and (uv >= 0).all() and (uv[..., 0] <= S - 1).all() and (uv[..., 1] <= S - 1).all())


for name in args.models.split(","):
    m = synth.MODEL_NAMES[name]
    p = rr.gt_params(m)
    for attitude in ("facing", "parallel"):
        tilt = (lambda a: a) if attitude == "facing" else (lambda a: 0.0)
        # ---- the board
        rng = 0.40 if m == rr.OPENCV5 else 0.18
        poses = np.stack([rr._board_pose(12.0, tilt(a), 90.0, centre(a, rng)) for a in angles])
        block = torch.zeros((len(poses), S, S), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.render_targets_dev(block.data_ptr(), m, p, _ffi.PIX_U8, S, S, poses, engine.checkerboard_target(*rr.BOARD))
        res = ctx.detect_checkerboards_dev(block.data_ptr(), _ffi.PIX_U8, S, S, len(poses), rr.BOARD[0], rr.BOARD[1], half_win=rr.RT_BOARD_HALF_WIN)
        for a, pose, (found, xy, _, stats) in zip(angles, poses, res):
            truth = rr.board_truth(oracle, m, p, pose)
            g = truth.reshape(rr.BOARD[1], rr.BOARD[0], 2)
            sp = np.concatenate([np.linalg.norm(np.diff(g, axis=1), axis=-1).ravel(), np.linalg.norm(np.diff(g, axis=0), axis=-1).ravel()])
            print(json.dumps({"model": name, "target": "board", "attitude": attitude, "angle": float(a), "in_image": inside(truth), "found": bool(found),
                              "worst_px": round(rr.board_error(xy, truth), 4) if found else None,
                              "spacing_px": [round(float(sp.min()), 1), round(float(sp.max()), 1)], "rows_kept": int(stats[0])}), flush=True)
        # ---- the grid
        rng = 0.25 if m == rr.OPENCV5 else 0.12
        poses = np.stack([rr._grid_pose(15.0, tilt(a), 90.0, centre(a, rng)) for a in angles])
        ctx.render_targets_dev(block.data_ptr(), m, p, _ffi.PIX_U8, S, S, poses,
                               engine.aprilgrid_target(0.03, 0.3, rr.GRID.tag_rows, rr.GRID.tag_cols, 0, fam.bits, fam.codes, 1))
        got = ctx.detect_tags_dev(block.data_ptr(), _ffi.PIX_U8, S, S, len(poses), fam.bits, fam.codes, half_win=rr.RT_GRID_HALF_WIN)
        for a, pose, (ids, rot, ham, corners, *_rest) in zip(angles, poses, got):
            truth = rr.grid_truth(oracle, m, p, pose)
            side = np.linalg.norm(truth - np.roll(truth, -1, axis=1), axis=-1)
            whole = list(ids) == list(range(6)) and not np.any(ham)
            worst = max([float(np.linalg.norm(c - truth[t], axis=1).max()) for t, c in zip(ids, corners) if 0 <= t < 6], default=None)
            print(json.dumps({"model": name, "target": "grid", "attitude": attitude, "angle": float(a), "in_image": inside(truth), "found": bool(whole),
                              "tags": [int(t) for t in ids], "worst_px": None if worst is None else round(worst, 4),
                              "side_px": [round(float(side.min()), 1), round(float(side.max()), 1)]}), flush=True)
