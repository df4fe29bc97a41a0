#!/usr/bin/env python3
"""Developer tool: time the sub-pixel corner refinement at a session's size - 600 frames of 512 x 512 u8, a 12 x 12 grid of rendered
saddles (tests/corner_ref.py) in each, one start per saddle up to 1.5 px off, half_win 5, eps 1e-3.  Host clock around whole calls,
each of which ends in a synchronise: ccal_refine_corners_dev (images resident on the device; corners up, results down) and
ccal_refine_corners_batch (the image block uploaded as well).  Medians over --reps calls after --warmup untimed ones.  The kernel's
own time comes from a kernel trace of this tool in a run of its own.  Prints one JSON line."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import corner_ref as ref
from camera_intrinsic_calibration_rs_amd import _ffi
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=600)
ap.add_argument("--half-win", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

img, centres, starts = ref.grid_fixture(500, n_side=12, first=36, spacing=40, radius=16)        # 512 x 512, 144 saddles
assert img.shape == (512, 512)
N, h = args.frames, args.half_win
frames = np.ascontiguousarray(np.broadcast_to(img, (N, 512, 512)))
xy = [starts] * N
ctx = Context(0)
dev = torch.from_numpy(frames.reshape(-1)).cuda()
torch.cuda.synchronize()


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


out = {"frames": N, "corners_per_frame": len(starts), "size": 512, "half_win": h, "reps": args.reps}
res = ctx.refine_corners_dev(dev.data_ptr(), _ffi.PIX_U8, 512, 512, N, xy, h, 30, 1e-3)
out["ok_fraction"] = float(np.mean(np.concatenate(res[1]) == _ffi.OK))
out["iterations_mean"] = float(np.mean(np.concatenate(res[2])))
out["worst_error_px"] = float(np.hypot(*(res[0][0] - centres).T).max())
out["dev_call_ms"] = median_ms(lambda: ctx.refine_corners_dev(dev.data_ptr(), _ffi.PIX_U8, 512, 512, N, xy, h, 30, 1e-3))
out["host_call_ms"] = median_ms(lambda: ctx.refine_corners_batch(frames, xy, h, 30, 1e-3))
ctx.close()
print(json.dumps(out))
