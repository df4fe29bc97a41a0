#!/usr/bin/env python3
"""Developer tool: time the target renderer (Context.render_targets_dev, ccal_kernels_render.hip) on two session-sized workloads,
for each of the four models and both targets, at 4 x 4 supersampling into a device-resident u8 block:
  wide    --frames (600) frames of 752 x 480: the model's GT parameters (synth.GT_PARAMS) with the principal point moved to the
          middle of the wider image
  square  --frames (600) frames of 512 x 512: the GT parameters as they are
The target is the 7 x 5 board of 30 mm squares or a 6 x 6 AprilGrid of 30 mm tags, turning and tilting in front of the camera over
the frames.  Per (workload, model, target): the host clock (time.perf_counter) around one render_targets_dev call followed by
Context.sync, after --warmup untimed calls; all --reps runs are listed, in ms, with the sub-pixel rays per second of the fastest.
The baseline is the yardstick, not the code under test: tests/render_ref.py renders ONE frame of each kind on the CPU (--baseline;
near=False, so it does a fifth of the work the parity tests ask of it).
The kernel's own time comes from a trace run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_render.py --reps 1 --warmup 0
Prints one JSON line per measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import render_ref as rr
from camera_intrinsic_calibration_rs_amd import _ffi, engine, synth
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--frames", type=int, default=600)
ap.add_argument("--workloads", default="wide,square")
ap.add_argument("--models", default="ucm,eucm,kb4,opencv5")
ap.add_argument("--targets", default="board,grid")
ap.add_argument("--baseline", action="store_true", help="also render one frame of each kind with the numpy yardstick")
args = ap.parse_args()

SIZES = {"wide": (752, 480), "square": (512, 512)}
SS = 4
BIG_GRID = rr.tag_ref.Board(0.03, 0.3, 6, 6)
ctx = Context(0)


def params_for(model, w, h):
    p = np.asarray(synth.GT_PARAMS[model], dtype=np.float64).copy()
    if (w, h) != (512, 512):
        p[2], p[3] = (w - 1) / 2.0, (h - 1) / 2.0
    return p


def poses_for(model, target, n):
    z = (0.40 if target == "board" else 0.45) if model == rr.OPENCV5 else (0.18 if target == "board" else 0.22)
    out = []
    for k in range(n):
        rot, tilt, axis = 360.0 * k / n, 35.0 * ((k * 7) % n) / n, 13.0 * k
        centre = (0.03 * np.cos(0.1 * k), 0.02 * np.sin(0.13 * k), z)
        if target == "board":
            out.append(rr.pose6(*rr.detect_ref.board_pose(7, 5, 0.03, rot, tilt, axis, centre)))
        else:
            out.append(rr.pose6(*rr.tag_ref.grid_pose(BIG_GRID, rot, tilt, axis, centre)))
    return np.stack(out)


def target_for(target):
    if target == "board":
        return engine.checkerboard_target(7, 5, 0.03)
    fam = rr.family()
    return engine.aprilgrid_target(0.03, 0.3, 6, 6, 0, fam.bits, fam.codes, 1)


for wl in args.workloads.split(","):
    w, h = SIZES[wl]
    block = torch.zeros((args.frames, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for name in args.models.split(","):
        model = synth.MODEL_NAMES[name]
        p = params_for(model, w, h)
        for target in args.targets.split(","):
            poses, tg = poses_for(model, target, args.frames), target_for(target)

            def call():
                ctx.render_targets_dev(block.data_ptr(), model, p, _ffi.PIX_U8, w, h, poses, tg, SS)
                ctx.sync()

            for _ in range(args.warmup):
                call()
            runs = []
            for _ in range(args.reps):
                t0 = time.perf_counter(); call(); runs.append((time.perf_counter() - t0) * 1e3)
            rays = args.frames * w * h * SS * SS
            rec = {"workload": wl, "size": [w, h], "frames": args.frames, "model": name, "target": target, "supersample": SS,
                   "runs_ms": [round(t, 3) for t in runs], "rays": rays, "rays_per_s_best": round(rays / (min(runs) * 1e-3), 1),
                   "covered": round(float((block[:: max(args.frames // 16, 1)] > 0).float().mean().item()), 3)}
            if args.baseline:
                from oracle import binding
                binding.load()
                ytarget = rr.board_target(7, 5, 0.03) if target == "board" else rr.grid_target(BIG_GRID, rr.family())
                t0 = time.perf_counter()
                img = rr.render(binding, model, p, w, h, poses[0], ytarget, ss=SS, near=False)[0]
                rec["yardstick_one_frame_s"] = round(time.perf_counter() - t0, 3)
                rec["first_frame_pixels_that_differ"] = int((block[0].cpu().numpy() != img).sum())
            print(json.dumps(rec), flush=True)
