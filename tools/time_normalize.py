#!/usr/bin/env python3
"""Developer tool: time local contrast normalisation (ccal_kernels_normalize.hip) on the session-sized workload of tools/time_photo.py -
--frames (600) frames of 752 x 480, the 7 x 5 board through the UCM camera, rendered with vignetting 2 and noise into a device-resident
u8 block:
  normalize r 8 / 16 / 32   Context.normalize_dev from that block to a second u8 block
  photo r 16                Context.photo_apply_dev between the same two blocks at blur radius 16 (blur_sigma 16/3), vignetting 0.5, no
                            noise: the kernel of the same tile and halo that does an f64 multiply-add per tap where this one adds
                            integers - normalize r 16 must not cost more
  detect                    Context.detect_checkerboards_dev on the block normalised at r 16: what the pass is a share of
The host clock (time.perf_counter) around one call followed by Context.sync, after --warmup untimed rounds; the variants alternate within
a round, all --reps rounds are listed, in ms.  The pass moves 2 bytes per pixel (u8 in, u8 out).
The kernels' own times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_normalize.py --reps 1 --warmup 1
Prints one JSON line per variant, then one with the ratios of the fastest runs."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import render_ref as rr
from camera_intrinsic_calibration_rs_amd import _ffi, api, engine, synth
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--frames", type=int, default=600)
args = ap.parse_args()

W, H, SS, N = 752, 480, 4, args.frames
ctx = Context(0)
model = synth.MODEL_NAMES["ucm"]
p = np.asarray(synth.GT_PARAMS[model], dtype=np.float64).copy()
p[2], p[3] = (W - 1) / 2.0, (H - 1) / 2.0
poses = np.stack([rr.pose6(*rr.detect_ref.board_pose(7, 5, 0.03, 360.0 * k / N, 35.0 * ((k * 7) % N) / N, 13.0 * k,
                                                     (0.03 * np.cos(0.1 * k), 0.02 * np.sin(0.13 * k), 0.18))) for k in range(N)])
tg = engine.checkerboard_target(7, 5, 0.03)
frames = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
out = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ctx.render_targets_dev(frames.data_ptr(), model, p, _ffi.PIX_U8, W, H, poses, tg, SS,
                       photo=api.PhotoOpts(blur_sigma=1.2, vignette=2.0, noise_read=2.0, noise_shot=0.05, seed=1))
ctx.sync()

U8 = _ffi.PIX_U8
blur16 = api.PhotoOpts(blur_sigma=16.0 / 3.0, vignette=0.5)
variants = [(f"normalize r {r}", lambda r=r: ctx.normalize_dev(frames.data_ptr(), out.data_ptr(), U8, U8, W, H, N, api.NormalizeOpts(radius=r)))
            for r in (8, 16, 32)]
variants.append(("photo r 16", lambda: ctx.photo_apply_dev(frames.data_ptr(), out.data_ptr(), U8, U8, W, H, N, blur16)))
# the detection call last in a round, on the block normalised at r 16
variants.append(("normalize r 16 for detect", variants[1][1]))
variants.append(("detect", lambda: ctx.detect_checkerboards_dev(out.data_ptr(), U8, W, H, N, 7, 5)))

runs = {name: [] for name, _ in variants}
found = 0
for rep in range(args.warmup + args.reps):
    for name, fn in variants:
        t0 = time.perf_counter(); res = fn(); ctx.sync(); dt = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            runs[name].append(dt)
        if name == "detect":
            found = sum(1 for r in res if r[0])
for name, _ in variants:
    if name.endswith("for detect"):
        continue
    rec = {"variant": name, "size": [W, H], "frames": N, "runs_ms": [round(t, 3) for t in runs[name]]}
    if name.startswith("normalize"):
        rec.update(bytes=2 * N * W * H, gbytes_per_s_best=round(2 * N * W * H / (min(runs[name]) * 1e-3) / 1e9, 1))
    if name == "detect":
        rec.update(boards_found=found)
    print(json.dumps(rec), flush=True)
best = {name: min(t) for name, t in runs.items()}
print(json.dumps({"normalize_r16_over_photo_r16": round(best["normalize r 16"] / best["photo r 16"], 3),
                  "normalize_r16_share_of_detect": round(best["normalize r 16"] / best["detect"], 3)}), flush=True)
