#!/usr/bin/env python3
"""Developer tool: time the photometric stage (ccal_kernels_photo.hip) on the session-sized workload of tools/time_render.py - --frames
(600) frames of 752 x 480, the 7 x 5 board through the UCM camera at 4 x 4 supersampling, device-resident u8 frames:
  ideal         Context.render_targets_dev, the call without the stage
  render+photo  Context.render_targets_dev(photo=...): the u16 ideal render chunk by chunk and the stage, one call
  photo alone   Context.photo_apply_dev from a block of u16 ideal frames rendered beforehand to the u8 block
each of the last two at r = 0 (no blur), r = 4 (blur_sigma 1.2) and r = 16 (blur_sigma 16/3), with vignetting 0.5, read noise 2 and
shot noise 0.05; and the photo pass alone without noise.  The host clock (time.perf_counter) around one call followed by Context.sync,
after --warmup untimed rounds; the variants alternate within a round, all --reps rounds are listed, in ms.  The pass moves 3 bytes per
pixel (u16 in, u8 out) and does 2 (2 r + 1) f64 multiply-adds per pixel, more by (16 + 2 r) / 16 in the horizontal pass for the halo
rows; both figures are printed with the rates of the fastest run.
The kernels' own times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_photo.py --reps 1 --warmup 1
Prints one JSON line per variant."""
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
out = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
ideal = torch.zeros((N, H, W), dtype=torch.int16, device="cuda")         # the u16 ideal frames, as bytes
torch.cuda.synchronize()
ctx.render_targets_dev(ideal.data_ptr(), model, p, _ffi.PIX_U16, W, H, poses, tg, SS)
ctx.sync()


def photo(sigma, noise=True):
    return api.PhotoOpts(blur_sigma=sigma, vignette=0.5, noise_read=2.0 if noise else 0.0, noise_shot=0.05 if noise else 0.0, seed=1)


variants = [("ideal render", None, lambda: ctx.render_targets_dev(out.data_ptr(), model, p, _ffi.PIX_U8, W, H, poses, tg, SS))]
for label, ph in (("r 0", photo(0.0)), ("r 4", photo(1.2)), ("r 16", photo(16.0 / 3.0)), ("r 4 no noise", photo(1.2, False))):
    if "no noise" not in label:
        variants.append((f"render+photo {label}", ph,
                         lambda ph=ph: ctx.render_targets_dev(out.data_ptr(), model, p, _ffi.PIX_U8, W, H, poses, tg, SS, photo=ph)))
    variants.append((f"photo alone {label}", ph,
                     lambda ph=ph: ctx.photo_apply_dev(ideal.data_ptr(), out.data_ptr(), _ffi.PIX_U16, _ffi.PIX_U8, W, H, N, ph)))

runs = {name: [] for name, _, _ in variants}
for rep in range(args.warmup + args.reps):
    for name, _, fn in variants:
        t0 = time.perf_counter(); fn(); ctx.sync(); dt = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            runs[name].append(dt)
for name, ph, _ in variants:
    rec = {"variant": name, "size": [W, H], "frames": N, "runs_ms": [round(t, 3) for t in runs[name]]}
    if name.startswith("photo alone"):
        r = engine.photo_tables(ph)[0]
        best = min(runs[name]) * 1e-3
        fma = N * W * H * (2 * r + 1) * (1.0 + (16 + 2 * r) / 16.0) if r else 0.0
        rec.update(radius=r, bytes=3 * N * W * H, gbytes_per_s_best=round(3 * N * W * H / best / 1e9, 1), f64_multiply_adds=int(fma),
                   gfma_per_s_best=round(fma / best / 1e9, 1))
    print(json.dumps(rec), flush=True)
