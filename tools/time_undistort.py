#!/usr/bin/env python3
"""Developer tool: time the undistortion path - one 512 x 512 map per model, and the remap of 256 frames of 512 x 512 u8 / u16 through a
device-resident map (ccal_remap_dev, device to device) - with torch.nn.functional.grid_sample (bilinear, align_corners=True, f32)
on the same frames beside it as an outside comparison.  Medians over --reps launches timed one by one with events, after
--warmup untimed launches (the clock ramp); "hbm_frac" = the bytes the kernel has to move (map once, every frame in and out) per
second over --hbm-gbps.  Prints one JSON line."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from camera_intrinsic_calibration_rs_amd import _ffi, api, synth
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--hbm-gbps", type=float, default=8000.0, help="the HBM rate the fractions refer to (MI355X: 8 TB/s nominal)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
ctx = Context(0, stream=stream.cuda_stream)
S, N = args.size, args.frames


def median_us(fn):
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            fn()
        stream.synchronize()
        ts = []
        for _ in range(args.reps):
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            a.record(stream); fn(); b.record(stream)
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


out = {"frames": N, "size": S, "reps": args.reps, "hbm_gbps": args.hbm_gbps}
maps = {}
for name, m in synth.MODEL_NAMES.items():
    p = np.asarray(synth.GT_PARAMS[m])
    K = api.GenericModel(name, p, S, S).estimate_new_camera_matrix_for_undistort(0.5, ctx=ctx)
    held = []

    def make():
        held.append(ctx.undistort_map(m, p, K, (S, S)))
        if len(held) > 1:
            held.pop(0).close()           # the block comes out of the context's cache again: allocation is not what is timed
    us = median_us(make)
    maps[name] = held[-1]
    out[f"map_{name}_us"] = us
    out[f"map_{name}_hbm_frac"] = (2 * 4 * S * S) / (us * 1e-6) / (args.hbm_gbps * 1e9)

umap = maps["eucm"]
xm, ym = umap.download()
rng = np.random.default_rng(0)
for tag, dtype, code in (("u8", np.uint8, _ffi.PIX_U8), ("u16", np.uint16, _ffi.PIX_U16)):
    frames = torch.from_numpy(rng.integers(0, np.iinfo(dtype).max + 1, (N, S, S), dtype=np.int64).astype(dtype).view(np.uint8).reshape(-1).copy()).to(dev)
    dst = torch.empty_like(frames)
    torch.cuda.synchronize()
    us = median_us(lambda: umap.remap_dev(frames.data_ptr(), dst.data_ptr(), code, 1, S, S, N))
    moved = 2 * 4 * S * S + 2 * frames.numel()
    out[f"remap_{tag}_us_per_frame"] = us / N
    out[f"remap_{tag}_GBps"] = moved / us / 1e3
    out[f"remap_{tag}_hbm_frac"] = moved / (us * 1e-6) / (args.hbm_gbps * 1e9)
    # the outside comparison: the same frames as f32 [N, 1, S, S] through grid_sample with the same map, normalised to [-1, 1]
    with torch.cuda.stream(stream):
        if tag == "u8":
            src32 = frames.view(N, 1, S, S).to(torch.float32)
        else:
            src32 = frames.view(torch.int16).view(N, 1, S, S).to(torch.float32)      # values do not matter for the timing
        gx = torch.from_numpy(xm).to(dev) * (2.0 / (S - 1)) - 1.0
        gy = torch.from_numpy(ym).to(dev) * (2.0 / (S - 1)) - 1.0
        grid = torch.stack([gx, gy], dim=-1)[None].expand(N, S, S, 2).contiguous()
        stream.synchronize()
    us_gs = median_us(lambda: torch.nn.functional.grid_sample(src32, grid, mode="bilinear", padding_mode="zeros", align_corners=True))
    out[f"grid_sample_f32_{tag}_us_per_frame"] = us_gs / N
    del src32, grid
for h in maps.values():
    h.close()
ctx.close()
print(json.dumps(out))
