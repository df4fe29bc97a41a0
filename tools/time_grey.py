#!/usr/bin/env python3
"""Developer tool: time the grey stage (ccal_kernels_grey.hip) on the session-sized workload of tools/time_normalize.py - --frames (600)
frames of 752 x 480, random samples, in a device-resident block - for GREY, RGB, RGBA and the RGGB mosaic at u8 and u16 sources
(the destination has the source's type) and bins 1, 2 and 4.  600 such frames are 217 MB (GREY u8) to 1.7 GB (RGBA u16): all but the
smallest exceed the 256 MiB Infinity Cache, the stage streams from HBM.

The yardstick is a plain device-to-device copy (hipMemcpyAsync through torch's Tensor.copy_) in the same run, not this kernel in
another configuration: the stage reads the source block and writes the destination block, so per case three copies are timed -
  copy src    the source block's bytes copied (reads and writes that many)
  copy dst    the destination block's bytes copied
  copy same   (source + destination) / 2 bytes copied: the copy that moves exactly the stage's traffic, the figure to compare with.
Times are device events around one call on one stream (the context is created on torch's), after --warmup untimed rounds that also ramp the clocks; the stage and its copies
alternate within a round; the median of --reps rounds is reported with all rounds listed, in ms.  GB/s is (source + destination
bytes) over the median.  The kernels' own times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_grey.py --reps 1 --warmup 1
Prints one JSON line per case."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from camera_intrinsic_calibration_rs_amd import _ffi, api, engine
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--frames", type=int, default=600)
ap.add_argument("--layouts", default="grey,rgb,rgba,bayer_rggb")
args = ap.parse_args()

W, H, N = 752, 480, args.frames
CHANNELS = {"grey": 1, "rgb": 3, "rgba": 4, "bayer_rggb": 1}
stream = torch.cuda.Stream()                                           # the context enqueues on torch's stream: one pair of events brackets either
torch.cuda.set_stream(stream)
ctx = Context(0, stream=stream.cuda_stream)


def timed(fn):
    """ms of fn() between two device events on the one stream."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record(stream)
    fn()
    t1.record(stream)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


for layout in args.layouts.split(","):
    for es, code in ((1, _ffi.PIX_U8), (2, _ffi.PIX_U16)):
        src_bytes = N * H * W * CHANNELS[layout] * es
        src = torch.randint(0, 256, (src_bytes,), dtype=torch.uint8, device="cuda")
        spare = torch.empty_like(src)                                  # the copies' destination
        for b in (1, 2, 4):
            Wo, Ho = engine.grey_out_size(W, H, b)
            dst_bytes = N * Ho * Wo * es
            dst = torch.zeros((dst_bytes,), dtype=torch.uint8, device="cuda")
            same = ((src_bytes + dst_bytes) // 2 + 15) & ~15
            variants = [
                ("grey", lambda: ctx.grey_dev(src.data_ptr(), dst.data_ptr(), api.LAYOUTS[layout], code, code, W, H, N, api.GreyOpts(bin=b))),
                ("copy src", lambda: spare.copy_(src)),
                ("copy dst", lambda: spare[:dst_bytes].copy_(src[:dst_bytes])),
                ("copy same", lambda: spare[:same].copy_(src[:same])),
            ]
            runs = {name: [] for name, _ in variants}
            for rep in range(args.warmup + args.reps):
                for name, fn in variants:
                    dt = timed(fn)
                    if rep >= args.warmup:
                        runs[name].append(dt)
            med = {name: statistics.median(t) for name, t in runs.items()}
            print(json.dumps({"layout": layout, "dtype": "u8" if es == 1 else "u16", "bin": b, "size": [W, H], "frames": N,
                              "src_bytes": src_bytes, "dst_bytes": dst_bytes,
                              "grey_ms": round(med["grey"], 3), "grey_gbytes_per_s": round((src_bytes + dst_bytes) / (med["grey"] * 1e-3) / 1e9, 1),
                              "copy_src_ms": round(med["copy src"], 3), "copy_dst_ms": round(med["copy dst"], 3),
                              "copy_same_traffic_ms": round(med["copy same"], 3),
                              "grey_over_copy_same_traffic": round(med["grey"] / med["copy same"], 2),
                              "grey_runs_ms": [round(t, 3) for t in runs["grey"]],
                              "copy_same_runs_ms": [round(t, 3) for t in runs["copy same"]]}), flush=True)
            del dst
        del src, spare
        torch.cuda.empty_cache()
