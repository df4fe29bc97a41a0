#!/usr/bin/env python3
"""Developer tool: time the quad proposer alone on two workloads built from the rendered AprilGrid fixture of tests/tag_ref.py
(four 320 x 240 u8 frames of a 3 x 2 grid; the points are the CPU chain's - tests/quad_ref.py: fixture_points, merged):
  copies   --copies (256) copies of the four frames: 1024 images of 70 to 90 points each
  tiled    each frame tiled 4 x 4 into 1280 x 960, its points with it: 4 images of 1100 to 1500 points each
Default parameters (max_side = half the larger image side).  Each figure is the median over --reps calls timed one by one with
events on the context's stream, after --warmup untimed calls; a call includes its uploads, its two synchronises and its
downloads: ccal_propose_quads_dev (images resident on the device) and ccal_propose_quads_batch (the image block uploaded as
well).  Next to them the numpy yardstick's time for the same input on this host (quad_ref.propose; for `copies` the four distinct
frames timed once and multiplied).  The kernels' own times come from a kernel trace of this tool in a run of its own.  Prints one
JSON line."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import quad_ref as ref
import tag_ref
from camera_intrinsic_calibration_rs_amd import _ffi
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--copies", type=int, default=256)
args = ap.parse_args()

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
ctx = Context(0, stream=stream.cuda_stream)


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
    return statistics.median(ts), min(ts), max(ts)


def workload(name, images, xy_list, distinct, times):
    """distinct: the images the yardstick runs on; times: how often each of them occurs in the call."""
    n, H, W = images.shape
    max_side = max(W, H) / 2.0
    t = time.perf_counter()
    want = [ref.propose(images[k], xy_list[k], max_side=max_side) for k in distinct]
    cpu_s = (time.perf_counter() - t) * times
    block = torch.from_numpy(images.reshape(-1)).cuda()
    torch.cuda.synchronize()
    got = ctx.propose_quads_dev(block.data_ptr(), _ffi.PIX_U8, W, H, n, xy_list)
    same = all(np.array_equal(got[k][0], want[i]["idx"]) and got[k][2] == want[i]["count"] and got[k][3] == want[i]["flags"]
               for i, k in enumerate(distinct))
    out = {"images": n, "width": W, "height": H, "points": [len(xy_list[k]) for k in distinct], "quads": [want[i]["count"] for i in range(len(distinct))],
           "image_bytes": int(images.nbytes), "matches_yardstick": bool(same), "yardstick_cpu_s": cpu_s}
    out["dev_call_us"] = median_us(lambda: ctx.propose_quads_dev(block.data_ptr(), _ffi.PIX_U8, W, H, n, xy_list))
    out["host_call_us"] = median_us(lambda: ctx.propose_quads_batch(images, xy_list))
    del block
    return {name: out}


imgs, _ = tag_ref.grid_frames(np.uint8)
pts = [m for _, m in ref.fixture_points(np.uint8)]
res = {"reps": args.reps, "warmup": args.warmup}
res.update(workload("copies", np.ascontiguousarray(np.tile(imgs, (args.copies, 1, 1))), pts * args.copies, range(4), args.copies))
tiled = np.ascontiguousarray(np.tile(imgs, (1, 4, 4)))
shift = np.array([[320.0 * i, 240.0 * j] for j in range(4) for i in range(4)])
res.update(workload("tiled", tiled, [np.concatenate([p + s for s in shift]) for p in pts], range(4), 1))
ctx.close()
print(json.dumps(res))
