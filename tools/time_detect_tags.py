#!/usr/bin/env python3
"""Developer tool: time the whole front end - images to AprilGrid detections - staged against fused, on two workloads built with
the renderer of tests/tag_ref.py:
  copies   --copies (256) copies of the four 320 x 240 u8 fixture frames (a 3 x 2 grid): 1024 images
  large    --large (600) frames of 752 x 480 u8 showing a 6 x 6 grid of the same tags (45 px wide) in the fixture's four poses
Per workload, each figure the median (min - max) over --reps calls timed one by one with events on the context's stream after
--warmup untimed calls; a call includes everything it does on the host:
  staged        api.detect_aprilgrid(..., fused=False): four stage calls, the links in Python - the image block goes up four times
  fused         api.detect_aprilgrid(..., fused=True): ccal_detect_tags_batch + frames_from_tags - the image block goes up once
  tags_batch    Context.detect_tags_batch alone (the C call and its unpacking)
  tags_dev      Context.detect_tags_dev alone, the image block resident on the device - nothing of it goes up
and the bytes of pixels each of them uploads.  --only fused restricts the run to tags_dev (for a kernel trace of its own:
rocprofv3 --kernel-trace --stats -- python tools/time_detect_tags.py --only fused --reps 3 --warmup 1).  Prints one JSON line."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import detect_ref
import tag_ref
from camera_intrinsic_calibration_rs_amd import _ffi, api
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--large", type=int, default=600)
ap.add_argument("--workloads", default="copies,large")
ap.add_argument("--only", default="all", choices=["all", "fused"])
args = ap.parse_args()

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
ctx = Context(0, stream=stream.cuda_stream)
family = api.TagFamily("toy", 36, tag_ref.grid_family().codes)


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
    print(f"  {statistics.median(ts):.0f} us", file=sys.stderr, flush=True)       # progress: a workload takes minutes
    return statistics.median(ts), min(ts), max(ts)


def workload(name, images, board):
    n, H, W = images.shape
    frames = list(images)
    out = {"images": n, "width": W, "height": H, "image_bytes": int(images.nbytes)}
    block = torch.from_numpy(images.reshape(-1)).cuda()
    torch.cuda.synchronize()
    tags = ctx.detect_tags_dev(block.data_ptr(), _ffi.PIX_U8, W, H, n, family.bits, family.codes)
    out["stats_first"] = tags[0][7].tolist()
    out["tags_per_image"] = sorted({t[5] for t in tags})
    out["flags"] = sorted({t[6] for t in tags})
    if args.only == "all":
        t = time.perf_counter()
        staged = api.detect_aprilgrid(frames, family, board, ctx=ctx)
        out["staged_first_call_s"] = time.perf_counter() - t
        out["fused_equals_staged"] = bool(api.detect_aprilgrid(frames, family, board, ctx=ctx, fused=True) == staged)
        out["frames_detected"] = sum(f is not None for f in staged)
        out["staged_us"] = median_us(lambda: api.detect_aprilgrid(frames, family, board, ctx=ctx))
        out["fused_us"] = median_us(lambda: api.detect_aprilgrid(frames, family, board, ctx=ctx, fused=True))
        out["tags_batch_us"] = median_us(lambda: ctx.detect_tags_batch(images, family.bits, family.codes))
        out["pixel_bytes_uploaded"] = {"staged": 4 * int(images.nbytes), "fused": int(images.nbytes), "tags_batch": int(images.nbytes), "tags_dev": 0}
    out["tags_dev_us"] = median_us(lambda: ctx.detect_tags_dev(block.data_ptr(), _ffi.PIX_U8, W, H, n, family.bits, family.codes))
    del block
    return {name: out}


res = {"reps": args.reps, "warmup": args.warmup}
todo = args.workloads.split(",")
if "copies" in todo:
    imgs, _ = tag_ref.grid_frames(np.uint8)
    board = api.AprilGridBoard(tag_ref.GRID.tag_size_meter, tag_ref.GRID.tag_spacing, tag_ref.GRID.tag_rows, tag_ref.GRID.tag_cols)
    res.update(workload("copies", np.ascontiguousarray(np.tile(imgs, (args.copies, 1, 1))), board))
if "large" in todo:
    W, H = 752, 480
    grid = tag_ref.Board(tag_ref.GRID.tag_size_meter, tag_ref.GRID.tag_spacing, 6, 6)
    t = time.perf_counter()
    poses = []
    for lam, rot, tilt, axis in tag_ref.GRID_FRAMES:
        cam = detect_ref.Camera(tag_ref.GRID_F, (W - 1) / 2.0, (H - 1) / 2.0, lam)
        R, tt = tag_ref.grid_pose(grid, rot, tilt, axis, (0.002, -0.003, 0.40))
        poses.append(tag_ref.render_aprilgrid(W, H, cam, R, tt, grid, tag_ref.grid_family(), tag_ref.GRID_BORDER, np.uint8))
    res["large_render_s"] = time.perf_counter() - t
    reps = -(-args.large // len(poses))
    board = api.AprilGridBoard(grid.tag_size_meter, grid.tag_spacing, 6, 6)
    res.update(workload("large", np.ascontiguousarray(np.tile(np.stack(poses), (reps, 1, 1))[:args.large]), board))
ctx.close()
print(json.dumps(res))
