#!/usr/bin/env python3
"""Developer tool: time the saddle detector at a session's size - 600 frames of 752 x 480 u8 and 64 frames of 1024 x 1024 u16, each
showing a rendered checkerboard (tests/detect_ref.py), default parameters (step 1, nms_radius 5, rel_threshold 0.1).  Host clock
around whole calls, each of which ends in a synchronise: ccal_detect_corners_dev (images resident on the device; candidates down)
and ccal_detect_corners_batch (the image block uploaded as well).  Medians over --reps calls after --warmup untimed ones.  Beside
them the byte-mover time for reading the same bytes once: tools/ubench/hbm_stream.bin with the batch's size as its argument (built
with the hipcc line at the top of hbm_stream.hip; null when it is not there).  The calls hold three kernels, two synchronises and
the result copies; the tile kernel's own time comes from a kernel trace of this tool in a run of its own.  Prints one JSON line."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import detect_ref as ref
from camera_intrinsic_calibration_rs_amd import _ffi
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
STREAM = os.path.join(ROOT, "tools", "ubench", "hbm_stream.bin")


def board(width, height, dtype, f, z):
    cam = ref.Camera(f, (width - 1) / 2.0, (height - 1) / 2.0, -0.2)
    R, t = ref.board_pose(7, 5, 0.03, 20.0, 25.0, 40.0, (0.0, 0.0, z))
    return ref.render_board(width, height, cam, R, t, 7, 5, 0.03, dtype)[0]


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def read_once_us(nbytes):
    if not os.path.exists(STREAM):
        return None
    out = subprocess.run([STREAM, str(nbytes)], capture_output=True, text=True, timeout=120).stdout
    rows = [ln.split() for ln in out.splitlines() if ln.startswith("read-once")]
    return float(rows[0][2]) if rows else None


ctx = Context(0)
out = {"reps": args.reps}
for name, n, W, H, dtype, f, z in (("u8_600x752x480", 600, 752, 480, np.uint8, 900.0, 0.45), ("u16_64x1024x1024", 64, 1024, 1024, np.uint16, 1500.0, 0.40)):
    img = board(W, H, dtype, f, z)
    frames = np.ascontiguousarray(np.broadcast_to(img, (n, H, W)))
    dev = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    code = _ffi.PIX_U8 if dtype == np.uint8 else _ffi.PIX_U16
    res = ctx.detect_corners_dev(dev.data_ptr(), code, W, H, n)
    want = ref.detect(img)
    row = {"bytes": int(frames.nbytes), "candidates_per_frame": res[0][3], "matches_yardstick": bool(
        all(r[3] == want["count"] and np.array_equal(r[0], want["xy"]) and np.array_equal(r[2], want["response"]) for r in res))}
    row["dev_call_ms"] = median_ms(lambda: ctx.detect_corners_dev(dev.data_ptr(), code, W, H, n))
    row["host_call_ms"] = median_ms(lambda: ctx.detect_corners_batch(frames))
    us = read_once_us(frames.nbytes)
    row["read_once_ms"] = None if us is None else us * 1e-3
    row["dev_call_over_read_once"] = None if us is None else row["dev_call_ms"][0] / (us * 1e-3)
    out[name] = row
    del dev
ctx.close()
print(json.dumps(out))
