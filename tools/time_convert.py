#!/usr/bin/env python3
"""Developer tool: time ccal_convert_model at its usual size - EUCM -> KB4 over the reference's grid of a 512 x 512 image (about 900
rays, 8 unknowns, a handful of Gauss-Newton iterations, each one upload + one launch + one download + a synchronise).  Host clock
around whole calls through the C ABI on one context; median, minimum and maximum over --reps calls after --warmup untimed ones.
Prints one JSON line."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from camera_intrinsic_calibration_rs_amd import _ffi, synth
from camera_intrinsic_calibration_rs_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()

k = args.size / 512.0
src = np.array([190.89618687183938 * k, 190.87022285882367 * k, 254.9375370481962 * k, 256.86414483060787 * k, 0.6283550447635853, 1.0458678747533083])
lib, ctx = _ffi.load(), Context(0)
dp = C.POINTER(C.c_double)
rep = _ffi.Report()


def call():
    tgt = np.zeros(8)
    rc = lib.ccal_convert_model(ctx.handle, synth.MODEL_EUCM, src.ctypes.data_as(dp), synth.MODEL_KB4, tgt.ctypes.data_as(dp),
                                float(args.size), float(args.size), 0, None, C.byref(rep))
    assert rc == _ffi.OK, (rc, ctx.last_error())
    return tgt


for _ in range(args.warmup):
    first = call()
ts = []
for _ in range(args.reps):
    t = time.perf_counter(); out = call(); ts.append((time.perf_counter() - t) * 1e3)
assert (out == first).all()
print(json.dumps({"size": args.size, "reps": args.reps, "iterations": int(rep.iterations), "final_cost": rep.final_cost,
                  "call_ms_median": statistics.median(ts), "call_ms_min": min(ts), "call_ms_max": max(ts),
                  "call_ms_p10": sorted(ts)[len(ts) // 10], "call_ms_p90": sorted(ts)[len(ts) * 9 // 10]}))
ctx.close()
