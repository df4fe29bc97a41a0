#!/usr/bin/env python3
"""Developer tool: time ccal_refine_poses_batch (k_pose_refine) on 600 and 10 000 frames x 144 corners, EUCM, 0.1 px noise, from the
problem's perturbed poses, default solver options - against (a) the numpy yardstick tests/refine_ref.py on a sample of the frames,
scaled to the batch, and (b) ONE joint ccal_solve (LM) of the same frames with every intrinsic fixed, if the solver accepts such a
problem (the tool says which is the case).  Each GPU figure is the median over --reps calls timed one by one on the host clock
around the blocking call, after --warmup untimed calls; a call includes its uploads and downloads.  Prints one JSON line."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from camera_intrinsic_calibration_rs_amd import _ffi, synth
from camera_intrinsic_calibration_rs_amd.engine import CcalError, Context, Problem, default_opts
import refine_ref

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, nargs="*", default=[600, 10000])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--ref-sample", type=int, default=20)
args = ap.parse_args()
ctx = Context(0)


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


out = {"reps": args.reps}
for n in args.frames:
    sp = synth.make_problem(n, "eucm")
    par = np.zeros(synth.PMAX); par[:6] = sp.intr_gt[0, :6]
    X = np.ascontiguousarray(sp.p3d, dtype=np.float64); U = np.ascontiguousarray(sp.p2d, dtype=np.float64)
    offs = np.ascontiguousarray(sp.obs_offsets, dtype=np.int64)
    poses = np.empty((n, 6)); st = np.empty(n, dtype=np.int32); it = np.empty(n, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def refine():
        poses[:] = sp.poses0
        rc = ctx.lib.ccal_refine_poses_batch(ctx.handle, int(sp.model[0]), dp(par), 1.0, n, offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                             dp(X), dp(U), 4, None, dp(poses), ip(st), ip(it), None, None, None, None)
        assert rc == _ffi.OK
    r = {"refine_ms": median_ms(refine), "status_ok": int((st == _ffi.OK).sum()), "iters_max": int(it.max()), "iters_mean": float(it.mean())}
    k = min(args.ref_sample, n)
    t0 = time.perf_counter()
    for f in range(k):
        a, b = int(offs[f]), int(offs[f + 1])
        refine_ref.refine(int(sp.model[0]), par[:6], X[a:b], U[a:b], sp.poses0[f], 1.0)
    r["numpy_ms_scaled"] = (time.perf_counter() - t0) * 1e3 / k * n
    gp = Problem.from_synth(ctx, sp)
    try:
        for i in range(6):
            gp.fix_param(0, i)
        lm = default_opts(_ffi.METHOD_LM)
        rep = gp.solve(sp.intr_gt, sp.poses0, None, lm)[3]
        r["joint_all_fixed"] = "accepted"
        r["joint_ms"] = median_ms(lambda: gp.solve(sp.intr_gt, sp.poses0, None, lm))
        r["joint_iters"] = int(rep.iterations)
    except CcalError as e:
        r["joint_all_fixed"] = f"refused: {e}"
    gp.close()
    out[str(n)] = r
ctx.close()
print(json.dumps(out))
