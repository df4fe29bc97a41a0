#!/usr/bin/env python3
"""Developer tool: time ccal_covariance (ccal_kernels_cov.hip) at 600 frames, 10 000 frames and 10 000 ragged frames (EUCM, one camera,
the headline problems of bench.py) beside the two calls it is built from, on the same problem at the same point:
  covariance       Problem.covariance() with the point on the device (intr == NULL), all outputs fetched: mode E with the loss into
                   d_r / d_J, the per-frame blocks, the slots' verdicts, mode N at lambda = 0, the host's K x K inverse, the slots' pass,
                   the two sums, the downloads (36 doubles per slot, one per corner)
  covariance bare  the same without cov_poses and leverage fetched
  eval_dev         mode E alone into device buffers (ccal_eval_dev + ccal_sync): the extra write of r and J the call pays
  build_normal_dev mode N alone (ccal_build_normal_dev + ccal_sync)
and, at 600 frames only, the numpy yardstick of tests/cov_ref.py (schur(), with the oracle's evaluation) on the CPU.
The calls block, so the times are wall-clock around one call that ends synchronised, after --warmup untimed rounds that also ramp the
clocks; the variants alternate within a round; the median of --reps rounds is reported with all rounds listed, in ms.  The kernels'
own times come from a trace run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_covariance.py --reps 1 --warmup 1
Prints one JSON line per problem."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from camera_intrinsic_calibration_rs_amd import synth
from camera_intrinsic_calibration_rs_amd.engine import Context, Problem

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--cases", default="600,10000,10000r")
ap.add_argument("--no-yardstick", action="store_true")
args = ap.parse_args()

ctx = Context(0)


def wall(fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


for case in args.cases.split(","):
    ragged = case.endswith("r")
    frames = int(case.rstrip("r"))
    sp = synth.make_problem(frames, "eucm", ragged=ragged)
    prob = Problem.from_synth(ctx, sp)
    intr, poses, _, rep = prob.solve(sp.intr0, sp.poses0)
    prob.upload_params(intr, poses)
    r_dev = torch.empty(2 * prob.n_corners, dtype=torch.float64, device="cuda")
    J_dev = torch.empty(prob.j_len, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    variants = [
        ("covariance", lambda: prob.covariance()),
        ("covariance bare", lambda: prob.covariance(poses_cov=False, leverage=False)),
        ("eval_dev", lambda: prob.eval_dev(r_dev.data_ptr(), J_dev.data_ptr(), apply_loss=True)),
        ("build_normal_dev", lambda: prob.build_normal_dev(0.0)),
    ]
    runs = {name: [] for name, _ in variants}
    for it in range(args.warmup + args.reps):
        for name, fn in variants:
            dt = wall(fn)
            if it >= args.warmup:
                runs[name].append(dt)
    res = prob.covariance()
    out = {"frames": frames, "ragged": ragged, "corners": prob.n_corners, "j_bytes": 8 * (prob.j_len + 2 * prob.n_corners),
           "n_free": res.report.n_free, "leverage_sum": res.report.leverage_sum, "sigma": res.report.sigma2 ** 0.5}
    for name, t in runs.items():
        key = name.replace(" ", "_")
        out[key + "_ms"] = round(statistics.median(t), 3)
        out[key + "_runs_ms"] = [round(x, 3) for x in t]
    if frames <= 600 and not args.no_yardstick:
        import cov_ref
        from oracle import binding as ob
        op = ob.OracleProblem.from_synth(sp)
        t0 = time.perf_counter()
        ref = cov_ref.schur(cov_ref.CovInputs(op, intr, poses))
        out["numpy_yardstick_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["device_vs_yardstick"] = ["%.2e" % x for x in cov_ref.deviation(
            dict(cov_cam=res.cov_cam, cov_poses=res.cov_poses, leverage=res.leverage), ref)]
    print(json.dumps(out), flush=True)
    prob.close()
    del r_dev, J_dev
    torch.cuda.empty_cache()
