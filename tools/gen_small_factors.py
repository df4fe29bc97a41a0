#!/usr/bin/env python3
"""Developer tool: record what the library computes for the two small factors, bit for bit, into tests/golden/small_factors_parent.json
(inputs and results, doubles as hex).  Run on the commit whose arithmetic is the yardstick; the tests then hold every later commit to it.
    --extrinsic   ccal_init_camera_extrinsic_opts (host code, no GPU): seeded pose pairs, n_common 1 / 3 / 20, a gross outlier pair
                  (the Huber branch s > 0.25), use_initial 0 and 1, error_metric 1, max_iterations 1 - and two inputs that overflow
                  the 6 x 6 system (entries of 1e200, an inf), of which only the status is on record
    --convert     ccal_convert_model (needs the GPU): every row of test_convert_model_vs_oracle at 512 x 512, EUCM -> KB4 at 640 x 480
                  and at 40 x 32 (step 1, edge 0: 1 280 grid points on one workgroup)
A section that is not asked for is kept as the file has it.  --out writes elsewhere (the inputs still come from the golden file)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import small_factors as sf
from camera_intrinsic_calibration_rs_amd import _ffi, synth

_EUCM = [190.89618687183938, 190.87022285882367, 254.9375370481962, 256.86414483060787, 0.6283550447635853, 1.0458678747533083]
_KB4 = [190.9, 190.9, 255.0, 257.0, 0.003, 0.0007, -0.002, 0.0002]
_CV5 = [380.0, 380.0, 255.0, 257.0, -0.28, 0.07, 0.0002, 0.00002, 0.0]


def _pose_pairs(seed, n):
    """board poses of camera 0 and, through one true relative pose plus noise, of camera i (composition left to the library's own
    start value: the pairs only have to be consistent up to the noise)"""
    rng = np.random.default_rng(seed)
    p0 = np.concatenate([0.2 * rng.standard_normal((n, 3)), rng.standard_normal((n, 3))], axis=1)
    pi = p0 + 0.01 * rng.standard_normal((n, 6))
    pi[:, 3] += 0.1
    return p0, pi


def extrinsic_cases():
    cases = []
    def add(name, p0, pi, x0=None, use_initial=0, opts=None):
        cases.append({"name": name, "poses0": sf.to_hex(p0), "posesi": sf.to_hex(pi), "x0": sf.to_hex(np.zeros(6) if x0 is None else x0),
                      "use_initial": use_initial, "opts": opts})
    for n in (1, 3, 20):
        add(f"n{n}", *_pose_pairs(100 + n, n))
    p0, pi = _pose_pairs(7, 20)
    pi[5] += [0.9, -0.7, 0.5, 2.0, -1.5, 1.0]                    # a gross outlier pair: |r|^2 far above 0.25
    add("outlier", p0, pi)
    p0, pi = _pose_pairs(8, 20)
    add("use_initial", p0, pi, x0=[0.01, -0.02, 0.015, 0.12, 0.01, -0.02], use_initial=1)
    p0, pi = _pose_pairs(12, 20)
    pi[3] -= [0.5, 0.6, -0.8, 1.0, 2.0, -1.0]
    add("use_initial_outlier", p0, pi, x0=[0.3, 0.2, -0.1, 0.5, -0.4, 0.3], use_initial=1)
    add("error_metric", *_pose_pairs(9, 20), opts={"error_metric": 1})
    add("max_iterations_1", *_pose_pairs(10, 20), opts={"max_iterations": 1})
    return cases


def overflow_cases():
    p0, pi = _pose_pairs(11, 3)
    big0, bigi = p0.copy(), pi.copy()
    big0[:, 3:] = 1e200; bigi[:, 3:] = -1e200
    inf0 = p0.copy(); inf0[1, 4] = np.inf
    mk = lambda name, a, b: {"name": name, "poses0": sf.to_hex(a), "posesi": sf.to_hex(b), "x0": sf.to_hex(np.zeros(6)), "use_initial": 0, "opts": None}
    return [mk("entries_1e200", big0, bigi), mk("an_inf", inf0, pi)]


def convert_cases():
    M = synth.MODEL_NAMES
    rows = [("eucm", _EUCM, "kb4", [0.0] * 8, 0), ("eucm", _EUCM, "kb4", [0.0] * 8, 2), ("eucm", _EUCM, "ucm", [0, 0, 0, 0, 0.6], 0),
            ("kb4", _KB4, "eucm", [0, 0, 0, 0, 0.5, 1.0], 0), ("opencv5", _CV5, "kb4", [0.0] * 8, 0), ("kb4", _KB4, "opencv5", [0.0] * 9, 0),
            ("ucm", _EUCM[:5], "kb4", [0.0] * 8, 0)]
    cases = [{"name": f"{s}_to_{t}_d{d}_512x512", "src": M[s], "tgt": M[t], "src_params": sf.to_hex(sp), "tgt_params": sf.to_hex(tp),
              "width": 512, "height": 512, "disabled": d} for s, sp, t, tp, d in rows]
    for w, h in ((640, 480), (40, 32)):
        k = w / 512.0
        sp = [_EUCM[0] * k, _EUCM[1] * k, 0.498 * w, 0.502 * h, _EUCM[4], _EUCM[5]]
        cases.append({"name": f"eucm_to_kb4_d0_{w}x{h}", "src": M["eucm"], "tgt": M["kb4"], "src_params": sf.to_hex(sp),
                      "tgt_params": sf.to_hex([0.0] * 8), "width": w, "height": h, "disabled": 0})
    return cases


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--extrinsic", action="store_true")
    ap.add_argument("--convert", action="store_true")
    ap.add_argument("--out", default=sf.FIXTURE)
    args = ap.parse_args()
    doc = sf.load() if os.path.exists(sf.FIXTURE) else {}
    lib = _ffi.load()
    if args.extrinsic:
        doc["extrinsic"] = [dict(c, expect=sf.run_extrinsic(lib, c)) for c in extrinsic_cases()]
        doc["extrinsic_overflow"] = [dict(c, expect_status=sf.run_extrinsic(lib, c)["status"]) for c in overflow_cases()]
        for c in doc["extrinsic"] + doc["extrinsic_overflow"]:
            print(c["name"], c.get("expect", c.get("expect_status")))
    if args.convert:
        from camera_intrinsic_calibration_rs_amd.engine import Context
        ctx = Context(0)
        doc["convert"] = [dict(c, expect=sf.run_convert(lib, ctx.handle, c)) for c in convert_cases()]
        ctx.close()
        for c in doc["convert"]:
            print(c["name"], c["expect"])
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
