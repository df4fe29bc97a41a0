"""The two small factors through the C ABI, for the bit-for-bit record of tests/golden/small_factors_parent.json: one call of
ccal_init_camera_extrinsic_opts (host code, no GPU) or of ccal_convert_model (device) for a case of the fixture, and the result in the
fixture's form - doubles as C99 hex strings, so that equality is equality of bits.  tools/gen_small_factors.py wrote the record with
these functions; tests/test_small_factors_cpu.py and tests/test_gpu_api.py hold the library to it with the same ones."""
import ctypes as C
import json
import os

import numpy as np

from camera_intrinsic_calibration_rs_amd import _ffi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_factors_parent.json")
_dp = C.POINTER(C.c_double)


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def to_hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def from_hex(h):
    return np.array([float.fromhex(s) for s in h], dtype=np.float64)


def _opts(lib, kw):
    if kw is None:
        return None
    o = _ffi.SolverOpts()
    lib.ccal_set_defaults(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def run_extrinsic(lib, case):
    """case: poses0 / posesi (hex, n_common x 6), x0 (hex, 6), use_initial, opts (None = NULL, else fields over the defaults)"""
    p0, pi, x = from_hex(case["poses0"]), from_hex(case["posesi"]), from_hex(case["x0"]).copy()
    o, rep = _opts(lib, case["opts"]), _ffi.Report()
    rc = lib.ccal_init_camera_extrinsic_opts(p0.ctypes.data_as(_dp), pi.ctypes.data_as(_dp), len(p0) // 6, x.ctypes.data_as(_dp),
                                             int(case["use_initial"]), C.byref(o) if o is not None else None, C.byref(rep))
    return {"rc": int(rc), "x": to_hex(x), "iterations": int(rep.iterations), "initial_cost": float(rep.initial_cost).hex(),
            "final_cost": float(rep.final_cost).hex(), "status": int(rep.status)}


def run_convert(lib, ctx_handle, case):
    """case: src / tgt (model ids), src_params / tgt_params (hex), width, height, disabled"""
    src, tgt = from_hex(case["src_params"]), from_hex(case["tgt_params"]).copy()
    rep = _ffi.Report()
    rc = lib.ccal_convert_model(ctx_handle, int(case["src"]), src.ctypes.data_as(_dp), int(case["tgt"]), tgt.ctypes.data_as(_dp),
                                float(case["width"]), float(case["height"]), int(case["disabled"]), None, C.byref(rep))
    return {"rc": int(rc), "params": to_hex(tgt), "iterations": int(rep.iterations), "final_cost": float(rep.final_cost).hex(),
            "status": int(rep.status)}
