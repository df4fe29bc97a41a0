"""GPU: the six pieces of f64 device math of csrc/ccal_device.hpp on the named inputs of tests/device_math_cases.py, against the
mpmath yardstick of tests/device_math_ref.py.

The inputs go in through ccal_test_device_math, an entry point of the second library only (csrc/ccal_legacy_test_hooks.hip): one element
per lane, the header's functions as they are.  Bounds are the header's own written claims, or derived from the arithmetic:

    RCP, SQRT_RSQRT   2 ulp                        the header's "<= 1-2 ulp"
    SINCOS            |ds|, |dc| <= 2^-52 ABSOLUTE kd * pio2_1 is exact (33 + 17 bits), the second fma rounds once (<= 2^-54 for
                                                   |r| < 0.79), the tail's own error is <= 6e4 * 7e-27, the kernel polynomials stay
                                                   under 1 ulp of a result <= 1.  No error RELATIVE to a tiny sine next to a multiple
                                                   of pi is claimed; a rotation matrix does not need it.
    ATAN2_POS         3 ulp                        the header's "~2 ulp"
    SO3               8 (1 + |w|) 2^-53 per entry  the computed angle carries the error of three rounded squares and a 2-ulp root,
                                                   which moves sin t and cos t by ~1.5 t 2^-53 before fast_sincos adds its 2^-52;
                                                   each entry then takes about six roundings at magnitude <= 2
    HUBER_SW          4 ulp                        two chained 2-ulp roots; the square root halves the first one's error

ulp = the spacing of the binade of the correctly rounded reference (device_math_ref.ulps).  Each test prints the worst error of
every list and the argument it is at."""
import ctypes as C

import numpy as np
import pytest

import device_math_cases as cases
import device_math_ref as ref
from camera_intrinsic_calibration_rs_amd import _ffi

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
OP = {name: i for i, name in enumerate(ref.OPS)}


def _fn(ctx):
    fn = ctx.lib.ccal_test_device_math                          # not in _ffi.SYMBOLS: the second library's own
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int64, _dp, _dp]
    return fn


def _run(ctx, op, inputs):
    v = np.ascontiguousarray(inputs, dtype=np.float64).reshape(-1, ref.N_IN[op])
    out = np.full((v.shape[0], ref.N_OUT[op]), np.nan)
    rc = _fn(ctx)(ctx.handle, OP[op], v.shape[0], v.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    assert rc == _ffi.OK, (rc, ctx.last_error())
    return out


def _worst(case, got, measure):
    """(worst error, its row) over every output of every row; printed"""
    want = case.reference()
    err = np.array([[measure(g, w) for g, w in zip(grow, wrow)] for grow, wrow in zip(got, want)])
    i = int(np.argmax(err.max(1)))
    print(f"{case.name}: n {len(got)} worst {err.max():.3f} at {case.inputs()[i].tolist()!r} got {got[i].tolist()!r}")
    return err


@pytest.mark.parametrize("op, bound", [("RCP", 2.0), ("SQRT_RSQRT", 2.0), ("ATAN2_POS", 3.0), ("HUBER_SW", 4.0)])
def test_relative_error_in_ulps(dev_ctx, op, bound):
    worst = {}
    for case in cases.of_op(op):
        got = _run(dev_ctx, op, case.inputs())
        if case.claims.get("exact_one"):
            print(f"{case.name}: n {len(got)} exactly 1.0: {bool((got == 1.0).all())}")
            worst[case.name] = 0.0 if (got == 1.0).all() else np.inf
        else:
            worst[case.name] = float(_worst(case, got, ref.ulps).max())
    print(f"{op}: worst {max(worst.values()):.3f} ulp (bound {bound})")
    assert all(w <= bound for w in worst.values()), worst


def test_sincos_absolute_error(dev_ctx):
    bound, worst = 2.0 ** -52, {}
    for case in cases.of_op("SINCOS"):
        err = _worst(case, _run(dev_ctx, "SINCOS", case.inputs()), lambda g, w: ref.abs_err(g, w) * 2.0 ** 53)     # in units of 2^-53
        worst[case.name] = float(err.max()) * 2.0 ** -53
    print(f"SINCOS: worst {max(worst.values()) * 2.0 ** 53:.3f} * 2^-53 absolute (bound 2 * 2^-53)")
    assert all(w <= bound for w in worst.values()), worst


def test_so3_entries(dev_ctx):
    worst = {}
    for case in cases.of_op("SO3"):
        v = case.inputs()
        got = _run(dev_ctx, "SO3", v)
        if case.claims.get("identity"):
            eye = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1] * 2)
            assert (got.view(np.uint64) == np.tile(eye, (len(v), 1)).view(np.uint64)).all(), got     # bit for bit, +0.0 included
        err = _worst(case, got, lambda g, w: ref.abs_err(g, w) * 2.0 ** 53)
        rel = err.max(1) / (1.0 + np.sqrt((v ** 2).sum(1)))                    # in units of (1 + |w|) 2^-53
        i = int(np.argmax(rel))
        print(f"    worst {rel[i]:.3f} (1 + |w|) 2^-53 at w = {v[i].tolist()!r}, |w| = {np.linalg.norm(v[i])!r}")
        worst[case.name] = float(rel.max())
    print(f"SO3: worst {max(worst.values()):.3f} (1 + |w|) 2^-53 (bound 8)")
    assert all(w <= 8.0 for w in worst.values()), worst


def test_so3_is_the_same_in_every_lane(dev_ctx):
    """one launch, the same w in different lanes, wavefronts and workgroups among other rows: bit-identical"""
    base = cases.by_name("so3_angles").inputs()
    v = np.array(np.tile(base, (3, 1))[:1000])
    where = {}
    for j, src in enumerate((5, 100, 257, 401)):
        where[src] = [src] + [(131 * (j + 1) + 67 * m) % len(v) for m in range(1, 6)]
        v[where[src]] = base[src]
    got = _run(dev_ctx, "SO3", v).view(np.uint64)
    for src, rows in where.items():
        assert len({r % 64 for r in rows}) > 1 and len({r // 256 for r in rows}) > 1
        for r in rows[1:]:
            assert (got[r] == got[rows[0]]).all(), (src, r)


def test_sqrt_of_zero_is_not_positive(dev_ctx):
    """r2 == 0 on the optical axis: KB4's `r > threshold` and `s > 0` must be false, whatever s is (project_partials)"""
    got = _run(dev_ctx, "SQRT_RSQRT", np.array([0.0, 1.0, 0.0]))
    print("sqrt_rsqrt(0) =", got[0].tolist())
    assert not (got[0, 0] > 0) and not (got[2, 0] > 0) and got[1, 0] == 1.0 and got[1, 1] == 1.0


def test_bad_arguments_are_refused(dev_ctx):
    fn = _fn(dev_ctx)
    v, out = np.array([0.5, 0.25, 1.0, 2.0]), np.full(36, -7.0)
    p, o = v.ctypes.data_as(_dp), out.ctypes.data_as(_dp)
    for op, n in ((-1, 1), (len(ref.OPS), 1), (1 << 20, 1), (0, 0), (0, -3), (4, 0)):
        assert fn(dev_ctx.handle, op, n, p, o) == _ffi.ERR_INVALID_ARG, (op, n)
        assert "ccal_test_device_math" in dev_ctx.last_error()
    assert fn(dev_ctx.handle, 0, 1, None, o) == _ffi.ERR_INVALID_ARG
    assert fn(dev_ctx.handle, 0, 1, p, None) == _ffi.ERR_INVALID_ARG
    assert fn(None, 0, 1, p, o) == _ffi.ERR_INVALID_ARG
    assert (out == -7.0).all()                                                  # nothing was launched
    assert fn(dev_ctx.handle, 0, 4, p, o) == _ffi.OK
    assert out[:4].tolist() == [2.0, 4.0, 1.0, 0.5] and (out[4:] == -7.0).all()
