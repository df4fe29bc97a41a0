"""GPU: the radix select behind validation()'s two numbers (csrc/ccal_kernels_stats.hip: k_sel_one, k_sel_hist, sel_advance,
k_sel_sum, k_sel_finish) on raw values, against the exact integer reference of tests/order_stats_ref.py.

The values go in through ccal_test_order_stats, an entry point of the second library only (csrc/ccal_legacy_test_hooks.hip): it uploads
them and calls order_stats_block, the multi-GPU path's call - the kernels are the product's (one object file in both libraries).

    median    the reference's BIT PATTERN (compared as uint64: also tells +0.0 from -0.0)
    mean      |got - T / 2^80| <= 3 * 2^-53 * T / 2^80, exactly, in Fractions: the device holds T as an exact 128-bit integer and
              rounds three times on the way out (double(hi), double(lo), the add or fma; the scale by 2^-80 is exact).
              T == 0 gives +0.0, the exact grid gives the reference's bits; the non-finite cases give what the kernel documents.

INPUT CONTRACT: values >= +0 (errors are norms).  Negative values and -0.0 are outside it and none is fed to the device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import order_stats_cases as cases
import order_stats_ref as ref
from camera_intrinsic_calibration_rs_amd import _ffi

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def _fn(ctx):
    fn = ctx.lib.ccal_test_order_stats                          # not in _ffi.SYMBOLS: the second library's own
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp]
    return fn


def _run(ctx, vals):
    """(bits of the mean, bits of the median)"""
    v = np.ascontiguousarray(vals, dtype=np.float64)
    out = np.full(2, -1.0)
    rc = _fn(ctx)(ctx.handle, v.ctypes.data_as(_dp), v.size, out[0:].ctypes.data_as(_dp), out[1:].ctypes.data_as(_dp))
    assert rc == _ffi.OK, (rc, ctx.last_error())
    bits = out.view(np.uint64)
    return int(bits[0]), int(bits[1])


def _check(case, got):
    r = case.ref()
    avg_bits, med_bits = got
    avg = float(np.uint64(avg_bits).view(np.float64))
    kind = case.claims["mean"]
    print(f"{case.name}: n {r.n} n99 {r.n99} median {med_bits:#018x} (ref {r.median_bits:#018x}) mean {avg!r} [{kind}]", end="")
    if r.T:
        print(f" rel err {float(abs(Fraction(avg) - r.mean) / r.mean) if np.isfinite(avg) else avg:.3e} (bound {3 * 2.0 ** -53:.3e})", end="")
    print()
    assert med_bits == r.median_bits
    if kind == "nan":
        assert avg != avg
    elif kind == "inf":
        assert avg_bits == ref.INF_BITS
    elif r.T == 0 or r.n99 == 0:
        assert avg_bits == 0                                                # +0.0
    else:
        assert np.isfinite(avg)
        assert abs(Fraction(avg) - r.mean) * (1 << 53) <= 3 * r.mean
        if kind == "exact":
            assert avg_bits == int(np.float64(float(r.mean)).view(np.uint64)) and Fraction(avg) == r.mean


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_statistics_equal_the_exact_reference(dev_ctx, name):
    case = cases.by_name(name)
    _check(case, _run(dev_ctx, case.values()))


@pytest.mark.parametrize("name", ["contested_m13_n8000", "contested_m13_n12000"])
def test_any_order_of_the_values_gives_the_same_bits(dev_ctx, name):
    """one contested case per form: ascending, descending and two random orders"""
    case = cases.by_name(name)
    v = np.sort(case.values())
    rng = np.random.default_rng(99)
    got = [_run(dev_ctx, o) for o in (v, v[::-1], v[rng.permutation(v.size)], v[rng.permutation(v.size)])]
    _check(case, got[0])
    assert got[1] == got[0] and got[2] == got[0] and got[3] == got[0]


def test_work_area_is_clean_for_every_call(dev_ctx):
    """One context, so one cached block: a general-form call, a different one of the same size (the same work area, full of
    the first call's histograms, states and partial sums), a one-launch call, then the first again.  Each is right and the first
    and the last agree - a dropped clear of the work area shows here."""
    a, b, one = (cases.by_name(n) for n in ("contested_m20_n12000", "contested_m31_n12000", "contested_m9_n8000"))
    assert a.claims["form"] == b.claims["form"] == "general" and one.claims["form"] == "one"
    first = _run(dev_ctx, a.values())
    _check(a, first)
    _check(b, _run(dev_ctx, b.values()))
    _check(one, _run(dev_ctx, one.values()))
    last = _run(dev_ctx, a.values())
    _check(a, last)
    assert first == last


def test_bad_arguments_are_refused(dev_ctx):
    fn = _fn(dev_ctx)
    v = np.array([0.5, 0.25, 1.0])
    out = np.zeros(2)
    p, a, m = v.ctypes.data_as(_dp), out[0:].ctypes.data_as(_dp), out[1:].ctypes.data_as(_dp)
    assert fn(dev_ctx.handle, p, 0, a, m) == _ffi.ERR_INVALID_ARG
    assert fn(dev_ctx.handle, p, -3, a, m) == _ffi.ERR_INVALID_ARG
    assert fn(dev_ctx.handle, None, 3, a, m) == _ffi.ERR_INVALID_ARG
    assert fn(dev_ctx.handle, p, 3, None, m) == _ffi.ERR_INVALID_ARG
    assert fn(dev_ctx.handle, p, 3, a, None) == _ffi.ERR_INVALID_ARG
    assert fn(None, p, 3, a, m) == _ffi.ERR_INVALID_ARG
    assert "ccal_test_order_stats" in dev_ctx.last_error()
    assert fn(dev_ctx.handle, p, 3, a, m) == _ffi.OK and out[1] == 0.5
