"""The yardstick for the f64 device math of csrc/ccal_device.hpp (TEST INFRASTRUCTURE): every function from its definition in
mpmath at 60 digits, and the error measure of tests/test_gpu_device_math.py.

    rcp(x) = 1 / x                     sqrt_rsqrt(x) = (sqrt x, 1 / sqrt x)           sincos(x) = (sin x, cos x)
    atan2_pos(r, z) = atan2(r, z)      huber_sw(s, d) = sqrt(d / sqrt s) if d > 0 and s > d^2, else 1
    so3(w) = (R, J_l), row-major 9 + 9:  R = I + a W + b W^2  (the matrix Rodrigues formula),  J_l = a I + b W + e w w^T,
             a = sin t / t, b = (1 - cos t) / t^2, e = (t - sin t) / t^3 evaluated as written (no series: 60 digits carry the
             cancellation of e down to t ~ 1e-6 with 40 digits to spare), t = 0 -> (I, I).

Inputs are doubles and are taken exactly (mpf(float) is exact)."""
import math

import mpmath as mp

DPS = 60
OPS = ("RCP", "SQRT_RSQRT", "SINCOS", "ATAN2_POS", "SO3", "HUBER_SW")
N_IN = dict(RCP=1, SQRT_RSQRT=1, SINCOS=1, ATAN2_POS=2, SO3=3, HUBER_SW=2)
N_OUT = dict(RCP=1, SQRT_RSQRT=2, SINCOS=2, ATAN2_POS=1, SO3=18, HUBER_SW=1)


def _mp(f):
    def g(*a):
        with mp.workdps(DPS):
            return f(*[mp.mpf(float(x)) for x in a])
    g.__name__ = f.__name__
    return g


@_mp
def rcp(x):
    return (1 / x,)


@_mp
def sqrt_rsqrt(x):
    s = mp.sqrt(x)
    return (s, 1 / s)


@_mp
def sincos(x):
    return (mp.sin(x), mp.cos(x))


@_mp
def atan2_pos(r, z):
    return (mp.atan2(r, z),)


@_mp
def huber_sw(s, d):
    return (mp.sqrt(d / mp.sqrt(s)),) if d > 0 and s > d * d else (mp.mpf(1),)


def skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


@_mp
def so3(x, y, z):
    w = (x, y, z)
    t2 = x * x + y * y + z * z
    if t2 == 0:
        return tuple(mp.eye(3)) * 2
    t = mp.sqrt(t2)
    a, b, e = mp.sin(t) / t, (1 - mp.cos(t)) / t2, (t - mp.sin(t)) / (t2 * t)
    W = skew(w)
    R = mp.eye(3) + a * W + b * (W * W)
    J = a * mp.eye(3) + b * W + e * (mp.matrix(w) * mp.matrix(w).T)
    return tuple(R) + tuple(J)               # mp.matrix iterates row-major


FUNCS = dict(RCP=rcp, SQRT_RSQRT=sqrt_rsqrt, SINCOS=sincos, ATAN2_POS=atan2_pos, SO3=so3, HUBER_SW=huber_sw)


def reference(op, inputs):
    """rows of N_OUT[op] mpf values for an (n, N_IN[op]) array of doubles"""
    f = FUNCS[op]
    return [f(*row) for row in inputs]


def spacing(ref):
    """the spacing of the doubles in the binade of the correctly rounded reference (the smallest normal's for anything below)"""
    r = abs(float(ref))
    if r == 0.0:
        return 2.0 ** -1074
    return 2.0 ** (max(math.frexp(r)[1] - 1, -1022) - 52)


def ulps(got, ref):
    """|got - ref| / spacing(ref), as a float; inf for a non-finite got"""
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    with mp.workdps(DPS):
        return float(abs(mp.mpf(got) - ref) / mp.mpf(spacing(ref)))


def abs_err(got, ref):
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    with mp.workdps(DPS):
        return float(abs(mp.mpf(got) - ref))
