"""Named inputs for the f64 device math of csrc/ccal_device.hpp (TEST INFRASTRUCTURE: tests/test_device_math_cpu.py checks what
every list claims, tests/test_gpu_device_math.py feeds the lists to the device through ccal_test_device_math).

Every list has a fixed seed, the op it is for, the seam or regime it is there for (`why`) and a dict of claims.  A list is an
(n, N_IN[op]) array of doubles; values that have to sit a given number of ulps from a seam are stepped with np.nextafter.

INPUT CONTRACT per op (nothing outside it is fed to the device, except the four cases named `outside`, whose result is pinned):
    RCP         finite, 2^-500 <= |x| <= 2^500
    SQRT_RSQRT  2^-500 <= x <= 2^500                 (outside: x = 0, for which only `s > 0 is false` is asserted)
    SINCOS      |x| <= 1e5
    ATAN2_POS   r > 0, both finite
    SO3         |w| <= 40
    HUBER_SW    s > delta^2 > 0, s / delta^2 <= 1e12 (outside, result exactly 1: s == delta^2, delta == 0, delta < 0)

Claims (tests/test_device_math_cpu.py):
    straddle: f            f(rows) -> bool array; both sides occur in the list
    k_of: f                SINCOS: f(rows) -> the quadrant count k = rint(x 2/pi) each row names; checked in mpmath
    tie                    SINCOS: every x is within 4 ulp of (k + 1/2) pi/2 for an integer k
    exact_one              HUBER_SW: the result must be exactly 1.0
    identity               SO3: R = J_l = I bit for bit
"""
from __future__ import annotations

from dataclasses import dataclass, field

import mpmath as mp
import numpy as np

import device_math_ref as ref

PI = np.pi
TAN_PI_8 = 0.41421356237309503           # the constant of fast_atan2_pos's `sel`
KB4_SMALL_RADIUS = 1e-8
SO3_SERIES_T2 = 0.04
SO3_ANGLES = (0.3, 1.0, PI / 2, 2.0, PI - 1e-6, PI + 1e-6, 3.5, 4.0, 5.5, 2 * PI - 1e-3, 2 * PI + 1e-3, 2 * PI - 1e-9,
              2 * PI + 1e-9, 7.0, 9.0, 4 * PI - 0.01, 12.9, 40.0)
HUBER_DELTAS = (1.0, 0.25, 3.0)


@dataclass
class CaseList:
    name: str
    op: str
    seed: int
    why: str
    build: object                    # rng -> array (n, N_IN[op]) or (n,)
    claims: dict = field(default_factory=dict)

    def inputs(self) -> np.ndarray:
        if self.name not in _INPUTS:
            v = np.ascontiguousarray(self.build(np.random.default_rng(self.seed)), dtype=np.float64).reshape(-1, ref.N_IN[self.op])
            v.setflags(write=False)
            _INPUTS[self.name] = v
        return _INPUTS[self.name]

    def reference(self):
        """the mpmath rows, computed once per process and shared"""
        if self.name not in _REFS:
            _REFS[self.name] = ref.reference(self.op, self.inputs())
        return _REFS[self.name]


_INPUTS: dict = {}
_REFS: dict = {}
LISTS: list = []


def _add(name, op, seed, why, build, **claims):
    LISTS.append(CaseList(name, op, seed, why, build, claims))


def by_name(name) -> CaseList:
    return next(c for c in LISTS if c.name == name)


def of_op(op):
    return [c for c in LISTS if c.op == op]


def step(x, k):
    """x moved by k ulps (k of either sign), elementwise"""
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _steps(x, ks):
    return np.concatenate([np.atleast_1d(step(x, k)) for k in ks])


# ---- RCP, SQRT_RSQRT ------------------------------------------------------------------------------------------------------
def _exponents(rng):
    e = np.arange(-500, 500)
    return np.ldexp(rng.uniform(1.0, 2.0, e.size), e)


def _pow2(rng):
    return np.concatenate([np.ldexp(1.0, np.arange(-500, 501)), [step(1.0, 1), step(1.0, -1)]])


def _mantissa_steps(rng):
    """mantissas next to 1 and 2 (the seed's table wraps) and next to sqrt 2 (where rsq's table steps between an even and an
    odd exponent), 0 .. 8 ulps either side, at a few even and odd exponents"""
    m = np.concatenate([_steps(1.0, range(0, 9)), _steps(2.0, range(-8, 0)), _steps(np.sqrt(2.0), range(-8, 9)),
                        _steps(1.5, range(-2, 3))])
    return np.concatenate([np.ldexp(m, e) for e in (-500, -101, -2, -1, 0, 1, 2, 100, 499)])


def _rcp_call_sites(rng):
    depth = rng.uniform(0.1, 10.0, 1000)
    x, y, z = rng.uniform(-2, 2, 600), rng.uniform(-2, 2, 600), rng.uniform(-0.5, 3.0, 600)
    alpha, beta = rng.choice([0.3, 0.6, 0.9], 600), rng.choice([0.7, 1.0, 1.3], 600)
    n = alpha * np.sqrt(beta * (x * x + y * y) + z * z) + (1 - alpha) * z        # the UCM / EUCM denominator
    return np.concatenate([depth, n[n > 1e-3], (x * x + y * y + z * z)])          # and KB4's r^2 + z^2


def _sqrt_call_sites(rng):
    res = rng.normal(0, 1, (1200, 2)) * 10.0 ** rng.uniform(-3, 2.5, (1200, 1))   # pixel residuals, 1e-3 .. 300 px
    x, y, z = rng.uniform(-2, 2, 800), rng.uniform(-2, 2, 800), rng.uniform(-3.0, 3.0, 800)
    beta = rng.choice([0.7, 1.0, 1.3], 800)
    w = rng.normal(0, 1, (400, 3)) * rng.uniform(0.2, 7.0, (400, 1))              # t^2 of the exp map
    return np.concatenate([(res ** 2).sum(1), beta * (x * x + y * y) + z * z, x * x + y * y, (w ** 2).sum(1)])


def _both_signs(build):
    def f(rng):
        v = build(rng)
        return np.concatenate([v, -v])
    return f


for _n, _b, _why in (("exponents", _exponents, "a seeded mantissa at every exponent -500 .. 499"),
                     ("pow2", _pow2, "exact powers of two 2^-500 .. 2^500, and 1 +- 1 ulp"),
                     ("mantissa_steps", _mantissa_steps, "mantissas next to 1, 2 and sqrt 2, where the hardware seed's table steps"),
                     ("call_sites", None, "the arguments the call sites produce")):
    _add(f"rcp_{_n}", "RCP", 11, _why + ", both signs", _both_signs(_b or _rcp_call_sites))
    _add(f"sqrt_{_n}", "SQRT_RSQRT", 12, _why, _b or _sqrt_call_sites)


# ---- SINCOS ---------------------------------------------------------------------------------------------------------------
SINCOS_K_SMALL = tuple(range(-8, 41))
SINCOS_K_LARGE = tuple(int(k) for k in np.unique(np.round(np.geomspace(41, 63661, 30))))     # 63661 = floor(1e5 * 2 / pi)
_NEIGH = (-2, -1, 0, 1, 2)


def _half_pi_times(k):
    """the double nearest to k pi/2 (k may be a half integer)"""
    with mp.workdps(ref.DPS):
        return float(mp.mpf(float(k)) * mp.pi / 2)


def _multiples(ks):
    def build(rng):
        return np.concatenate([_steps(_half_pi_times(k), _NEIGH) for k in ks])
    return build


def _multiples_k(ks):
    return lambda rows: np.repeat(np.array(ks), len(_NEIGH))


def _ties(rng):
    ks = np.concatenate([np.arange(-9, 41), SINCOS_K_LARGE[:-1]])
    return np.concatenate([_steps(_half_pi_times(k + 0.5), (-4, -1, 0, 1, 4)) for k in ks])


def _log_magnitudes(rng):
    m = 10.0 ** rng.uniform(-12, 5, 600)
    return np.minimum(np.concatenate([m, -m, [1e5, -1e5, 1e-300, 0.0]]), 1e5)


def _half_angles(rng):
    return 0.5 * np.concatenate([np.array(SO3_ANGLES), rng.uniform(0.2, 40.0, 800)])


_add("sincos_dense", "SINCOS", 21, "[0, 4 pi] dense: quadrants k = 0 .. 8", lambda rng: np.linspace(0.0, 4 * PI, 4001))
_add("sincos_coarse", "SINCOS", 22, "[-4 pi, 4 pi] coarse: negative k", lambda rng: np.linspace(-4 * PI, 4 * PI, 1001))
_add("sincos_multiples_small", "SINCOS", 23, "the doubles nearest k pi/2, k = -8 .. 40, +- 1, 2 ulp: the Cody-Waite tail decides r",
     _multiples(SINCOS_K_SMALL), k_of=_multiples_k(SINCOS_K_SMALL))
_add("sincos_multiples_large", "SINCOS", 24, "the same for thirty k up to 1e5 * 2 / pi: kd * tail at its largest",
     _multiples(SINCOS_K_LARGE), k_of=_multiples_k(SINCOS_K_LARGE))
_add("sincos_ties", "SINCOS", 25, "ties of rint(x 2/pi): |r| at its largest, either k is right", _ties, tie=True)
_add("sincos_log", "SINCOS", 26, "log-spaced magnitudes 1e-12 .. 1e5, both signs, and 0", _log_magnitudes)
_add("sincos_half_angles", "SINCOS", 27, "the half angles 0.5 t the exp map feeds it", _half_angles)


# ---- ATAN2_POS ------------------------------------------------------------------------------------------------------------
def _atan2_log(rng):
    r, z = 2.0 ** rng.uniform(-60, 60, 1500), 2.0 ** rng.uniform(-60, 60, 1500)
    z[::2] = -z[::2]
    return np.stack([r, z], 1)


_SEAM_K = tuple(range(-4, 5))


def _seam_rows(base, ratio, vary_r):
    """base: the magnitudes of the coordinate held fixed; the other is fl(ratio * base) stepped by -4 .. 4 ulp; both signs of z"""
    rows = []
    for b in base:
        for v in _steps(ratio * b, _SEAM_K):
            r, az = (v, b) if vary_r else (b, v)
            rows += [(r, az), (r, -az)]
    return np.array(rows)


def _seam_base(rng):
    return np.concatenate([[1.0, 0.75, 3.0, 2.0 ** -40, 2.0 ** 40], rng.uniform(0.05, 20.0, 40)])


def sel_of(rows):
    """fast_atan2_pos's own predicates in its own arithmetic (one rounded product, two comparisons): (big, sel)"""
    r, az = rows[:, 0], np.abs(rows[:, 1])
    big = r > az
    a, b = np.where(big, az, r), np.where(big, r, az)
    return big, a > TAN_PI_8 * b


_add("atan2_log", "ATAN2_POS", 31, "log-spaced r and |z| over 2^+-60, both signs of z: all five octant cases", _atan2_log)
_add("atan2_seam_tan_pi_8", "ATAN2_POS", 32, "r / |z| = tan(pi/8) +- 4 ulp: the switch to (a - b) / (a + b), octants 0 | 1 and 4 | 3",
     lambda rng: _seam_rows(_seam_base(rng), TAN_PI_8, True), straddle=lambda rows: sel_of(rows)[1], ratio=TAN_PI_8)
_add("atan2_seam_one", "ATAN2_POS", 33, "r / |z| = 1 +- 4 ulp: a and b swap, x = (a - b) / (a + b) crosses 0",
     lambda rng: _seam_rows(_seam_base(rng), 1.0, True), straddle=lambda rows: sel_of(rows)[0], ratio=1.0)
_add("atan2_seam_cot_pi_8", "ATAN2_POS", 34, "|z| / r = tan(pi/8) +- 4 ulp: octants 1 | 2 and 3 | 2",
     lambda rng: _seam_rows(_seam_base(rng), TAN_PI_8, False), straddle=lambda rows: sel_of(rows)[1], ratio=1 / TAN_PI_8)
_TINY = float(np.finfo(np.float64).tiny)
_add("atan2_z_zero", "ATAN2_POS", 35, "z = +-0 exactly and z = +- the smallest normal: theta = pi/2",
     lambda rng: np.array([(r, z) for r in (2.0 ** -60, 1e-8, 1.0, 3.7, 2.0 ** 60) for z in (0.0, -0.0, _TINY, -_TINY)]))
_add("atan2_kb4_threshold", "ATAN2_POS", 36, "r = 1e-8 (1 + 2^-52) at z = +-1: the first radius past the KB4 threshold",
     lambda rng: np.array([(float(step(KB4_SMALL_RADIUS, 1)), 1.0), (float(step(KB4_SMALL_RADIUS, 1)), -1.0)]))


def _atan2_extreme(rng):
    m1, m2 = rng.uniform(1, 2, 100), rng.uniform(1, 2, 100)
    sgn = np.where(np.arange(100) % 2, -1.0, 1.0)
    return np.concatenate([np.stack([np.ldexp(m1, 100), sgn * np.ldexp(m2, -100)], 1),
                           np.stack([np.ldexp(m1, -100), sgn * np.ldexp(m2, 100)], 1)])


_add("atan2_extreme_ratio", "ATAN2_POS", 37, "r >> |z| and r << |z| by 2^+-200", _atan2_extreme)


# ---- SO3 ------------------------------------------------------------------------------------------------------------------
def so3_axes(rng):
    """the three coordinate axes and twenty seeded unit vectors"""
    a = rng.normal(0, 1, (20, 3))
    return np.concatenate([np.eye(3), a / np.linalg.norm(a, axis=1, keepdims=True)])


def _inside(w, limit=40.0):
    """shrink by ulps until the rounded norm is inside the contract"""
    w = np.array(w, dtype=np.float64)
    for i in range(len(w)):
        while np.sqrt(np.sum(np.longdouble(w[i]) ** 2)) > limit:
            w[i] = w[i] * (1 - 2.0 ** -52)
    return w


def _so3_angles(rng):
    ax = so3_axes(rng)
    return _inside(np.concatenate([t * ax for t in SO3_ANGLES]))


def _so3_seam_axis(rng):
    """w along one coordinate axis: t^2 = fl(x^2) whatever the contraction of the sum of squares, so the side is known"""
    x = _steps(np.sqrt(SO3_SERIES_T2), range(-4, 5))
    return np.concatenate([np.outer(s * x, e) for e in np.eye(3) for s in (1.0, -1.0)])


def _so3_seam_generic(rng):
    """seeded axes, |w|^2 within a few ulp of 0.04: the side depends on how the sum rounds, both branches must be right"""
    ax = so3_axes(rng)[3:]
    return np.concatenate([ax * s for s in _steps(np.sqrt(SO3_SERIES_T2), (-3, -1, 0, 1, 3))])


def _so3_zero_components(rng):
    rows = []
    for t in (1e-3, 0.19, 0.3, 2.0, PI - 1e-6, 4.0, 2 * PI - 1e-3, 12.9):
        for i in range(3):
            for sgn in (1.0, -1.0):
                one = np.full(3, sgn * t / np.sqrt(2.0)); one[i] = 0.0           # one zero component
                two = np.zeros(3); two[i] = sgn * t                              # two zero components
                rows += [one * np.array([1.0, -1.0, 1.0]), two]
    return np.array(rows)


_add("so3_angles", "SO3", 41, "angles 0.3 .. 40 (quadrants k up to 25, pi and 2 pi neighbourhoods) about 23 axes", _so3_angles)
_add("so3_seam_axis", "SO3", 42, "t^2 = 0.04 +- 4 ulp about the coordinate axes: series | closed form",
     _so3_seam_axis, straddle=lambda rows: (rows ** 2).sum(1) < SO3_SERIES_T2)
_add("so3_seam_generic", "SO3", 43, "|w|^2 within a few ulp of 0.04 about seeded axes", _so3_seam_generic)
_add("so3_zero_components", "SO3", 44, "w with one and with two zero components, both signs", _so3_zero_components)
_add("so3_small", "SO3", 45, "the series side: angles 1e-9 .. 0.2 about seeded axes",
     lambda rng: np.concatenate([t * so3_axes(rng) for t in (1e-9, 1e-6, 1e-3, 0.05, 0.1, 0.19, 0.1999)]))
_add("so3_above_seam", "SO3", 47, "the closed-form side from the seam up: angles 0.2001 .. 0.64, where e = (1 - a) / t^2 cancels most",
     lambda rng: np.concatenate([t * so3_axes(rng) for t in np.linspace(0.2001, 0.64, 30)]))
_add("so3_zero", "SO3", 46, "w = 0 exactly: the documented limit R = J_l = I", lambda rng: np.zeros((1, 3)), identity=True)


# ---- HUBER_SW -------------------------------------------------------------------------------------------------------------
def _huber_edge(k):
    return lambda rng: np.array([(float(step(d * d, k)), d) for d in HUBER_DELTAS])


def _huber_log(rng):
    rows = []
    for d in HUBER_DELTAS:
        s = d * d * np.concatenate([10.0 ** rng.uniform(0, 12, 700), 1 + 10.0 ** rng.uniform(-15, 0, 200)])
        s = np.minimum(s[s > d * d], step(1e12 * d * d, -1))
        rows.append(np.stack([s, np.full(s.size, d)], 1))
    return np.concatenate(rows)


_add("huber_edge_0", "HUBER_SW", 51, "s = delta^2 exactly: an inlier", _huber_edge(0), exact_one=True, outside=True)
_add("huber_edge_1", "HUBER_SW", 52, "s = delta^2 (1 + 1 ulp): the first outlier", _huber_edge(1))
_add("huber_edge_2", "HUBER_SW", 53, "s = delta^2 (1 + 2 ulp)", _huber_edge(2))
_add("huber_log", "HUBER_SW", 54, "log-spaced s up to 1e12 delta^2 and s / delta^2 - 1 down to 1e-15: the two chained roots", _huber_log)
_add("huber_off", "HUBER_SW", 55, "delta = 0 and delta < 0: no robust loss",
     lambda rng: np.array([(s, d) for s in (0.0, 0.5, 4.0, 1e9) for d in (0.0, -0.0, -1.0, -0.25)]), exact_one=True, outside=True)
