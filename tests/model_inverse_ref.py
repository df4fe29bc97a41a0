"""The yardstick for the two model inverses of the device (TEST INFRASTRUCTURE): unproject_ray (csrc/ccal_model_inverse.hpp) and
unproject_normalized (csrc/ccal_pose_init.hpp), and for `project`.  mpmath at 50 digits and more (DPS); the models are restated from their
definitions, the device's iterations are not:

    UCM / EUCM   m = (u - c) / f, r2 = |m|^2, t1 = 1 - (2 alpha - 1) beta r2,
                 mz = (1 - beta alpha^2 r2) / (alpha sqrt t1 + 1 - alpha), ray = (mx, my, mz) / |.|          (Usenko et al. 2018)
                 domain: alpha <= 1/2 everything, else r2 <= 1 / (beta (2 alpha - 1))
    KB4          the roots of theta P(theta^2) - r in (0, pi), P = 1 + k1 s + k2 s^2 + k3 s^3 + k4 s^4, from mpmath.polyroots
    OPENCV5      the published fixed point (x, y) <- ((mx, my) - tangential(x, y)) / radial(x, y), replayed at 50 digits, then
                 polished by Newton's method on distort(x, y) = (mx, my)

Every pixel row gets a CLASS from this file alone (classify):

    A     the inverse exists, is well conditioned and the published iteration reaches it with room to spare: the device must
          return it
    B     no ray exists: the device must return None
    near  UCM / EUCM: within BOUNDARY_REL of the domain's limit; either answer is right
    C     everything else: only soundness is asked (a valid row re-projects onto its pixel)

KB4: A = the smallest root theta* in (0, pi) exists, fp = d(theta P)/d theta > FP_MIN on [0, theta*], and Newton's method from t = r
at 50 digits is at theta* after `newton_steps` steps: 12 for unproject_ray, 8 under its 20; 8 for unproject_normalized, 2 under its
10 (the same reasoning - the device must not need its last steps - for a loop half as long).  B = min over (0, pi) of
|theta P - r| > B_MIN.  For the normalised inverse A also needs theta* < 1.5 - 1e-6 and B also holds the rows whose every root is
> 1.5 + 1e-6.  OPENCV5: A = the fixed point's residual |ex| + |ey| is < 1e-12 at step `fixed_steps`: 40 for unproject_ray (of its
50), 20 for unproject_normalized (of its 25); no B.  UCM / EUCM, normalised inverse: the device also refuses mz <= 1e-3 (not in
front of the camera): A needs mz > 1e-3 (1 + 1e-9), rows with mz < 1e-3 (1 - 1e-9) are B, between them `near`.

Inputs are doubles and are taken exactly."""
from dataclasses import dataclass

import mpmath as mp
import numpy as np

UCM, EUCM, KB4, OPENCV5 = 0, 1, 2, 3
DPS = 70                                # 50 digits are asked of the yardstick; 20 more carry the cancellation of the round trip through a
                                        # unit ray at alpha -> 1/2 (13 digits at the limit rows of alpha = 1/2 + 2^-30) down to 1e-40 px
BOUNDARY_REL = 1e-12                    # the suite's `near` convention (tests/undistort_ref.py)
SMALL_RADIUS = 1e-8
FP_MIN = 0.05
B_MIN = 1e-6
FRONT_T = 1.5                           # unproject_normalized's KB4 limit on theta
FRONT_K = 1e-3                          # and its UCM / EUCM limit on mz
U = 2.0 ** -53


def _f(x):
    return mp.mpf(float(x))


def _params(p):
    return [_f(v) for v in np.asarray(p, dtype=np.float64)]


# ---- project ----------------------------------------------------------------------------------------------------------------------
def project_mp(model, p, xyz):
    """GenericModel::project of camera-frame points xyz [n, 3] (doubles): (uv, valid, near).  uv: a list of (u, v) mpf pairs, None
    where project is undefined; valid, near: bool arrays, near = within BOUNDARY_REL of the validity boundary."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    uv, valid, near = [None] * n, np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    with mp.workdps(DPS):
        q = _params(p)
        fx, fy, cx, cy = q[:4]
        for i in range(n):
            if not np.isfinite(xyz[i]).all():
                continue
            x, y, z = (_f(v) for v in xyz[i])
            r2 = x * x + y * y
            if model in (UCM, EUCM):
                alpha, beta = q[4], (q[5] if model == EUCM else mp.mpf(1))
                d = mp.sqrt(beta * r2 + z * z)
                w = alpha / (1 - alpha) if alpha <= mp.mpf(0.5) else (1 - alpha) / alpha
                margin = z + w * d
                valid[i] = margin > 0
                near[i] = abs(margin) <= BOUNDARY_REL * max(d, abs(z))
                if valid[i]:
                    nrm = alpha * d + (1 - alpha) * z
                    uv[i] = (fx * (x / nrm) + cx, fy * (y / nrm) + cy)
            elif model == KB4:
                valid[i] = r2 + z * z > 0
                if valid[i]:
                    r = mp.sqrt(r2)
                    if r > SMALL_RADIUS:
                        t = mp.atan2(r, z)
                        td = _kb4_g(q[4:8], t)
                        uv[i] = (fx * (td * x / r) + cx, fy * (td * y / r) + cy)
                    else:
                        uv[i] = (fx * (x / z) + cx, fy * (y / z) + cy)
            else:
                valid[i] = z > mp.mpf(1e-9)
                near[i] = abs(z - mp.mpf(1e-9)) <= BOUNDARY_REL * 1e-9
                if valid[i]:
                    mx, my = _ocv5_forward(q[4:9], x / z, y / z)
                    uv[i] = (fx * mx + cx, fy * my + cy)
    return uv, valid, near


def _kb4_g(k, t):
    s = t * t
    return t * (1 + s * (k[0] + s * (k[1] + s * (k[2] + s * k[3]))))


def _kb4_gp(k, t):
    s = t * t
    return 1 + s * (3 * k[0] + s * (5 * k[1] + s * (7 * k[2] + s * 9 * k[3])))


def _ocv5_forward(d, x, y):
    k1, k2, p1, p2, k3 = d
    q = x * x + y * y
    rad = 1 + q * (k1 + q * (k2 + q * k3))
    return (x * rad + 2 * p1 * x * y + p2 * (q + 2 * x * x), y * rad + p1 * (q + 2 * y * y) + 2 * p2 * x * y)


# ---- unproject ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Row:
    cls: str                            # "A", "B", "C" or "near"
    xy: tuple = None                    # A rows: the normalised image point (x / z, y / z) of the ray, mpf (None where z <= 0)
    ray: tuple = None                   # A rows: the unit ray, mpf (KB4 below the small radius: (mx, my, 1), not normalised)
    theta: object = None                # KB4 A rows: theta*
    small: bool = False                 # KB4: below the small radius
    bound: float = 0.0                  # UCM / EUCM A rows: the derived bound on the device's ray / normalised point (module docstring
                                        # of tests/test_gpu_model_inverse.py)
    principal: bool = False             # KB4 C rows: a principal root exists with fp > FP_MIN on [0, theta*]


def _real_roots(coeffs, lo, hi):
    """the real roots of the polynomial (highest power first) in the open interval (lo, hi), ascending"""
    c = list(coeffs)
    while c and c[0] == 0:
        c.pop(0)
    if len(c) < 2:
        return []
    # numpy's f64 roots as the start of mpmath's iteration: the same roots to the working precision in a quarter of the steps
    init = [mp.mpc(complex(z)) for z in np.roots([float(v) for v in c])]
    roots = mp.polyroots(c, maxsteps=2000, extraprec=400, roots_init=init if len(init) == len(c) - 1 else None)
    out = [mp.re(z) for z in roots if abs(mp.im(z)) <= mp.mpf(10) ** -30 * (1 + abs(mp.re(z)))]
    return sorted(t for t in out if lo < t < hi)


class Kb4Set:
    """what the rows of one KB4 parameter set share: the critical points of g = theta P(theta^2) in (0, pi), the first theta at
    which g' comes down to FP_MIN, and the fold (the first local maximum r_c = g(theta_c), None for a monotone g)"""

    def __init__(self, p):
        with mp.workdps(DPS):
            self.k = _params(p)[4:8]
            k = self.k
            crit_s = _real_roots([9 * k[3], 7 * k[2], 5 * k[1], 3 * k[0], mp.mpf(1)], 0, mp.pi ** 2)
            self.crit = [mp.sqrt(s) for s in crit_s]
            s05 = _real_roots([9 * k[3], 7 * k[2], 5 * k[1], 3 * k[0], mp.mpf(1) - FP_MIN], 0, mp.inf)
            self.t_fp = mp.sqrt(s05[0]) if s05 else mp.inf
            self.fold = (self.crit[0], _kb4_g(k, self.crit[0])) if self.crit else None
        self._roots = {}

    def roots(self, r):
        if r not in self._roots:
            self._roots[r] = self._polyroots(r)
        return self._roots[r]

    def _polyroots(self, r):
        k = self.k
        return _real_roots([k[3], 0, k[2], 0, k[1], 0, k[0], 0, mp.mpf(1), -r], 0, mp.pi)

    def min_abs(self, r, hi=None):
        """min over (0, hi) of |g - r| when g - r has no root there: at a critical point or an end"""
        hi = mp.pi if hi is None else hi
        pts = [t for t in self.crit if t < hi] + [mp.mpf(0), hi]
        return min(abs(_kb4_g(self.k, t) - r) for t in pts)


_KB4_SETS: dict = {}


def kb4_set(p):
    """the Kb4Set of a parameter vector, made once per process (it keeps the roots of its rows)"""
    key = tuple(float(v) for v in np.asarray(p, dtype=np.float64))
    if key not in _KB4_SETS:
        _KB4_SETS[key] = Kb4Set(p)
    return _KB4_SETS[key]


def _classify_kb4(ks, mx, my, normalized, newton_steps):
    k = ks.k
    r = mp.sqrt(mx * mx + my * my)
    if r < SMALL_RADIUS:
        return Row("A", xy=(mx, my), ray=(mx, my, mp.mpf(1)), theta=r, small=True)
    roots = ks.roots(r)
    if not roots:
        return Row("B" if ks.min_abs(r) > B_MIN else "C")
    if normalized and all(t > FRONT_T + 1e-6 for t in roots):
        return Row("B")
    t_star = roots[0]
    for _ in range(2 if t_star < ks.t_fp else 0):               # polyroots' root, polished at the working precision (fp > FP_MIN)
        t_star = t_star - (_kb4_g(k, t_star) - r) / _kb4_gp(k, t_star)
    principal = t_star < ks.t_fp
    ok = principal and (not normalized or t_star < FRONT_T - 1e-6)
    if ok:
        t = r
        for _ in range(newton_steps):
            fp = _kb4_gp(k, t)
            if fp == 0:
                ok = False
                break
            t = t - (_kb4_g(k, t) - r) / fp
        ok = ok and abs(t - t_star) < mp.mpf(10) ** -15
    if not ok:
        return Row("C", principal=principal and (not normalized or t_star < FRONT_T - 1e-6))
    s, c = mp.sin(t_star), mp.cos(t_star)
    xy = (mx * (s / c) / r, my * (s / c) / r) if c > 0 else None
    return Row("A", xy=xy, ray=(mx * s / r, my * s / r, c), theta=t_star)


def _classify_ocv5(d, mx, my, fixed_steps):
    k1, k2, p1, p2, k3 = d
    x, y = mx, my
    for _ in range(fixed_steps):
        q = x * x + y * y
        rad = 1 + q * (k1 + q * (k2 + q * k3))
        if rad == 0:
            return Row("C")
        dx = 2 * p1 * x * y + p2 * (q + 2 * x * x)
        dy = p1 * (q + 2 * y * y) + 2 * p2 * x * y
        x, y = (mx - dx) / rad, (my - dy) / rad
        if abs(x) + abs(y) > 1e30:
            return Row("C")
    fx, fy = _ocv5_forward(d, x, y)
    if not abs(fx - mx) + abs(fy - my) < mp.mpf(10) ** -12:
        return Row("C")
    x0, y0 = x, y
    for _ in range(8):                                          # Newton on distort(x, y) = (mx, my) from the accepted iterate
        fx, fy = _ocv5_forward(d, x, y)
        ex, ey = fx - mx, fy - my
        q = x * x + y * y
        rad = 1 + q * (k1 + q * (k2 + q * k3))
        dr = k1 + q * (2 * k2 + q * 3 * k3)
        a = rad + 2 * x * x * dr + 2 * p1 * y + 6 * p2 * x
        b = 2 * x * y * dr + 2 * p1 * x + 2 * p2 * y
        e = rad + 2 * y * y * dr + 6 * p1 * y + 2 * p2 * x
        det = a * e - b * b
        if det == 0:
            return Row("C")
        x, y = x - (e * ex - b * ey) / det, y - (a * ey - b * ex) / det
    fx, fy = _ocv5_forward(d, x, y)
    if not (abs(fx - mx) + abs(fy - my) < mp.mpf(10) ** -45 and abs(x - x0) + abs(y - y0) < mp.mpf(10) ** -9):
        return Row("C")
    nrm = mp.sqrt(x * x + y * y + 1)
    return Row("A", xy=(x, y), ray=(x / nrm, y / nrm, 1 / nrm))


def _classify_ucm(alpha, beta, mx, my, normalized):
    r2 = mx * mx + my * my
    c = (2 * alpha - 1) * beta
    if alpha > mp.mpf(0.5):
        lim = 1 / c
        if abs(r2 - lim) <= BOUNDARY_REL * lim:
            return Row("near")
        if r2 > lim:
            return Row("B")
    t1 = 1 - c * r2
    s = mp.sqrt(t1)
    den = alpha * s + (1 - alpha)
    num = 1 - beta * alpha * alpha * r2
    mz = num / den
    if normalized:
        if abs(mz - FRONT_K) <= mp.mpf(1e-9) * FRONT_K:
            return Row("near")
        if mz < FRONT_K:
            return Row("B")
    nrm = mp.sqrt(r2 + mz * mz)
    # the derived bound (the docstring of tests/test_gpu_model_inverse.py): absolute errors in f64, u = 2^-53, rounded-up counts
    u = mp.mpf(U)
    r = mp.sqrt(r2)
    d_t1 = 10 * u * abs(c) * r2 + u * t1
    d_s = d_t1 / (2 * s) + 2 * u * s                             # the conditioning 1 / sqrt t1
    d_den = alpha * d_s + 3 * u * den
    d_num = 10 * u * beta * alpha * alpha * r2 + u * abs(num)
    d_mz = d_num / den + abs(num) * d_den / (den * den) + 2 * u * abs(mz)
    if normalized:
        bound = (r / mz) * (d_mz / mz + 4 * u)
    else:
        bound = 2 * d_mz / nrm + 3 * u * r / nrm + 8 * u
    xy = (mx / mz, my / mz) if mz > 0 else None
    return Row("A", xy=xy, ray=(mx / nrm, my / nrm, mz / nrm), bound=float(bound))


def classify(model, p, uv, normalized=False):
    """one Row per pixel of uv [n, 2] (doubles) for unproject_ray (normalized False) or unproject_normalized (True)"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    rows = []
    with mp.workdps(DPS):
        q = _params(p)
        ks = kb4_set(p) if model == KB4 else None
        for u, v in uv:
            mx, my = (_f(u) - q[2]) / q[0], (_f(v) - q[3]) / q[1]
            if model in (UCM, EUCM):
                rows.append(_classify_ucm(q[4], q[5] if model == EUCM else mp.mpf(1), mx, my, normalized))
            elif model == KB4:
                rows.append(_classify_kb4(ks, mx, my, normalized, 8 if normalized else 12))
            else:
                rows.append(_classify_ocv5(q[4:9], mx, my, 20 if normalized else 40))
    return rows


def pixel_error(uv_mp, pixel):
    """max(|du|, |dv|) in pixels between an mpf pair and a pixel of doubles, as a float"""
    with mp.workdps(DPS):
        return float(max(abs(uv_mp[0] - _f(pixel[0])), abs(uv_mp[1] - _f(pixel[1]))))


def vec_error(got, want):
    """the largest component difference between doubles and mpf values, as a float; inf for a non-finite component"""
    if not np.isfinite(np.asarray(got, dtype=np.float64)).all():
        return float("inf")
    with mp.workdps(DPS):
        return float(max(abs(_f(g) - w) for g, w in zip(got, want)))
