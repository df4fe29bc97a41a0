"""The two small dense solves at the end of every step, in mpmath at 50 digits (TEST INFRASTRUCTURE, not collected): exactly what
the comments above k_solve, k_backsub (csrc/ccal_kernels_normal.hip) and head_wave (csrc/ccal_head.hpp) state.

The system of a camera solve, column by column:
    a fixed column            identity row and column, right-hand side 0
    otherwise                 S_ii += lambda * clamp(hdiag_i, min_diag, max_diag) when lambda > 0
    k_head                    S = A_dir - Y^T Y, the damping is read from A_dir's diagonal, b_i = A_dir[i][K] - Y^T Y[i][K]
and its results:
    dc   = S^-1 (-b)
    cand = clamp(x + dc) where bounded
    mc   = sum over the free columns of d (D_ii d - g_i), g_i = gc_i (k_solve) or A_dir[i][K] (k_head)
The pose back-substitution of one slot, from its record L (21, row-major lower, diagonal stored INVERTED) | Y [6][K + 1] | g_p | dC:
    dp = -L^-T (y_r + Y dc),  mc = sum dp (lambda clamp(dC) dp - g_p);  R[0] == 0: the slot keeps its pose, mc 0

truth()      dc by mpmath.cholesky_solve up to K = ROUTE_K, beyond it by refinement of an f64 solve with mpmath residuals until the
             scaled residual is below 1e-40 (the residuals in exact integer arithmetic on the mpf values: K = 127 in a fraction of
             the time); tests/test_camera_solve_cpu.py holds the two routes against each other.
yardstick()  the same algorithm in f64: a plain row-oriented Cholesky written out in numpy with IEEE sqrt and division, no library
             solve - in four operation orders (ORDERS).  Its distance from truth() is what the device's is compared with.
dc_error()   max_i |d dc_i| sqrt(S_ii) / max_i |dc*_i| sqrt(S_ii): Cholesky is invariant under diagonal scaling and camera systems are
             scaled over seven decades - an unscaled norm would let the focal columns hide the distortion columns.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

mp.mp.dps = 50
ROUTE_K = 40
RESIDUAL_GOAL = mp.mpf(10) ** -40

COL_DTYPE = np.dtype([("lo", "f8"), ("hi", "f8"), ("has_bound", "i4"), ("fixed", "i4"), ("is_extr", "i4"), ("dst", "i4"), ("dst2", "i4"),
                      ("pad_", "i4")])             # csrc/ccal_normal.hpp: ColInfo (40 bytes)
KMAX = 128                                          # include/ccal.h: CCAL_KMAX
PMAX = 10                                           # CCAL_PMAX


def red_size(K):
    return (K + 1) * (K + 1) + 2 * K + 3


def fused_red_size(K):
    return 2 * (K + 1) * (K + 1) + 2


def pf_size(K):
    return (21 + 6 * (K + 1) + 12 + 1) & ~1


def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


# ---- the system, from the form's own layout (f64 inputs, exact in whatever `num` is: mp.mpf or float)
def system(case, num=mp.mpf):
    """(S [K][K] full symmetric, rhs [K], Dii [K], g [K]) of the damped, masked system; `num` converts an input value"""
    K, K1 = case.K, case.K + 1
    red = case.red
    fixed = case.cols["fixed"] != 0
    S = [[None] * K for _ in range(K)]
    rhs, Dii, g = [None] * K, [None] * K, [None] * K
    zero, one = num(0.0), num(1.0)
    for i in range(K):
        if case.form == "k_solve":
            hd, b, g[i] = num(red[K1 * K1 + i]), num(red[K * K1 + i]), num(red[K1 * K1 + K + i])
        else:
            hd, b, g[i] = num(red[i * K1 + i]), num(red[i * K1 + K]) - num(red[K1 * K1 + i * K1 + K]), num(red[i * K1 + K])
        Dii[i] = num(case.lam) * _clamp(hd, num(case.min_diag), num(case.max_diag)) if case.lam > 0 else zero
        rhs[i] = zero if fixed[i] else -b
        for j in range(i + 1):
            if fixed[i] or fixed[j]:
                v = one if i == j else zero
            else:
                v = num(red[i * K1 + j]) if case.form == "k_solve" else num(red[i * K1 + j]) - num(red[K1 * K1 + i * K1 + j])
                if i == j:
                    v = v + Dii[i]
            S[i][j] = S[j][i] = v
    return S, rhs, Dii, g


def _f64_matrix(S):
    return np.array([[float(v) for v in row] for row in S], dtype=np.float64)


# ---- the f64 yardstick: row-oriented Cholesky, forward and back substitution; None with the failing column when a pivot is not positive
def cholesky_f64(S):
    K = len(S)
    L = np.zeros((K, K))
    for j in range(K):
        t = S[j:, j] - (L[j:, :j] * L[j, :j]).sum(axis=1)
        if not (t[0] > 0.0) or not (t[0] < 1.7e308):
            return None, j
        d = np.sqrt(t[0])
        L[j, j] = d
        L[j + 1:, j] = t[1:] / d
    return L, -1


def solve_f64(L, rhs):
    K = len(rhs)
    y = np.zeros(K)
    for i in range(K):
        y[i] = (rhs[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(K)
    for i in range(K - 1, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


def cholesky_f64_right(S):
    """the right-looking form: column j, then the trailing block minus its outer product - every entry's sum in the order k = 0, 1, ..."""
    K = len(S)
    A, L = np.array(S, dtype=np.float64), np.zeros((K, K))
    for j in range(K):
        if not (A[j, j] > 0.0) or not (A[j, j] < 1.7e308):
            return None, j
        d = np.sqrt(A[j, j])
        L[j, j] = d
        L[j + 1:, j] = A[j + 1:, j] / d
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L, -1


def cholesky_f64_reversed_sums(S):
    """the row-oriented form with every sum taken from k = j - 1 down"""
    K = len(S)
    L = np.zeros((K, K))
    for j in range(K):
        t = S[j:, j] - (L[j:, :j][:, ::-1] * L[j, :j][::-1]).sum(axis=1)
        if not (t[0] > 0.0) or not (t[0] < 1.7e308):
            return None, j
        d = np.sqrt(t[0])
        L[j, j] = d
        L[j + 1:, j] = t[1:] / d
    return L, -1


ORDERS = 4          # 0 row-oriented | 1 right-looking | 2 right-looking on the columns in reverse order | 3 row-oriented, sums reversed


def yardstick(case, order=0):
    """dict(dc, mc) in f64, or dict(failed_at=j) (order 0).  The four orders are the same algorithm with its roundings elsewhere: on an
    ill-conditioned system the error of ONE order is one draw of a quantity whose size is (rounding noise along the weakest
    direction) / (smallest eigenvalue) - it can come out ten times under its typical size; the worst of four does not."""
    S, rhs, Dii, g = system(case, num=float)
    S, rhs, Dii, g = np.array(S), np.array(rhs), np.array(Dii), np.array(g)
    if order == 2:
        L, bad = cholesky_f64_right(S[::-1, ::-1])
        dc = None if L is None else solve_f64(L, rhs[::-1])[::-1]
    else:
        L, bad = (cholesky_f64, cholesky_f64_right, None, cholesky_f64_reversed_sums)[order](S)
        dc = None if L is None else solve_f64(L, rhs)
    if L is None:
        return {"failed_at": bad}
    free = case.cols["fixed"] == 0
    return {"dc": dc, "mc": float((dc[free] * (Dii[free] * dc[free] - g[free])).sum())}


# ---- the truth
def solve_cholesky_mp(S, rhs):
    return [v for v in mp.cholesky_solve(mp.matrix(S), mp.matrix(rhs))]


class _Exact:
    """The system as integers over a common power of two (every mpf is man * 2^exp: no rounding), so that a residual is K^2 integer
    products - a tenth of the time of mpmath dot products, and exact for the x it is given (x itself is cut at 2^-XBITS of its
    largest component: 60 digits)."""
    XBITS = 200

    def __init__(self, S, rhs):
        K = self.K = len(rhs)
        vals = [v for row in S for v in row] + list(rhs)
        shift = self.shift = -min(v._mpf_[2] for v in vals if v._mpf_[1])       # _mpf_ = (sign, man, exp, bitcount)

        def to_int(v):
            sign, man, exp, _ = v._mpf_
            return (-man if sign else man) << (exp + shift) if man else 0
        self.S = [[to_int(v) for v in row] for row in S]
        self.rhs = [to_int(v) for v in rhs]
        self.sd = [mp.sqrt(S[i][i]) for i in range(K)]

    def residual(self, x):
        """rhs - S x, exactly, as mpf"""
        top = max(abs(v) for v in x)
        P = self.XBITS - (int(mp.floor(mp.log(top, 2))) if top else 0)
        X = [int(mp.floor(mp.ldexp(v, P) + mp.mpf(0.5))) for v in x]
        return [mp.ldexp(mp.mpf((b << P) - sum(map(int.__mul__, row, X))), -(P + self.shift)) for row, b in zip(self.S, self.rhs)]

    def scaled(self, r, x):
        """max_i |r_i| / sqrt(S_ii)  over  max_i |x_i| sqrt(S_ii)"""
        top = max(abs(r[i]) / self.sd[i] for i in range(self.K))
        bot = max(abs(x[i]) * self.sd[i] for i in range(self.K))
        return top / bot if bot else top


def scaled_residual(S, rhs, x):
    ex = _Exact(S, rhs)
    return ex.scaled(ex.residual(x), x)


def solve_refined(S, rhs, max_rounds=40):
    """an f64 Cholesky solve of the rounded system, refined with residuals of the exact one"""
    K = len(rhs)
    L, bad = cholesky_f64(_f64_matrix(S))
    assert L is not None, bad
    ex = _Exact(S, rhs)
    x = [mp.mpf(0)] * K
    for _ in range(max_rounds):
        r = ex.residual(x)
        res = ex.scaled(r, x)
        if res < RESIDUAL_GOAL:
            return x
        top = max(abs(v) for v in r)                 # (the f64 corrector sees the residual at unit scale: no underflow far down)
        d = solve_f64(L, np.array([float(v / top) for v in r]))
        x = [xi + top * mp.mpf(float(di)) for xi, di in zip(x, d)]
    raise AssertionError(f"refinement stalled at a scaled residual of {mp.nstr(res, 3)}")


def truth(case, route=None):
    """dict(dc [K] mpf, mc mpf, cand [K] f64 values after the clamp, clamped [K] in {-1, 0, +1}, sdiag [K] mpf = sqrt(S_ii))"""
    S, rhs, Dii, g = system(case)
    route = route or ("cholesky" if case.K <= ROUTE_K else "refined")
    dc = solve_cholesky_mp(S, rhs) if route == "cholesky" else solve_refined(S, rhs)
    cols = case.cols
    mc = mp.fsum(dc[i] * (Dii[i] * dc[i] - g[i]) for i in range(case.K) if not cols["fixed"][i])
    cand, clamped = [], []
    for i in range(case.K):
        x = mp.mpf(float((case.extr if cols["is_extr"][i] else case.intr)[cols["dst"][i]]))
        v = x + dc[i]
        c = 0
        if cols["has_bound"][i] and not cols["fixed"][i]:
            c = -1 if v < mp.mpf(float(cols["lo"][i])) else (1 if v > mp.mpf(float(cols["hi"][i])) else 0)
        cand.append(v)
        clamped.append(c)
    return {"dc": dc, "mc": mc, "cand": cand, "clamped": clamped, "sdiag": [mp.sqrt(S[i][i]) for i in range(case.K)]}


def dc_error(dc, tr):
    """the scaled error of an f64 step against truth()"""
    K = len(tr["dc"])
    top = max(abs(mp.mpf(float(dc[i])) - tr["dc"][i]) * tr["sdiag"][i] for i in range(K))
    bot = max(abs(tr["dc"][i]) * tr["sdiag"][i] for i in range(K))
    return float(top / bot) if bot else float(top)


def rel_error(got, want):
    got, want = mp.mpf(float(got)), mp.mpf(want)
    return float(abs(got - want) / abs(want)) if want else float(abs(got))


# ---- the pose back-substitution of one slot
def _backsub(rec, dc, K, lam, min_diag, max_diag, num):
    K1 = K + 1
    if rec[0] == 0.0:
        return None
    L = [[num(rec[i * (i + 1) // 2 + j]) for j in range(i + 1)] for i in range(6)]
    rhs = []
    for r in range(6):
        y = rec[21 + r * K1: 21 + (r + 1) * K1]
        t = num(y[K])
        for j in range(K):
            t = t + num(y[j]) * dc[j]
        rhs.append(-t)
    dp = [None] * 6
    for i in range(5, -1, -1):                       # L^T x = rhs, the stored diagonal is 1 / L_ii
        t = rhs[i]
        for k in range(i + 1, 6):
            t = t - L[k][i] * dp[k]
        dp[i] = t * L[i][i]
    mc = num(0.0)
    for i in range(6):
        gp, dC = num(rec[21 + 6 * K1 + i]), num(rec[21 + 6 * K1 + 6 + i])
        Dii = num(lam) * _clamp(dC, num(min_diag), num(max_diag)) if lam > 0 else num(0.0)
        mc = mc + dp[i] * (Dii * dp[i] - gp)
    return dp, mc


def backsub_truth(case):
    """per slot: (dp [6] mpf, mc mpf), or None where the slot keeps its pose"""
    dc = [mp.mpf(float(v)) for v in case.dc]
    return [_backsub(rec, dc, case.K, case.lam, case.min_diag, case.max_diag, mp.mpf) for rec in case.pf]


def backsub_yardstick(case):
    """per slot: (fl(pose + dp) [6], mc) in f64, or None"""
    out = []
    for rec, pose in zip(case.pf, case.poses):
        r = _backsub(rec, [float(v) for v in case.dc], case.K, case.lam, case.min_diag, case.max_diag, float)
        out.append(None if r is None else (pose + np.array(r[0]), float(r[1])))
    return out


def pose_error(cand, pose, want_dp):
    """max_i |cand_i - (pose_i + dp*_i)| over max_i |dp*_i|: the candidate pose is what the kernel writes, so the rounding of its
    addition is part of the measure - of the yardstick's as well"""
    top = max(abs(mp.mpf(float(cand[i])) - (mp.mpf(float(pose[i])) + want_dp[i])) for i in range(6))
    return float(top / max(abs(w) for w in want_dp))
