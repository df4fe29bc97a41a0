"""The yardstick of the planar pose initialiser (k_pose_init, csrc/ccal_kernels_init.hip): a plain numpy restatement, no GPU.

It works from the f32-rounded board points and detections the library receives and otherwise computes in np.longdouble:
  unproject    the published inverse of each model, iterated to convergence (the kernel: 10 Newton / 25 fixed-point steps)
  solve        the same least-squares problem for h11 .. h32 (h33 = 1), by Householder QR of the design instead of normal
               equations, then the kernel's own post-processing (pose_from_h); returns R, t and two diagnostics, kappa and min_rel_pivot
  frame_pose   unproject + the kernel's rules for "no pose" (too few valid corners, rank-deficient by PIVOT_TOL) + solve
emulate_f64 is NOT a yardstick: it is the kernel's arithmetic (lane-private sums, butterfly reduction, normal equations, Cholesky,
matrix -> quaternion -> rvec) in f64 numpy, the instrument that sizes the tolerance factor of tests/test_gpu_pose_init.py and shows
which quaternion branch a frame takes."""
import numpy as np

LD = np.longdouble
U_LD = float(np.finfo(LD).eps) / 2.0
U_F64 = 2.0 ** -53

UCM, EUCM, KB4, OPENCV5, DIVISION = 0, 1, 2, 3, 100
NPARAMS = {UCM: 5, EUCM: 6, KB4: 8, OPENCV5: 9, DIVISION: 5}

# The kernel's rule for a frame whose corners do not span the board plane: a Cholesky pivot s of the 8 x 8 normal matrix must
# exceed PIVOT_TOL x its own diagonal entry M_jj.  Between 100 x the pivot's rounding floor (10 u = 1.1e-15) and 1 / 100 of the
# smallest pivot of a well-posed frame of tests/pose_init_cases.py (2.7e-6: the board whose origin is 100 m away).
PIVOT_TOL = 2.0 ** -36

try:
    import mpmath as _mp
except Exception:                                            # the 50-digit cross-checks are left out, nothing else
    _mp = None


def have_mpmath():
    return _mp is not None


def division_theta(width, height, lam):
    """th of the division model of init_pose: [half, half, w / 2, h / 2, lambda]."""
    hw, hh = 0.5 * width, 0.5 * height
    half = max(hw, hh)
    return np.array([half, half, hw, hh, lam], dtype=np.float64)


# ---- unprojection ----------------------------------------------------------------------------------------------------------------
def _ocv5_forward(x, y, k1, k2, p1, p2, k3):
    q = x * x + y * y
    rad = 1 + q * (k1 + q * (k2 + q * k3))
    return (x * rad + 2 * p1 * x * y + p2 * (q + 2 * x * x), y * rad + p1 * (q + 2 * y * y) + 2 * p2 * x * y)


def unproject(model, params, uv, unproject_eps=1e-8):
    """(xn, yn, valid) of detections uv [n, 2] (pixels): the normalised image points in long double, and which of them the model
    can unproject (the rules of unproject_normalized, csrc/ccal_pose_init.hpp).  Rows that are not valid hold NaN."""
    th = np.asarray(params, dtype=np.float64).astype(LD)
    uv = np.asarray(uv).astype(LD).reshape(-1, 2)
    mx, my = (uv[:, 0] - th[2]) / th[0], (uv[:, 1] - th[3]) / th[1]
    r2 = mx * mx + my * my
    n = len(mx)
    xn, yn, valid = np.full(n, np.nan, dtype=LD), np.full(n, np.nan, dtype=LD), np.zeros(n, dtype=bool)
    one = LD(1)
    if model == DIVISION:
        sc = one + th[4] * r2
        valid = sc > 1e-9
        xn[valid], yn[valid] = (mx / sc)[valid], (my / sc)[valid]
    elif model in (UCM, EUCM):
        alpha, beta = th[4], (th[5] if model == EUCM else one)
        valid = np.ones(n, dtype=bool)
        if alpha > 0.5:
            valid &= ~(r2 > one / (beta * (2 * alpha - one)))
        t1 = one - (2 * alpha - one) * beta * r2
        valid &= ~(t1 < 0)
        k = (one - alpha * alpha * beta * r2) / (alpha * np.sqrt(np.where(valid, t1, one)) + (one - alpha))
        valid &= k > 1e-3
        xn[valid], yn[valid] = (mx / k)[valid], (my / k)[valid]
    elif model == KB4:
        r = np.sqrt(r2)
        for i in range(n):
            if r[i] < unproject_eps:
                xn[i], yn[i], valid[i] = mx[i], my[i], True
                continue
            t = r[i]
            for _ in range(100):                                 # Newton on theta d(theta) = r, to a stalled step
                t2 = t * t
                f = t * (one + t2 * (th[4] + t2 * (th[5] + t2 * (th[6] + t2 * th[7])))) - r[i]
                fp = one + t2 * (3 * th[4] + t2 * (5 * th[5] + t2 * (7 * th[6] + t2 * 9 * th[7])))
                step = f / fp
                t = t - step
                if not abs(step) > 4 * U_LD * abs(t):
                    break
            if not (t > 0) or not (t < 1.5):
                continue
            tt = t * t
            if not abs(t * (one + tt * (th[4] + tt * (th[5] + tt * (th[6] + tt * th[7])))) - r[i]) < 1e-9:   # the kernel's acceptance rule
                continue
            s = np.tan(t) / r[i]
            xn[i], yn[i], valid[i] = mx[i] * s, my[i] * s, True
    elif model == OPENCV5:
        k1, k2, p1, p2, k3 = th[4:9]
        for i in range(n):
            x, y = mx[i], my[i]
            for _ in range(25):                                  # the published fixed point as the start ...
                q = x * x + y * y
                rad = one + q * (k1 + q * (k2 + q * k3))
                dx = 2 * p1 * x * y + p2 * (q + 2 * x * x)
                dy = p1 * (q + 2 * y * y) + 2 * p2 * x * y
                x, y = (mx[i] - dx) / rad, (my[i] - dy) / rad
            for _ in range(50):                                  # ... then Newton on distort(x, y) = (mx, my), to a stalled step
                fx, fy = _ocv5_forward(x, y, k1, k2, p1, p2, k3)
                ex, ey = fx - mx[i], fy - my[i]
                q = x * x + y * y
                rad = one + q * (k1 + q * (k2 + q * k3))
                dr = k1 + q * (2 * k2 + q * 3 * k3)              # d rad / d q
                a = rad + 2 * x * x * dr + 2 * p1 * y + 6 * p2 * x
                b = 2 * x * y * dr + 2 * p1 * x + 2 * p2 * y
                d = rad + 2 * y * y * dr + 6 * p1 * y + 2 * p2 * x
                det = a * d - b * b
                sx, sy = (d * ex - b * ey) / det, (a * ey - b * ex) / det
                x, y = x - sx, y - sy
                if not abs(sx) + abs(sy) > 4 * U_LD * (abs(x) + abs(y) + U_LD):
                    break
            fx, fy = _ocv5_forward(x, y, k1, k2, p1, p2, k3)
            if not (abs(fx - mx[i]) + abs(fy - my[i]) < 1e-9):   # the kernel's acceptance rule
                continue
            xn[i], yn[i], valid[i] = x, y, True
    else:
        raise ValueError(f"unknown model {model}")
    return xn, yn, valid


def unproject_kernel_f64(model, params, uv, unproject_eps=1e-8):
    """unproject_normalized as the kernel computes it, in f64: fixed iteration counts.  (xn, yn, valid), NaN where not valid."""
    th = np.asarray(params, dtype=np.float64)
    uv = np.asarray(uv).astype(np.float64).reshape(-1, 2)
    mx, my = (uv[:, 0] - th[2]) / th[0], (uv[:, 1] - th[3]) / th[1]
    r2 = mx * mx + my * my
    n = len(mx)
    xn, yn = np.full(n, np.nan), np.full(n, np.nan)
    with np.errstate(all="ignore"):
        if model == DIVISION:
            sc = 1.0 + th[4] * r2
            valid = sc > 1e-9
            x, y = mx / sc, my / sc
        elif model in (UCM, EUCM):
            alpha, beta = th[4], (th[5] if model == EUCM else 1.0)
            valid = np.ones(n, dtype=bool)
            if alpha > 0.5:
                valid &= ~(r2 > 1.0 / (beta * (2.0 * alpha - 1.0)))
            t1 = 1.0 - (2.0 * alpha - 1.0) * beta * r2
            valid &= ~(t1 < 0.0)
            den = alpha * np.sqrt(t1) + (1.0 - alpha)
            k = (1.0 - alpha * alpha * beta * r2) / den
            valid &= (den > 0.0) & (k > 1e-3) & (k < np.inf)
            x, y = mx / k, my / k
        elif model == KB4:
            r = np.sqrt(r2)
            t = r.copy()
            for _ in range(10):
                t2 = t * t
                f = t * (1.0 + t2 * (th[4] + t2 * (th[5] + t2 * (th[6] + t2 * th[7])))) - r
                fp = 1.0 + t2 * (3.0 * th[4] + t2 * (5.0 * th[5] + t2 * (7.0 * th[6] + t2 * 9.0 * th[7])))
                t = t - f / fp
            small = r < unproject_eps
            tt = t * t
            res = t * (1.0 + tt * (th[4] + tt * (th[5] + tt * (th[6] + tt * th[7])))) - r
            valid = small | ((t > 0.0) & (t < 1.5) & (np.abs(res) < 1e-9))          # the kernel's acceptance rule
            s = np.tan(t) / r
            x, y = np.where(small, mx, mx * s), np.where(small, my, my * s)
        elif model == OPENCV5:
            k1, k2, p1, p2, k3 = th[4:9]
            x, y = mx.copy(), my.copy()
            for _ in range(25):
                q = x * x + y * y
                rad = 1.0 + q * (k1 + q * (k2 + q * k3))
                dx = 2.0 * p1 * x * y + p2 * (q + 2.0 * x * x)
                dy = p1 * (q + 2.0 * y * y) + 2.0 * p2 * x * y
                x, y = (mx - dx) / rad, (my - dy) / rad
            fx, fy = _ocv5_forward(x, y, k1, k2, p1, p2, k3)
            valid = np.abs(fx - mx) + np.abs(fy - my) < 1e-9
        else:
            raise ValueError(f"unknown model {model}")
    xn[valid], yn[valid] = x[valid], y[valid]
    return xn, yn, valid


# ---- the least-squares problem ---------------------------------------------------------------------------------------------------
def design(X, Y, xn, yn, dtype=LD):
    """A [2 n, 8] and b [2 n]: corner i gives rows 2 i (x) and 2 i + 1 (y) of A h = b, h = h11 h12 h13 h21 h22 h23 h31 h32."""
    X, Y, xn, yn = (np.asarray(v).astype(dtype) for v in (X, Y, xn, yn))
    n = len(X)
    A, b = np.zeros((2 * n, 8), dtype=dtype), np.zeros(2 * n, dtype=dtype)
    A[0::2, 0], A[0::2, 1], A[0::2, 2], A[0::2, 6], A[0::2, 7] = X, Y, 1, -xn * X, -xn * Y
    A[1::2, 3], A[1::2, 4], A[1::2, 5], A[1::2, 6], A[1::2, 7] = X, Y, 1, -yn * X, -yn * Y
    b[0::2], b[1::2] = xn, yn
    return A, b


def _householder_lstsq(A, b):
    """min |A h - b| by Householder QR in A's own precision (no pivoting); None where a column has nothing left below the diagonal."""
    A, b = A.copy(), b.copy()
    m, n = A.shape
    for j in range(n):
        x = A[j:, j]
        nx = np.sqrt((x * x).sum())
        if not nx > 0:
            return None
        alpha = -nx if x[0] >= 0 else nx
        v = x.copy()
        v[0] = v[0] - alpha
        vv = (v * v).sum()
        if vv > 0:
            A[j:, j:] = A[j:, j:] - np.outer(v, (2 / vv) * (v @ A[j:, j:]))
            b[j:] = b[j:] - v * ((2 / vv) * (v @ b[j:]))
    h = np.zeros(n, dtype=A.dtype)
    for i in range(n - 1, -1, -1):
        h[i] = (b[i] - (A[i, i + 1:n] * h[i + 1:]).sum()) / A[i, i]
    return h


def _rel_pivots(M, sqrt):
    """s_j / M_jj of the Cholesky of M (whatever number type M holds); stops at a pivot that is not positive."""
    n = len(M)
    L = [[M[i][j] for j in range(n)] for i in range(n)]
    out = []
    for j in range(n):
        s = L[j][j]
        for q in range(j):
            s = s - L[j][q] * L[j][q]
        out.append(s / M[j][j])
        if not s > 0:
            break
        l = sqrt(s)
        L[j][j] = l
        for i in range(j + 1, n):
            t = L[i][j]
            for q in range(j):
                t = t - L[i][q] * L[j][q]
            L[i][j] = t / l
    return out


def min_rel_pivot_ld(A):
    """The smallest s / M_jj of the Cholesky of A^T A, all of it in long double."""
    M = A.T @ A
    if not (np.diag(M) > 0).all():
        return 0.0
    return float(min(_rel_pivots(M, np.sqrt)))


def _mpf(v):
    """A long double as an mpf, exactly: its f64 rounding plus what that left over."""
    hi = float(v)
    return _mp.mpf(hi) + _mp.mpf(float(LD(v) - LD(hi)))


def _mp_matrix(A):
    return [[_mpf(v) for v in row] for row in A]


def min_rel_pivot_mp(A):
    """The same at 50 digits (mpmath), or None where mpmath cannot be imported."""
    if _mp is None:
        return None
    with _mp.workdps(50):
        a = _mp_matrix(A)
        n = len(a[0])
        M = [[_mp.fsum(row[i] * row[j] for row in a) for j in range(n)] for i in range(n)]
        if not all(M[j][j] > 0 for j in range(n)):
            return 0.0
        return float(min(_rel_pivots(M, _mp.sqrt)))


def solve_mp(A, b):
    """h of the same system at 50 digits (normal equations are harmless there), as floats; None without mpmath."""
    if _mp is None:
        return None
    with _mp.workdps(50):
        Am = _mp.matrix(_mp_matrix(A))
        bm = _mp.matrix([[v[0]] for v in _mp_matrix(b.reshape(-1, 1))])
        h = _mp.lu_solve(Am.T * Am, Am.T * bm)
        return np.array([LD(_mp.nstr(h[i], 30)) for i in range(8)], dtype=LD)


def pose_from_h(h, sum_x, sum_y, n):
    """The kernel's post-processing: lambda = 2 / (n1 + n2), the sign that puts the corners in front of the camera (their summed
    depth h31 sum X + h32 sum Y + n is positive), Gram-Schmidt of column 2 against column 1, r3 = r1 x r2.  (R, t) or None."""
    c1, c2 = np.array([h[0], h[3], h[6]]), np.array([h[1], h[4], h[7]])
    n1, n2 = np.sqrt((c1 * c1).sum()), np.sqrt((c2 * c2).sum())
    lam = 2 / (n1 + n2)
    t = np.array([lam * h[2], lam * h[5], lam])
    if not n1 > 1e-12:
        return None
    c1 = c1 / n1
    if h[6] * sum_x + h[7] * sum_y + n < 0:
        c1, c2, t = -c1, -c2, -t
    c2 = c2 - (c1 * c2).sum() * c1
    n2b = np.sqrt((c2 * c2).sum())
    if not n2b > 1e-12 or not lam == lam:
        return None
    c2 = c2 / n2b
    c3 = np.array([c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]])
    return np.stack([c1, c2, c3], axis=1), t


def solve(X, Y, xn, yn):
    """The estimate from corners (X, Y, 0) seen at (xn, yn): dict with R [3, 3] and t [3] (float64 values of the long-double
    result; None / None where the QR breaks down), h (long double), kappa (2-norm condition number of the design with its columns
    scaled to unit length) and min_rel_pivot (long double; min_rel_pivot_mp beside it where mpmath imports)."""
    A, b = design(X, Y, xn, yn)
    out = {"R": None, "t": None, "h": None, "A": A, "b": b}
    norms = np.sqrt((A * A).sum(axis=0))
    with np.errstate(all="ignore"):
        sv = np.linalg.svd((A / np.where(norms > 0, norms, 1)).astype(np.float64), compute_uv=False)
        out["kappa"] = float(sv[0] / sv[-1]) if sv[-1] > 0 else np.inf
    out["min_rel_pivot"] = min_rel_pivot_ld(A)
    out["min_rel_pivot_mp"] = min_rel_pivot_mp(A)
    h = _householder_lstsq(A, b)
    if h is None or not np.isfinite(h.astype(np.float64)).all():
        return out
    out["h"] = h
    rt = pose_from_h(h, A[0::2, 0].sum(), A[0::2, 1].sum(), len(A) // 2)
    if rt is not None:
        out["R"], out["t"] = rt[0].astype(np.float64), rt[1].astype(np.float64)
    return out


def frame_pose(model, params, X, Y, uv, min_points=10, unproject_eps=1e-8, tol=PIVOT_TOL):
    """One frame as the library is to treat it: None where fewer than min_points corners unproject or where the valid corners do
    not span the board plane (an exact Cholesky pivot <= tol x its diagonal entry); else solve()'s dict over exactly the valid
    corners, with `used` = their number."""
    xn, yn, valid = unproject(model, params, uv, unproject_eps)
    used = int(valid.sum())
    if used < max(int(min_points), 0) or used == 0:
        return None
    X, Y = np.asarray(X)[valid], np.asarray(Y)[valid]
    s = solve(X, Y, xn[valid], yn[valid])
    piv = s["min_rel_pivot_mp"] if s["min_rel_pivot_mp"] is not None else s["min_rel_pivot"]
    if not piv > tol or s["R"] is None:
        return None
    s["used"] = used
    return s


# ---- the kernel's arithmetic in f64 ------------------------------------------------------------------------------------------------
_PAIRS = [(i, j) for i in range(8) for j in range(i, 8)]


def rotmat_to_rvec_kernel(R):
    """The kernel's matrix -> quaternion -> rvec: (rvec, branch 0 .. 3, flipped)."""
    R00, R10, R20, R01, R11, R21, R02, R12, R22 = R[0, 0], R[1, 0], R[2, 0], R[0, 1], R[1, 1], R[2, 1], R[0, 2], R[1, 2], R[2, 2]
    tr = R00 + R11 + R22
    if tr >= R00 and tr >= R11 and tr >= R22:
        branch, s = 0, 2.0 * np.sqrt(max(tr + 1.0, 1e-300))
        qw, qx, qy, qz = 0.25 * s, (R21 - R12) / s, (R02 - R20) / s, (R10 - R01) / s
    elif R00 >= R11 and R00 >= R22:
        branch, s = 1, 2.0 * np.sqrt(max(1.0 + R00 - R11 - R22, 1e-300))
        qw, qx, qy, qz = (R21 - R12) / s, 0.25 * s, (R01 + R10) / s, (R02 + R20) / s
    elif R11 >= R22:
        branch, s = 2, 2.0 * np.sqrt(max(1.0 + R11 - R00 - R22, 1e-300))
        qw, qx, qy, qz = (R02 - R20) / s, (R01 + R10) / s, 0.25 * s, (R12 + R21) / s
    else:
        branch, s = 3, 2.0 * np.sqrt(max(1.0 + R22 - R00 - R11, 1e-300))
        qw, qx, qy, qz = (R10 - R01) / s, (R02 + R20) / s, (R12 + R21) / s, 0.25 * s
    flipped = bool(qw < 0.0)
    if flipped:
        qw, qx, qy, qz = -qw, -qx, -qy, -qz
    vn = np.sqrt(qx * qx + qy * qy + qz * qz)
    ang = 2.0 * np.arctan2(vn, qw)
    sc = ang / vn if vn > 1e-15 else 0.0
    return np.array([qx * sc, qy * sc, qz * sc]), branch, flipped


def emulate_f64(model, params, X, Y, uv, min_points=10, unproject_eps=1e-8, tol=PIVOT_TOL):
    """k_pose_init on one frame in f64 numpy: corner c goes to lane c % 64, each lane sums its corners in order, the 64 lanes are
    added by the xor butterfly (32, 16, ... 1), lane 0 does the Cholesky with the pivot rule s > tol M_jj (tol = 0: s > 0).
    dict: pose [6] (zeros without a pose), used, R, t (None without a pose), branch, flipped, min_rel_pivot."""
    X, Y = np.asarray(X).astype(np.float64), np.asarray(Y).astype(np.float64)
    xn, yn, valid = unproject_kernel_f64(model, params, uv, unproject_eps)
    part = np.zeros((64, 44))
    for c in range(len(X)):
        if not valid[c]:
            continue
        r1 = np.array([X[c], Y[c], 1.0, 0.0, 0.0, 0.0, -xn[c] * X[c], -xn[c] * Y[c]])
        r2 = np.array([0.0, 0.0, 0.0, X[c], Y[c], 1.0, -yn[c] * X[c], -yn[c] * Y[c]])
        row = part[c % 64]
        for k, (i, j) in enumerate(_PAIRS):
            row[k] += r1[i] * r1[j] + r2[i] * r2[j]
        row[36:] += r1 * xn[c] + r2 * yn[c]
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[idx ^ off]
    M, rhs, cnt = part[0, :36], part[0, 36:], int(valid.sum())
    out = {"pose": np.zeros(6), "used": 0, "R": None, "t": None, "branch": None, "flipped": None, "min_rel_pivot": None}
    if cnt < min_points:
        return out
    L = np.zeros((8, 8))
    for k, (i, j) in enumerate(_PAIRS):
        L[j, i] = M[k]
    diag = L.diagonal().copy()
    rel = []
    for j in range(8):
        s = L[j, j]
        for q in range(j):
            s -= L[j, q] * L[j, q]
        rel.append(s / diag[j] if diag[j] > 0 else 0.0)
        out["min_rel_pivot"] = min(rel)
        if not s > tol * diag[j]:
            return out
        l = np.sqrt(s)
        L[j, j] = l
        for i in range(j + 1, 8):
            t = L[i, j]
            for q in range(j):
                t -= L[i, q] * L[j, q]
            L[i, j] = t / l
    h = np.zeros(8)
    for i in range(8):
        t = rhs[i]
        for q in range(i):
            t -= L[i, q] * h[q]
        h[i] = t / L[i, i]
    for i in range(7, -1, -1):
        t = h[i]
        for q in range(i + 1, 8):
            t -= L[q, i] * h[q]
        h[i] = t / L[i, i]
    rt = pose_from_h(h, M[2], M[9], M[15])
    if rt is None:
        return out
    R, t = rt
    rvec, branch, flipped = rotmat_to_rvec_kernel(R)
    pose = np.concatenate([rvec, t])
    if not np.isfinite(pose).all():
        return out
    out.update(pose=pose, used=cnt, R=R, t=t, branch=branch, flipped=flipped)
    return out
