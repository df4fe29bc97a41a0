"""Named, seeded systems for the camera solves and the pose back-substitution (TEST INFRASTRUCTURE, not collected:
tests/test_camera_solve_cpu.py checks what every case claims, tests/test_gpu_camera_solve.py feeds them to k_solve, k_head and k_backsub
through ccal_test_camera_solve / ccal_test_backsub).

Sizes: k_solve every K in 1 .. 127, k_head every K in 4 .. 9.  Families, at every size (seeds 0 and 1, thinned above K = 40: seeds(); cur = (K + seed) & 1):
    scaled   D M D, M = J^T J of a 4K x K Gaussian J scaled to a unit diagonal (condition number about 10), log10 D uniform in [-4, 3];
             the step x* is chosen first (|D x*| in [0.3, 3]) and b = -S x*, so b is of matching scale; every term of mc is positive
             (g_i = -sign(x*_i) |.|): the relative measure of mc sees no cancellation of the test's own making
    stiff    the same with M = Q diag(s) Q^T, unit diagonal, condition number within [1e6, 1e8] (drawn until it is)
    fixed    fixed flags on column 0, K - 1, three in the middle and 31 / 32 / 33 / 63 / 64 where K allows (K <= 5: column 0 or K - 1
             alone); NaN, 1e300 and -7.5 in the fixed rows and columns of the input; seed 1 has lambda = 1.5, max_diag = 1.7e308 and a damping
             diagonal of 1.7e308 on the fixed columns: "a fixed diagonal stays 1" - damped, it would overflow and the solve report not-PD
    bounds   every third column clamps at hi, every third at lo - x + dc* at least 10 % of the interval outside it - the rest sit well
             inside; dst2 mirrors on some columns; intrinsic and extrinsic columns mixed (as in every family)
    damped   lambda = (1e-4, 1, 1e4)[(K + seed) % 3], min_diag 1e-6, max_diag 1e2, hdiag below, inside and above (K >= 3)
    layout   (k_solve) the product's parameter layout for 2 .. 8 cameras (10 intrinsics and 6 extrinsics per camera, one-focal mirrors),
             and layout_strided: n_intr = 70 at K = 40 - the strided copy of the parameter sets, which no product call reaches
    not_pd   per size six ways to fail: the first non-positive pivot at column 0, K / 2, K - 1 (pivot = -0.5 x what it was), an exactly
             zero pivot (a duplicated column of an integer system L L^T with a unit diagonal: every operation of the factorisation is
             exact in any order, at any precision), one NaN entry, one +inf diagonal; seed 0 Gauss-Newton, seed 1 LM
Backsub: K in (4, 9, 24, 63, 64, 114, 127) x n_slots in (1, 15, 16, 17, 33); in each launch one record with R[0] == 0, one with dC
below min_diag and one above max_diag (n_slots == 1: one of the three, in turn).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import camera_solve_ref as ref

SOLVE_SIZES = {"k_solve": range(1, 128), "k_head": range(4, 10)}
FAMILIES = ("scaled", "stiff", "fixed", "bounds", "damped")
NOT_PD_KINDS = ("first", "middle", "last", "duplicate", "nan", "inf")
LAMBDAS = (1e-4, 1.0, 1e4)
BACKSUB_K = (4, 9, 24, 63, 64, 114, 127)
BACKSUB_SLOTS = (1, 15, 16, 17, 33)
GARBAGE = (np.nan, 1e300, -7.5)
FIXED_HDIAG = 1.7e308
TWO_SEEDS = frozenset((*range(61, 67), *range(112, 117), *range(124, 128)))


@dataclass
class SolveCase:
    name: str
    form: str
    family: str
    K: int
    seed: int
    red: np.ndarray
    cols: np.ndarray                 # ref.COL_DTYPE [K]
    n_intr: int
    n_extr: int
    intr: np.ndarray                 # the current set's values
    extr: np.ndarray
    lam: float
    min_diag: float
    max_diag: float
    cur: int
    claims: dict = field(default_factory=dict)


@dataclass
class BacksubCase:
    name: str
    K: int
    n_slots: int
    seed: int
    pf: np.ndarray                   # [n_slots][pf_size(K)]
    dc: np.ndarray
    poses: np.ndarray                # [n_slots][6], the current set
    lam: float
    min_diag: float
    max_diag: float
    cur: int
    claims: dict = field(default_factory=dict)


def _seed(*parts):
    return np.random.default_rng([abs(hash_part(p)) for p in parts])


def hash_part(p):
    if isinstance(p, int):
        return p
    return int.from_bytes(str(p).encode(), "little") % (1 << 31)


def _unit_diagonal(M):
    d = 1.0 / np.sqrt(np.diag(M))
    M = M * d[:, None] * d[None, :]
    M = 0.5 * (M + M.T)
    np.fill_diagonal(M, 1.0)
    return M


def scaled_condition(S):
    """condition number of S scaled to a unit diagonal"""
    if len(S) == 1:
        return 1.0
    w = np.linalg.eigvalsh(_unit_diagonal(S))
    return float(w[-1] / w[0])


def _well_conditioned(rng, K):
    J = rng.standard_normal((4 * K + 4, K))
    return _unit_diagonal(J.T @ J)


def _stiff(rng, K):
    if K == 1:
        return np.ones((1, 1))
    for _ in range(200):
        cond = 10.0 ** rng.uniform(6.5, 7.5)
        Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
        s = np.exp(rng.uniform(-np.log(cond), 0.0, K))
        s[0], s[-1] = 1.0, 1.0 / cond
        M = _unit_diagonal((Q * s) @ Q.T)
        if 1e6 <= scaled_condition(M) <= 1e8:
            return M
    raise AssertionError("no stiff matrix drawn")


def _layout_generic(rng, K, NTH, mirrors=True, n_intr=None):
    """columns scattered over two parameter arrays: about 40 % extrinsic from K = 3 on, a few one-focal mirrors, parameters that are
    no column's; both arrays within the one-pass copy (<= NTH) unless n_intr says otherwise"""
    cols = np.zeros(K, ref.COL_DTYPE)
    cols["dst2"] = -1
    n_e = int(round(0.4 * K)) if K >= 3 else 0
    is_e = np.zeros(K, bool)
    is_e[rng.permutation(K)[:n_e]] = True
    n_i = K - n_e
    n_m = min(n_i, 1 + K // 20) if mirrors and K >= 2 else 0
    total_i = n_intr if n_intr is not None else n_i + n_m + 3
    total_e = n_e + 2 if K >= 3 else 0
    assert n_intr is not None or (total_i <= NTH and total_e <= NTH)
    slots_i, slots_e = list(rng.permutation(total_i)), list(rng.permutation(total_e))
    cols["is_extr"] = is_e
    icols = [i for i in range(K) if not is_e[i]]
    for i in range(K):
        cols["dst"][i] = (slots_e if is_e[i] else slots_i).pop()
    for i in [icols[j] for j in rng.permutation(len(icols))[:n_m]]:
        cols["dst2"][i] = slots_i.pop()
    return cols, total_i, total_e


PRODUCT_RIGS = {                    # cameras -> (columns per camera, one focal length); K = sum + 6 (cameras - 1)
    2: ((6, 8), False), 3: ((5, 7, 8), True), 4: ((9, 9, 6, 8), False), 5: ((5, 5, 5, 5, 5), True), 6: ((6, 6, 8, 8, 9, 5), False),
    7: ((8, 8, 8, 8, 8, 8, 8), True), 8: ((9,) * 8, False),
}


def _layout_product(n_cams):
    peff, one_focal = PRODUCT_RIGS[n_cams]
    rows = []
    for c, p in enumerate(peff):
        for i in range(p):
            full = (0 if i == 0 else i + 1) if one_focal else i
            rows.append((0, c * ref.PMAX + full, c * ref.PMAX + 1 if one_focal and i == 0 else -1))
    for c in range(1, n_cams):
        rows += [(1, c * 6 + i, -1) for i in range(6)]
    cols = np.zeros(len(rows), ref.COL_DTYPE)
    for k, (e, d, d2) in enumerate(rows):
        cols["is_extr"][k], cols["dst"][k], cols["dst2"][k] = e, d, d2
    return cols, n_cams * ref.PMAX, n_cams * 6


def _pack(form, K, S, b, hdiag, gc, rng, yscale=None):
    """the form's reduced sums for the system S (symmetric, f64), right-hand-side row b, damping diagonal and gradient"""
    K1 = K + 1
    if form == "k_solve":
        red = np.full(ref.red_size(K), np.nan)                  # what the kernel must not read stays NaN: the upper triangle, A[K][K]
        A = red[:K1 * K1].reshape(K1, K1)
        il = np.tril_indices(K)
        A[:K, :K][il] = S[il]
        A[K, :K] = b
        red[K1 * K1:K1 * K1 + K] = hdiag
        red[K1 * K1 + K:K1 * K1 + 2 * K] = gc
        red[-3:] = (1.25, 0.5, 0.0)                              # cost, mc_pose, failed pose blocks
        return red
    # k_head: S = A_dir - Y^T Y, b = A_dir[:, K] - Y^T Y[:, K], the damping diagonal IS A_dir's, the gradient A_dir[:, K]
    red = np.zeros(ref.fused_red_size(K))
    Ad, Yt = red[:K1 * K1].reshape(K1, K1), red[K1 * K1:2 * K1 * K1].reshape(K1, K1)
    if yscale is None:
        W = rng.standard_normal((K, 3)) * np.sqrt(np.abs(np.diag(S)))[:, None] * 0.4
        Y = W @ W.T
        np.fill_diagonal(Y, hdiag - np.diag(S))                  # (hdiag >= diag S: the caller's)
    else:
        Y = yscale
    Yt[:K, :K] = Y
    Ad[:K, :K] = S + Y
    Ad[:K, K] = gc
    Yt[:K, K] = gc - b
    Ad[K, :K], Yt[K, :K] = Ad[:K, K], Yt[:K, K]
    Ad[K, K], Yt[K, K] = 1.25, 0.25
    red[-2:] = (0.5, 0.0)
    return red


def _build(form, family, K, seed):
    rng = _seed("camera_solve", form, family, K, seed)
    NTH = 128 if K >= 64 else 64
    lam, min_diag, max_diag = 0.0, 1e-6, 1e32
    claims = {}
    M = _stiff(rng, K) if family == "stiff" else _well_conditioned(rng, K)
    D = 10.0 ** rng.uniform(-4.0, 3.0, K)
    if family == "damped":
        lam, max_diag = LAMBDAS[(K + seed) % 3], 1e2
        if K >= 3:
            D[rng.permutation(K)[:3]] = (1e-4, 1.0, 1e3)          # hdiag = D^2 u: below min_diag, inside, above max_diag
    if family == "fixed" and seed == 1:
        lam, max_diag = 1.5, 1.7e308               # with FIXED_HDIAG on the fixed columns: damping one of them overflows its diagonal
    S = M * D[:, None] * D[None, :]
    hdiag = np.diag(S) * rng.uniform(1.0, 2.0, K)
    if form == "k_head":
        cols = np.zeros(K, ref.COL_DTYPE)
        one_focal = (K + seed) % 2 == 0
        cols["dst"] = [(0 if i == 0 else i + 1) if one_focal else i for i in range(K)]
        cols["dst2"] = -1
        if one_focal:
            cols["dst2"][0] = 1
        n_intr, n_extr = ref.PMAX, 0
    else:
        cols, n_intr, n_extr = _layout_generic(rng, K, NTH)
    z = rng.uniform(0.3, 3.0, K) * rng.choice((-1.0, 1.0), K)
    xstar = z / D
    Dii = lam * np.clip(hdiag, min_diag, max_diag) if lam > 0 else np.zeros(K)
    b = -((S + np.diag(Dii)) @ xstar)
    gc = -np.sign(xstar) * D * rng.uniform(0.5, 2.0, K)
    intr = rng.uniform(-5.0, 5.0, n_intr)
    extr = rng.uniform(-5.0, 5.0, n_extr)
    for i in range(K):                                            # the current value of a column's parameter: of the step's size
        (extr if cols["is_extr"][i] else intr)[cols["dst"][i]] = rng.uniform(-5.0, 5.0) / D[i]
        if cols["dst2"][i] >= 0:
            intr[cols["dst2"][i]] = intr[cols["dst"][i]]
    if family == "fixed":
        mid = K // 2
        if K == 1:
            fx = {0}
        elif K <= 5:
            fx = {0} if seed == 0 else {K - 1}
        else:
            fx = {c for c in (0, K - 1, mid - 1, mid, mid + 1, 31, 32, 33, 63, 64) if c < K}
        cols["fixed"][sorted(fx)] = 1
        claims["fixed"] = sorted(fx)
    if family == "bounds":
        for i in range(K):
            x = (extr if cols["is_extr"][i] else intr)[cols["dst"][i]]
            v, w = x + xstar[i], abs(xstar[i]) * rng.uniform(0.5, 2.0)
            kind = i % 3 if K >= 3 else (i + seed) % 3               # 0: clamps at hi, 1: at lo, 2: well inside
            if kind == 0:
                hi = v - rng.uniform(0.1, 0.6) * w
                lo = hi - w
            elif kind == 1:
                lo = v + rng.uniform(0.1, 0.6) * w
                hi = lo + w
            else:
                lo = v - rng.uniform(0.3, 0.7) * w
                hi = lo + w
            cols["lo"][i], cols["hi"][i], cols["has_bound"][i] = lo, hi, 1
        claims["clamped"] = [(1, -1, 0)[i % 3 if K >= 3 else (i + seed) % 3] for i in range(K)]
    red = _pack(form, K, S, b, hdiag, gc, rng)
    if family == "fixed":                                         # garbage in the fixed rows and columns of the input
        K1 = K + 1
        n_mat = 1 if form == "k_solve" else 2
        for f in claims["fixed"]:
            for m in range(n_mat):
                A = red[m * K1 * K1:(m + 1) * K1 * K1].reshape(K1, K1)
                g = rng.choice(GARBAGE, 2 * K + 1)
                A[f, :K], A[:K, f] = g[:K], g[K:2 * K]
                if form == "k_head":
                    A[f, K] = g[-1]
                else:
                    A[K, f] = g[-1]
            if form == "k_solve":
                red[K1 * K1 + f], red[K1 * K1 + K + f] = rng.choice(GARBAGE, 2)
            if lam > 0:                                           # the damping diagonal of a fixed column: hdiag, or A_dir's own
                red[K1 * K1 + f if form == "k_solve" else f * K1 + f] = FIXED_HDIAG
    return SolveCase(f"{form}_{family}_K{K}_s{seed}", form, family, K, seed, red, cols, n_intr, n_extr, intr, extr, lam, min_diag,
                     max_diag, (K + seed) & 1, claims)


def _build_layout(n_cams, seed, strided=False):
    rng = _seed("camera_solve_layout", n_cams, seed, int(strided))
    if strided:
        K = 40
        cols, n_intr, n_extr = _layout_generic(rng, K, 64, n_intr=70)
        name = f"k_solve_layout_strided_s{seed}"
    else:
        cols, n_intr, n_extr = _layout_product(n_cams)
        K = len(cols)
        name = f"k_solve_layout_cams{n_cams}_s{seed}"
    M, D = _well_conditioned(rng, K), 10.0 ** rng.uniform(-4.0, 3.0, K)
    S = M * D[:, None] * D[None, :]
    xstar = rng.uniform(0.3, 3.0, K) * rng.choice((-1.0, 1.0), K) / D
    lam = 1.0 if seed else 0.0
    hdiag = np.diag(S) * rng.uniform(1.0, 2.0, K)
    b = -((S + np.diag(lam * np.clip(hdiag, 1e-6, 1e32))) @ xstar)
    gc = -np.sign(xstar) * D * rng.uniform(0.5, 2.0, K)
    intr, extr = rng.uniform(-5.0, 5.0, n_intr), rng.uniform(-5.0, 5.0, n_extr)
    for i in range(K):
        (extr if cols["is_extr"][i] else intr)[cols["dst"][i]] = rng.uniform(-5.0, 5.0) / D[i]
        if cols["dst2"][i] >= 0:
            intr[cols["dst2"][i]] = intr[cols["dst"][i]]
    return SolveCase(name, "k_solve", "layout", K, seed, _pack("k_solve", K, S, b, hdiag, gc, rng), cols, n_intr, n_extr, intr, extr, lam,
                     1e-6, 1e32, (n_cams + seed) & 1, {"n_cams": n_cams})


def _integer_system(rng, K, p):
    """L L^T of a unit lower-triangular band matrix of small integers whose row p repeats row q = p - 1 (p == 0: a zero row): rows and
    columns p and q of the product are equal, the pivots before p are exactly 1 and pivot p is exactly 0"""
    L = np.eye(K)
    for i in range(1, K):
        L[i, max(0, i - 2):i] = rng.integers(-1, 2, min(i, 2))
    if p == 0:
        L[0, 0] = 0.0
    else:
        L[p, :] = L[p - 1, :]
    return L @ L.T


def _build_not_pd(form, K, kind, seed):
    rng = _seed("camera_solve_not_pd", form, K, kind, seed)
    lm = seed == 1
    lam, min_diag, max_diag = (1e-3 if lm else 0.0), 1e-6, 1e32
    p = {"first": 0, "middle": K // 2, "last": K - 1}.get(kind)
    yscale = None
    if kind == "duplicate":
        p = int(rng.integers(1, K)) if K > 1 else 0
        S, D = _integer_system(rng, K, p), np.ones(K)
        min_diag = max_diag = 0.0                                 # LM: the damping term is exactly 0, the system stays the integer one
        hdiag = np.diag(S) + 1.0
        if form == "k_head":
            yscale = np.diag(hdiag - np.diag(S))
    else:
        M, D = _well_conditioned(rng, K), 10.0 ** rng.uniform(-4.0, 3.0, K)
        S = M * D[:, None] * D[None, :]
        hdiag = np.diag(S) * rng.uniform(1.0, 2.0, K)
        if kind in ("nan", "inf"):
            p = int(rng.integers(1, K)) if K > 1 else 0
        Dii = lam * np.clip(hdiag, min_diag, max_diag) if lm else np.zeros(K)
        if kind == "inf":
            S[p, p] = np.inf
        elif kind == "nan":
            if K > 1:
                q = int(rng.integers(0, p))
                S[p, q] = S[q, p] = np.nan
            else:
                S[0, 0] = np.nan
        elif form == "k_solve":
            L, bad = ref.cholesky_f64(S + np.diag(Dii))
            assert L is not None, bad
            S[p, p] -= 1.5 * L[p, p] ** 2                           # the damped pivot becomes -0.5 x what it was
    b = rng.uniform(0.3, 3.0, K) * rng.choice((-1.0, 1.0), K) * D
    gc = rng.uniform(0.3, 3.0, K) * D
    if form == "k_head":
        cols = np.zeros(K, ref.COL_DTYPE)
        cols["dst"], cols["dst2"], n_intr, n_extr = np.arange(K), -1, ref.PMAX, 0
        if kind in ("nan", "inf"):
            yscale = np.diag(hdiag - np.where(np.isfinite(np.diag(S)), np.diag(S), 0.0))
    else:
        cols, n_intr, n_extr = _layout_generic(rng, K, 128 if K >= 64 else 64)
    red = _pack(form, K, S, b, hdiag, gc, rng, yscale)
    if form == "k_head" and kind not in ("duplicate", "nan", "inf"):
        # on the sums as the kernel will subtract them (S + Y - Y is not S to the last bit); the damping reads A_dir's diagonal, which
        # the change itself moves by 1.5e-3 of the pivot: it stays below -0.49 x what it was
        K1 = K + 1
        Ad, Yt = red[:K1 * K1].reshape(K1, K1), red[K1 * K1:2 * K1 * K1].reshape(K1, K1)
        Sd = Ad[:K, :K] - Yt[:K, :K] + np.diag(lam * np.clip(np.diag(Ad)[:K], min_diag, max_diag) if lm else np.zeros(K))
        L, bad = ref.cholesky_f64(Sd)
        assert L is not None, bad
        Ad[p, p] -= 1.5 * L[p, p] ** 2
    intr, extr = rng.uniform(-5.0, 5.0, n_intr), rng.uniform(-5.0, 5.0, n_extr)
    return SolveCase(f"{form}_not_pd_{kind}_K{K}_s{seed}", form, "not_pd", K, seed, red, cols, n_intr, n_extr, intr, extr, lam, min_diag,
                     max_diag, (K + seed) & 1, {"fails_at": p, "kind": kind, "lm": lm})


def _build_backsub(K, n_slots, seed):
    rng = _seed("backsub", K, n_slots, seed)
    PF, K1 = ref.pf_size(K), K + 1
    lam, min_diag, max_diag = (1.0 if seed else 0.0), 1e-6, 1e2
    pf = np.zeros((n_slots, PF))
    Dp = 10.0 ** rng.uniform(-2.0, 2.0, 6)                          # rotation and translation columns of a pose differ in scale
    Dc = 10.0 ** rng.uniform(-4.0, 3.0, K)
    dc = rng.uniform(0.3, 3.0, K) * rng.choice((-1.0, 1.0), K) / Dc
    special = {}
    for s in range(n_slots):
        J = rng.standard_normal((30, 6))
        C = (J.T @ J / 30.0) * Dp[:, None] * Dp[None, :]
        L = np.linalg.cholesky(C)
        for i in range(6):
            for j in range(i + 1):
                pf[s, i * (i + 1) // 2 + j] = 1.0 / L[i, i] if i == j else L[i, j]
        Y = rng.standard_normal((6, K1)) * Dp[:, None]
        Y[:, :K] *= Dc[None, :]
        pf[s, 21:21 + 6 * K1] = Y.ravel()
        dp = -np.linalg.solve(L.T, Y[:, K] + Y[:, :K] @ dc)         # every term of the slot's mc is positive: g_p against the step
        pf[s, 21 + 6 * K1:21 + 6 * K1 + 6] = -np.sign(dp) * rng.uniform(0.3, 3.0, 6) * Dp
        pf[s, 21 + 6 * K1 + 6:21 + 6 * K1 + 12] = np.diag(C) * rng.uniform(1.0, 2.0, 6)
        if PF > 21 + 6 * K1 + 12:
            pf[s, 21 + 6 * K1 + 12:] = np.nan                       # the record's padding is nobody's
    order = list(rng.permutation(n_slots))
    kinds = ("unobserved", "dC_below", "dC_above") if n_slots >= 3 else (("unobserved", "dC_below", "dC_above")[(BACKSUB_K.index(K) + seed) % 3],)
    for kind, s in zip(kinds, order):
        special[kind] = int(s)
        if kind == "unobserved":
            pf[s, 0] = 0.0
        elif kind == "dC_below":
            pf[s, 21 + 6 * K1 + 6:21 + 6 * K1 + 12] = rng.uniform(1e-9, 1e-7, 6)
        else:
            pf[s, 21 + 6 * K1 + 6:21 + 6 * K1 + 12] = rng.uniform(1e3, 1e5, 6)
    poses = rng.uniform(-2.0, 2.0, (n_slots, 6))
    return BacksubCase(f"backsub_K{K}_n{n_slots}_s{seed}", K, n_slots, seed, pf, dc, poses, lam, min_diag, max_diag, (K + n_slots + seed) & 1,
                       special)


_CACHE: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        c = _CACHE[key] = make()
        for a in (getattr(c, n, None) for n in ("red", "cols", "intr", "extr", "pf", "dc", "poses")):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _CACHE[key]


def solve_case(form, family, K, seed):
    return _cached((form, family, K, seed), lambda: _build(form, family, K, seed))


def seeds(K):
    """both seeds up to K = 40 and round the sizes where the code changes its path or ends its claim; one in between, alternating with K
    (the reference's time goes with K^2 per residual: seeds are thinned, never sizes)"""
    return (0, 1) if K <= 40 or K in TWO_SEEDS else (K & 1,)


def cell(form, family, K):
    """the cases of one (form, family, K)"""
    return [solve_case(form, family, K, s) for s in seeds(K)]


def layout_cases():
    out = [_cached(("layout", n, s), lambda n=n, s=s: _build_layout(n, s)) for n in sorted(PRODUCT_RIGS) for s in (0, 1)]
    return out + [_cached(("layout_strided", s), lambda s=s: _build_layout(7, s, strided=True)) for s in (0, 1)]


def not_pd_cases(form, K):
    return [_cached(("not_pd", form, K, kind, s), lambda kind=kind, s=s: _build_not_pd(form, K, kind, s))
            for kind in NOT_PD_KINDS for s in (0, 1)]


def backsub_cases():
    return [_cached(("backsub", K, n, s), lambda K=K, n=n, s=s: _build_backsub(K, n, s))
            for K in BACKSUB_K for n in BACKSUB_SLOTS for s in (0, 1)]
