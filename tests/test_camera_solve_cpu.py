"""CPU: what tests/test_gpu_camera_solve.py rests on - the inputs of tests/camera_solve_cases.py are what they claim, the two routes
of tests/camera_solve_ref.py to the truth agree, the unpacking index of k_solve is the integer division, and the two hooks are in the
second library only and refuse a call without a context."""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import camera_solve_cases as cases
import camera_solve_ref as ref
from camera_intrinsic_calibration_rs_amd import _ffi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camera_intrinsic_calibration_rs_amd", "csrc")


def test_unpacking_index_is_the_integer_division():
    """k_solve unpacks entry e of the K x K system with i = (int)(((float)e + 0.5f) * (1.0f / (float)K)) instead of e / K (the
    prefetch and both unpacking loops, csrc/ccal_kernels_normal.hip); the two agree for every K in 1 .. 127 and e < K^2, in IEEE float32.
    head_wave (csrc/ccal_head.hpp) uses the integer division itself."""
    src = open(os.path.join(CSRC, "ccal_kernels_normal.hip")).read()
    assert src.count("(int)(((float)e + 0.5f) * rk)") == 2 and src.count("(int)(((float)ec + 0.5f) * rk)") == 1
    assert "const int i = e / K, j = e - i * K;" in open(os.path.join(CSRC, "ccal_head.hpp")).read()
    mismatches = 0
    for K in range(1, ref.KMAX):
        e = np.arange(K * K, dtype=np.int32)
        rk = np.float32(1.0) / np.float32(K)
        i = ((e.astype(np.float32) + np.float32(0.5)) * rk).astype(np.int32)
        mismatches += int((i != e // K).sum())
    assert mismatches == 0


def test_column_record_is_the_headers():
    body = re.search(r"struct ColInfo \{(.*?)\n\};", open(os.path.join(CSRC, "ccal_normal.hpp")).read(), flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = [n.strip() for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for n in decl.split(",")]
    assert fields == [n for n in ref.COL_DTYPE.names if n != "pad_"] and ref.COL_DTYPE.itemsize == 40
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "ccal.h")).read()
    assert f"#define CCAL_KMAX {ref.KMAX}" in hdr and f"#define CCAL_PMAX {ref.PMAX}" in hdr


def _all_solve_cases():
    for form, sizes in cases.SOLVE_SIZES.items():
        for K in sizes:
            for family in cases.FAMILIES:
                yield from cases.cell(form, family, K)
    yield from cases.layout_cases()


def _check_layout(c):
    K = c.K
    assert c.red.size == (ref.red_size(K) if c.form == "k_solve" else ref.fused_red_size(K)) and c.cols.dtype == ref.COL_DTYPE
    assert len(c.cols) == K and c.intr.size == c.n_intr and c.extr.size == c.n_extr and c.cur in (0, 1)
    used = set()
    for i in range(K):
        e, n = int(c.cols["is_extr"][i]), (c.n_extr if c.cols["is_extr"][i] else c.n_intr)
        for d in (int(c.cols["dst"][i]), int(c.cols["dst2"][i])):
            if d == -1 and d == c.cols["dst2"][i]:
                continue
            assert 0 <= d < n and (e, d) not in used, (c.name, i, d)
            used.add((e, d))
    if c.family != "layout":
        NTH = 128 if K >= 64 else 64
        assert c.n_intr <= NTH and c.n_extr <= NTH, c.name                  # the one-pass copy; layout_strided alone goes beyond
        if c.form == "k_solve":
            assert len(used) < c.n_intr + c.n_extr, c.name                   # parameters that are no column's
            assert K < 3 or 0 < c.cols["is_extr"].sum() < K, c.name           # intrinsic and extrinsic columns mixed
    if c.form == "k_head":
        assert c.n_intr == ref.PMAX and c.n_extr == 0
    assert np.isfinite(c.red).any()


def test_every_size_and_family_is_there():
    names = set()
    for c in _all_solve_cases():
        _check_layout(c)
        assert c.name not in names
        names.add(c.name)
    for form, sizes in cases.SOLVE_SIZES.items():
        assert list(sizes) == (list(range(1, 128)) if form == "k_solve" else list(range(4, 10)))
        for K in sizes:
            assert set(cases.seeds(K)) <= {0, 1} and (len(cases.seeds(K)) == 2 or K > 40)
            for f in cases.FAMILIES:
                assert {c.cur for c in cases.cell(form, f, K)} == {(K + s) & 1 for s in cases.seeds(K)}
    assert all(len(cases.seeds(K)) == 2 for K in (24, 25, 32, 33, 63, 64, 114, 115, 127))
    lay = cases.layout_cases()
    assert {c.claims["n_cams"] for c in lay if "strided" not in c.name} == set(range(2, 9))
    for c in lay:
        if "strided" in c.name:
            assert (c.n_intr, c.K) == (70, 40)
        else:
            n = c.claims["n_cams"]
            assert (c.n_intr, c.n_extr) == (10 * n, 6 * n) and c.K == sum(cases.PRODUCT_RIGS[n][0]) + 6 * (n - 1)
    assert max(c.K for c in lay) == 114


def test_conditioning_is_as_claimed():
    for form, sizes in cases.SOLVE_SIZES.items():
        for K in sizes:
            if K < 2:
                continue
            for family, lo, hi in (("scaled", 1.0, 60.0), ("stiff", 1e6, 1e8)):
                for c in cases.cell(form, family, K):
                    S = np.array(ref.system(c, float)[0])
                    d = np.sqrt(np.diag(S))
                    assert lo <= cases.scaled_condition(S) <= hi, (c.name, cases.scaled_condition(S))
                    assert d.min() >= 0.9e-4 and d.max() <= 1.1e3                  # log10 D in [-4, 3]


def test_fixed_and_damped_inputs():
    for form, sizes in cases.SOLVE_SIZES.items():
        for K in sizes:
            for c in cases.cell(form, "fixed", K):
                fx = set(np.nonzero(c.cols["fixed"])[0].tolist())
                assert fx == set(c.claims["fixed"]) and fx and (c.lam > 0) == (c.seed == 1)
                if K >= 6:
                    assert fx == {i for i in (0, K - 1, K // 2 - 1, K // 2, K // 2 + 1, 31, 32, 33, 63, 64) if i < K} and len(fx) < K
                K1 = K + 1
                A = c.red[:K1 * K1].reshape(K1, K1)
                for f in fx:                                                    # garbage in the fixed rows and columns
                    assert not np.isfinite(A[f, :f + 1]).all() or (np.abs(A[f, :f + 1]) >= 7.5).all(), c.name
                if c.lam > 0:                                                   # damping a fixed column would overflow its diagonal
                    hd = c.red[K1 * K1:K1 * K1 + K] if form == "k_solve" else np.diag(A)[:K]
                    assert all(float(c.lam) * min(max(float(hd[f]), c.min_diag), c.max_diag) == float("inf") for f in fx), c.name
                    assert c.lam * np.clip(np.delete(hd, sorted(fx)), c.min_diag, c.max_diag).max() < 1e10 if len(fx) < K else True
                y = ref.yardstick(c)
                assert "dc" in y and (y["dc"][sorted(fx)] == 0.0).all() and np.isfinite(y["dc"]).all() and np.isfinite(y["mc"]), c.name
            for c in cases.cell(form, "damped", K):
                assert c.lam == cases.LAMBDAS[(K + c.seed) % 3] and (c.min_diag, c.max_diag) == (1e-6, 1e2)
                K1 = K + 1
                hd = c.red[K1 * K1:K1 * K1 + K] if form == "k_solve" else np.diag(c.red[:K1 * K1].reshape(K1, K1))[:K]
                if K >= 3:
                    assert (hd < c.min_diag).any() and (hd > c.max_diag).any() and ((hd > c.min_diag) & (hd < c.max_diag)).any(), c.name
    lams = {(K, c.lam) for K in range(1, 128) for c in cases.cell("k_solve", "damped", K)}
    for cliff in (24, 32, 63):                                                  # all three dampings on either side of every path change
        assert {l for K, l in lams if cliff - 2 <= K <= cliff + 3} == set(cases.LAMBDAS)


def test_bounds_inputs_clamp_where_they_claim():
    """x + dc* at least 10 % of the interval outside it, or well inside; never within 1e-6 of a bound"""
    for form, sizes in cases.SOLVE_SIZES.items():
        for K in sizes:
            for c in cases.cell(form, "bounds", K):
                tr = ref.truth(c)
                assert tr["clamped"] == c.claims["clamped"], c.name
                assert K < 3 or {-1, 0, 1} == set(tr["clamped"]), c.name
                assert K < 20 or (c.cols["dst2"] >= 0).any(), c.name
                for i in range(K):
                    lo, hi = mp.mpf(float(c.cols["lo"][i])), mp.mpf(float(c.cols["hi"][i]))
                    w, v = hi - lo, tr["cand"][i]
                    out = max(lo - v, v - hi) / w
                    assert (out >= mp.mpf("0.0999")) if tr["clamped"][i] else (out <= mp.mpf("-0.25")), (c.name, i, out)
                    assert min(abs(v - lo), abs(v - hi)) > mp.mpf(10) ** -6 * max(w, abs(v)), (c.name, i)


def test_the_two_routes_to_the_truth_agree():
    """mpmath.cholesky_solve against the refinement: every k_head case, k_solve's to K = 40 (seed 0), three sizes above"""
    worst = mp.mpf(0)
    todo = [c for K in cases.SOLVE_SIZES["k_head"] for f in cases.FAMILIES for c in cases.cell("k_head", f, K)]
    todo += [cases.solve_case("k_solve", f, K, 0) for K in range(1, 41) for f in cases.FAMILIES]
    todo += [cases.solve_case("k_solve", f, K, K & 1) for K in (47, 64, 127) for f in ("stiff", "damped")]
    for c in todo:
        a, b = ref.truth(c, "cholesky"), ref.truth(c, "refined")
        bot = max(abs(a["dc"][i]) * a["sdiag"][i] for i in range(c.K))
        if bot == 0:
            assert all(v == 0 for v in b["dc"]), c.name
            continue
        d = max(abs(a["dc"][i] - b["dc"][i]) * a["sdiag"][i] for i in range(c.K)) / bot
        worst = max(worst, d)
        assert d < mp.mpf(10) ** -36, (c.name, mp.nstr(d, 3))                  # 1e-40 in the residual x a condition number <= 1e8, with room
        S, rhs, _, _ = ref.system(c)
        assert ref.scaled_residual(S, rhs, a["dc"]) < mp.mpf(10) ** -40, c.name
    print("routes differ by at most", mp.nstr(worst, 3))


def test_the_yardstick_is_an_f64_cholesky():
    """against numpy's own solve on a well-conditioned case, and an error of the size f64 allows against the truth"""
    for K in (1, 7, 40, 90):
        c = cases.solve_case("k_solve", "scaled", K, 0)
        y, tr = ref.yardstick(c), ref.truth(c)
        S, rhs, _, _ = ref.system(c, float)
        np.testing.assert_allclose(y["dc"], np.linalg.solve(np.array(S), np.array(rhs)), rtol=1e-10)
        assert ref.dc_error(y["dc"], tr) < 64 * K * 2.0 ** -52 and ref.rel_error(y["mc"], tr["mc"]) < 64 * K * 2.0 ** -52


def _mp_pivots(S, upto):
    """the Cholesky pivots 0 .. upto of S in mpmath (S with finite entries up to there)"""
    L, piv = [[mp.mpf(0)] * (upto + 1) for _ in range(upto + 1)], []
    for j in range(upto + 1):
        d = S[j][j] - mp.fsum(L[j][k] ** 2 for k in range(j))
        piv.append(d)
        if j == upto or d <= 0:
            break
        r = mp.sqrt(d)
        for i in range(j + 1, upto + 1):
            L[i][j] = (S[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / r
    return piv


@pytest.mark.parametrize("form", list(cases.SOLVE_SIZES))
def test_not_pd_inputs_fail_at_the_stated_pivot(form):
    """every case with the yardstick; in mpmath up to K = 16 and at 33, 64 and 127: positive definite with margin up to the stated pivot,
    which is negative (-0.5 x what it was), exactly zero (the duplicated column), NaN or +inf"""
    for K in cases.SOLVE_SIZES[form]:
        cs = cases.not_pd_cases(form, K)
        assert [c.claims["kind"] for c in cs] == [k for k in cases.NOT_PD_KINDS for _ in (0, 1)]
        for c in cs:
            p, kind = c.claims["fails_at"], c.claims["kind"]
            _check_layout(c)
            assert (c.lam > 0) == c.claims["lm"] == (c.seed == 1)
            assert {"first": p == 0, "middle": p == K // 2, "last": p == K - 1}.get(kind, 0 <= p < K), c.name
            assert ref.yardstick(c) == {"failed_at": p}, (c.name, ref.yardstick(c))
            if K > 16 and K not in (33, 64, 127):
                continue
            S = ref.system(c)[0]
            piv = _mp_pivots(S, p)
            assert len(piv) == p + 1, (c.name, len(piv))
            for j in range(p):
                assert piv[j] > mp.mpf("1e-3") * S[j][j], (c.name, j)            # positive definite up to there, with margin
            if kind == "duplicate":
                assert piv[p] == 0, (c.name, piv[p])
                if p:
                    assert S[p][:p + 1] == S[p - 1][:p - 1] + [S[p - 1][p - 1]] * 2 and all(v == 1 for v in piv[:p]), c.name
            elif kind == "nan":
                assert mp.isnan(piv[p]), c.name
            elif kind == "inf":
                assert piv[p] == mp.inf, c.name
            else:
                assert piv[p] < 0 and abs(piv[p]) > mp.mpf("0.2") * abs(S[p][p]) * mp.mpf("1e-3"), (c.name, piv[p])


def test_backsub_inputs():
    seen = set()
    for c in cases.backsub_cases():
        seen.add((c.K, c.n_slots))
        K1 = c.K + 1
        assert c.pf.shape == (c.n_slots, ref.pf_size(c.K)) and c.dc.shape == (c.K,) and c.poses.shape == (c.n_slots, 6)
        assert (c.min_diag, c.max_diag) == (1e-6, 1e2) and (c.lam > 0) == (c.seed == 1)
        assert set(c.claims) == {"unobserved", "dC_below", "dC_above"} if c.n_slots >= 3 else len(c.claims) == 1
        tr, ya = ref.backsub_truth(c), ref.backsub_yardstick(c)
        for s in range(c.n_slots):
            dC = c.pf[s, 21 + 6 * K1 + 6:21 + 6 * K1 + 12]
            if c.claims.get("unobserved") == s:
                assert c.pf[s, 0] == 0.0 and tr[s] is None and ya[s] is None
                continue
            assert tr[s] is not None and (np.array([c.pf[s, i * (i + 1) // 2 + i] for i in range(6)]) > 0).all()
            if c.claims.get("dC_below") == s:
                assert (dC < c.min_diag).all()
            elif c.claims.get("dC_above") == s:
                assert (dC > c.max_diag).all()
            else:
                assert ((dC > c.min_diag) & (dC < 1e5)).all()
            assert ref.pose_error(ya[s][0], c.poses[s], tr[s][0]) < 1e-9 and ref.rel_error(ya[s][1], tr[s][1]) < 1e-9, (c.name, s)
    assert {k for k, _ in seen} == set(cases.BACKSUB_K) and {n for _, n in seen} == set(cases.BACKSUB_SLOTS)
    assert len(seen) == len(cases.BACKSUB_K) * len(cases.BACKSUB_SLOTS)
    assert {len(c.claims) for c in cases.backsub_cases() if c.n_slots == 1} == {1}
    assert {k for c in cases.backsub_cases() if c.n_slots == 1 for k in c.claims} == {"unobserved", "dC_below", "dC_above"}


def test_hooks_are_in_the_second_library_only():
    """not declared in include/ccal.h, not in _ffi.SYMBOLS, not exported by the product; a call without a context is refused"""
    product, legacy = C.CDLL(_ffi.LIB_PATH), C.CDLL(_ffi.LEGACY_LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "ccal.h")).read()
    for name in ("ccal_test_camera_solve", "ccal_test_backsub"):
        assert hasattr(legacy, name) and not hasattr(product, name)
        assert name not in hdr and name not in {n for n, _, _ in _ffi.SYMBOLS}
    none = C.POINTER(C.c_double)()
    fn = legacy.ccal_test_camera_solve
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_double] * 3 + [C.c_int,
                                                                                                                    C.c_void_p, C.c_void_p]
    assert fn(None, 0, 4, none, None, 40, 10, 0, 0, 0, None, None, None, None, 0.0, 0.0, 1.0, 0, None, None) == _ffi.ERR_INVALID_ARG
    fb = legacy.ccal_test_backsub
    fb.restype = C.c_int
    fb.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_double] * 3 + [C.c_int,
                                                                                                                            C.c_void_p]
    assert fb(None, 1, 4, None, None, 0, None, None, 0.0, 0.0, 1.0, 0, None) == _ffi.ERR_INVALID_ARG
