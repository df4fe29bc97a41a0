"""CPU: the yardstick of the planar pose initialiser (tests/pose_init_ref.py) checked on its own, and the frames of
tests/pose_init_cases.py checked for what tests/test_gpu_pose_init.py relies on, before any kernel is held to either."""
import math

import numpy as np
import pytest

import pose_init_cases as cases
import pose_init_ref as ref

LD = ref.LD


def _exact_points(f):
    """The frame's corners and their normalised image points at its generating pose, in long double (no detection rounding)."""
    X = f["X"].astype(LD)
    pc = X @ f["R"].astype(LD).T + f["t"].astype(LD)
    return X, pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]


def _true_h(f):
    R, t = f["R"].astype(LD), f["t"].astype(LD)
    return np.array([R[0, 0], R[0, 1], t[0], R[1, 0], R[1, 1], t[1], R[2, 0], R[2, 1]]) / t[2]


def _noise_free():
    out = []
    for m in (cases.UCM, cases.KB4):
        out += cases.lane_frames(m)
    return out + cases.rotation_frames() + cases.conditioning_frames() + cases.degenerate_frames()[1] + [cases.count_frames(cases.EUCM)[-1]]


def test_solve_recovers_the_generating_pose():
    """Exact normalised points: the system is consistent, its solution is [r1 r2 t] / t_z of the generating pose.  Householder QR
    is backward stable - a relative perturbation of A of a small multiple of u, which a consistent system turns into
    kappa x that in h; the rows are short (5 non-zeros of 8 columns) and the 8 reflections touch 8 columns each, so the multiple
    is taken as 64 (8 x 8), not the worst-case m n.  The generating R is a float64 matrix, orthonormal to 1e-16 only: the pose is
    compared with the post-processing of the true h, which is what the estimator is defined to return."""
    worst = 0.0
    for f in _noise_free():
        X, xn, yn = _exact_points(f)
        s = ref.solve(X[:, 0], X[:, 1], xn, yn)
        h_true = _true_h(f)
        bound = 64 * s["kappa"] * ref.U_LD
        eh = float(np.abs(s["h"] - h_true).max() / np.abs(h_true).max())
        sums = (X[:, 0].sum(), X[:, 1].sum(), len(X))
        R, t = ref.pose_from_h(s["h"], *sums)
        Rt, tt = ref.pose_from_h(h_true, *sums)
        eR = float(np.abs(R - Rt).max())
        et = float(np.sqrt(((t - tt) ** 2).sum()) / np.sqrt((tt ** 2).sum()))
        worst = max(worst, max(eh, eR, et) / (s["kappa"] * ref.U_LD))
        assert eh <= bound and eR <= bound and et <= bound, (f["name"], eh, eR, et, bound)
        assert np.abs(s["R"] - f["R"]).max() < 1e-14 * max(1.0, s["kappa"])       # and the float64 copy it returns
    print(f"solve against the generating pose: worst error {worst:.3g} kappa u_longdouble")


def test_solve_agrees_with_fifty_digits():
    """The same systems (f32-rounded detections: not consistent any more) solved at 50 digits by mpmath, where it imports."""
    if not ref.have_mpmath():
        pytest.skip("mpmath is not importable: only this cross-check is left out")
    frames = cases.lane_frames(cases.EUCM)[:6] + cases.conditioning_frames() + cases.noisy_frames()[:3] + cases.degenerate_frames()[1]
    for f in frames:
        r = cases.reference(f)
        h = ref.solve_mp(r["A"], r["b"])
        e = float(np.abs(r["h"] - h).max() / np.abs(h).max())
        assert e <= 64 * r["kappa"] * ref.U_LD, (f["name"], e, r["kappa"])
        assert abs(r["min_rel_pivot"] / r["min_rel_pivot_mp"] - 1) < 1e-9, f["name"]


def test_unproject_inverts_the_projection():
    """Every valid test corner: the long-double inverse reproduces the normalised point of the generating pose to the f32 rounding
    of the detection (2^-24 x 512 px over ~190 px of focal length, amplified at most 10 x by the model's slope here)."""
    for f in cases.well_posed_frames():
        if "noisy" in f["name"]:
            continue
        xn, yn, valid = ref.unproject(f["model"], f["params"], f["uv"])
        assert sorted(np.nonzero(~valid)[0]) == sorted(f["invalid"]), f["name"]
        _, xe, ye = _exact_points(f)
        d = np.abs(np.stack([xn - xe, yn - ye])[:, valid].astype(np.float64)).max()
        assert d < 10 * 2.0 ** -24 * 512 / 190, (f["name"], d)


def test_opencv5_fixed_point_has_converged_on_every_test_corner():
    """The kernel's 25 fixed-point steps, in f64, against the converged inverse: 1e-14 on every OPENCV5 corner of the case list, so
    that the estimator's tests do not test that iteration."""
    n = 0
    for f in cases.all_frames():
        if f["model"] != cases.OPENCV5:
            continue
        xk, yk, vk = ref.unproject_kernel_f64(f["model"], f["params"], f["uv"])
        xn, yn, v = ref.unproject(f["model"], f["params"], f["uv"])
        assert vk.all() and v.all()
        d = max(np.abs(xk - xn.astype(np.float64)).max(), np.abs(yk - yn.astype(np.float64)).max())
        assert d <= 1e-14, (f["name"], d)
        fx, fy = ref._ocv5_forward(xk, yk, *f["params"][4:9])
        mx, my = (f["uv"].astype(np.float64) - f["params"][2:4]).T / f["params"][:2][:, None]
        assert (np.abs(fx - mx) + np.abs(fy - my)).max() < 1e-12       # the acceptance rule (1e-9) is three decades away
        n += len(xk)
    assert n > 1000


def test_kb4_newton_has_converged_on_every_test_corner():
    for f in cases.all_frames():
        if f["model"] != cases.KB4:
            continue
        xk, yk, vk = ref.unproject_kernel_f64(f["model"], f["params"], f["uv"])
        xn, yn, v = ref.unproject(f["model"], f["params"], f["uv"])
        assert vk.all() and v.all()
        d = max(np.abs(xk / xn.astype(np.float64) - 1).max(), np.abs(yk / yn.astype(np.float64) - 1).max())
        assert d <= 1e-14, (f["name"], d)


def test_no_test_corner_sits_on_a_validity_boundary():
    """Valid corners stay 1e-6 relative inside the radius at which their model stops returning a ray (and KB4's clear of the
    small-radius branch); the deliberately invalid ones lie beyond it by at least a factor of 2 in r^2."""
    for f in cases.all_frames():
        lim = cases.domain_r2_limit(f["model"], f["params"])
        m = (f["uv"].astype(np.float64) - f["params"][2:4]) / f["params"][:2]
        r2 = (m * m).sum(axis=1)
        bad = np.zeros(len(r2), dtype=bool)
        bad[list(f["invalid"])] = True
        if lim is not None:
            assert (r2[~bad] <= lim * (1 - 1e-6)).all(), f["name"]
            assert (r2[bad] >= 2 * lim).all(), f["name"]
        else:
            assert not bad.any()
        if f["model"] == cases.KB4:
            assert (np.sqrt(r2) > 1e-8 * (1 + 1e-6)).all(), f["name"]
        _, _, valid = ref.unproject(f["model"], f["params"], f["uv"])
        _, _, valid_k = ref.unproject_kernel_f64(f["model"], f["params"], f["uv"])
        assert np.array_equal(valid, ~bad) and np.array_equal(valid_k, ~bad), f["name"]


def test_domain_limit_is_where_the_rules_change():
    for model in (cases.UCM, cases.EUCM, cases.DIVISION, cases.KB4):
        p = cases.PARAMS[model]
        lim = cases.domain_r2_limit(model, p)
        for scale, want in ((1 - 1e-6, True), (1 + 1e-6, False)):
            uv = np.array([[p[2] + p[0] * math.sqrt(lim * scale), p[3]]])
            assert ref.unproject(model, p, uv)[2][0] == want, (model, scale)
            assert ref.unproject_kernel_f64(model, p, uv)[2][0] == want, (model, scale)


def test_pivots_fall_into_two_clusters_around_the_tolerance():
    """What the kernel's pivot rule relies on: every frame that spans the board plane has its smallest relative pivot at least
    100 x above PIVOT_TOL, every frame that does not has it at least 100 x below (exactly: at 50 digits where mpmath imports,
    else in long double; and as the f64 emulation of the kernel computes it), and PIVOT_TOL is 100 x above the rounding bound
    10 u of a computed pivot and a power of two."""
    tol = ref.PIVOT_TOL
    assert math.log2(tol) == round(math.log2(tol)) and tol >= 100 * 10 * ref.U_F64
    good = {}
    for f in cases.well_posed_frames():
        r = cases.reference(f, cases.min_points_of(f))
        if r is not None:
            good[f["name"]] = r["min_rel_pivot"]
    assert len(good) >= 100
    low = min(good, key=good.get)
    print(f"well-posed: smallest relative pivot {good[low]:.3g} ({low})")
    assert good[low] >= 100 * tol, (low, good[low])
    assert low == "origin-100m" and 1e-6 < good[low] < 1e-5            # the figure the kernel's comment and ccal.h quote
    worst = 0.0
    for f in cases.degenerate_frames()[0] + [cases.row_plus_one()]:
        assert cases.reference(f) is None, f["name"]
        xn, yn, v = ref.unproject(f["model"], f["params"], f["uv"])
        assert v.all()
        s = ref.solve(f["X"][:, 0], f["X"][:, 1], xn, yn)
        exact = s["min_rel_pivot_mp"] if ref.have_mpmath() else s["min_rel_pivot"]
        emu = cases.emulation(f, tol=0.0)["min_rel_pivot"]
        worst = max(worst, abs(exact), abs(s["min_rel_pivot"]), abs(emu))
        assert abs(exact) <= tol / 100 and abs(s["min_rel_pivot"]) <= tol / 100 and abs(emu) <= tol / 100, (f["name"], exact, emu)
        if f["name"] != "row-plus-one":                                # exactly rank-deficient: what is left is rounding, below 10 u
            assert abs(emu) <= 10 * ref.U_F64, (f["name"], emu)
    print(f"not spanning the plane: largest |relative pivot| {worst:.3g}")


def test_a_row_plus_one_corner_is_rank_deficient():
    """One row and ONE corner of the next: at exact detections the design has rank 7, so this L has no pose; it reaches rank 8 only
    through the f32 rounding of its detections (relative pivot 1e-14).  One row and TWO corners of the next is the smallest L
    that has one."""
    f = cases.row_plus_one()
    X, xn, yn = _exact_points(f)
    s = ref.solve(X[:, 0], X[:, 1], xn, yn)
    assert abs(s["min_rel_pivot"]) < 1e-15
    if ref.have_mpmath():
        assert abs(s["min_rel_pivot_mp"]) < 1e-30
    assert cases.reference(f) is None
    good = cases.degenerate_frames()[1]
    assert [g["name"] for g in good] == ["two-rows", "row-plus-two"]
    assert len(good[1]["X"]) == len(f["X"]) + 1
    for g in good:
        r = cases.reference(g)
        assert r is not None and r["min_rel_pivot"] > 1e-5 and np.abs(r["R"] - g["R"]).max() < 1e-3, g["name"]


def test_the_sign_only_pivot_test_lets_collinear_frames_through():
    """The defect this yardstick was written around, in the f64 emulation of the kernel: with `s > 0` a detected row, a column and
    two corners repeated come back as valid poses that are nowhere near the truth; with the relative rule none of them does."""
    slipped = {}
    for f in cases.degenerate_frames()[0] + [cases.e2e_row_frame()]:
        e = cases.emulation(f, tol=0.0)
        if e["used"]:
            slipped[f["name"]] = float(np.abs(e["R"] - f["R"]).max())
        fixed = cases.emulation(f)
        assert fixed["used"] == 0 and not fixed["pose"].any(), f["name"]
    print("sign-only pivot test, poses returned:", {k: round(v, 2) for k, v in slipped.items()})
    assert {"row-noise1", "column-noise1", "row-e2e"} <= set(slipped), slipped
    assert min(slipped.values()) > 0.1


def test_every_quaternion_branch_decides_a_frame():
    want = {"rot-zero": (0, False), "rot-1e-9": (0, False),
            "rot-pi-x": (1, False), "rot-pi-minus-x": (1, True), "rot-pi-y": (2, False), "rot-pi-minus-y": (2, True),
            "rot-pi-z": (3, False), "rot-pi-minus-z": (3, True)}
    seen = set()
    for f in cases.rotation_frames():
        e = cases.emulation(f)
        assert e["used"] == 144, f["name"]
        if f["name"] in want:
            assert (e["branch"], e["flipped"]) == want[f["name"]], (f["name"], e["branch"], e["flipped"])
        elif f["name"] == "rot-2pi/3-111":                      # trace = R00 = R11 = R22 = 0: a four-way tie that rounding decides
            assert e["flipped"] is False
        else:                                                   # about (1, 1, 0): R00 = R11, rounding picks x or y
            assert e["branch"] in (1, 2) and e["flipped"] == ("minus" in f["name"]), (f["name"], e["branch"], e["flipped"])
        seen.add((e["branch"], e["flipped"]))
        assert np.linalg.norm(e["pose"][:3]) <= np.pi + 1e-12
        assert np.abs(e["R"] - f["R"]).max() < 1e-6
    assert {b for b, _ in seen} == {0, 1, 2, 3} and {(1, True), (2, True), (3, True)} <= seen


def test_the_count_of_valid_corners():
    for model in (cases.EUCM, cases.DIVISION):
        fr = cases.count_frames(model)
        for f in fr[:3]:
            assert cases.reference(f) is None and cases.emulation(f)["used"] == 0
            assert cases.reference(f, 4)["used"] == 9
        for f in fr[3:6]:
            assert cases.reference(f)["used"] == 10 and cases.emulation(f)["used"] == 10
        assert [cases.reference(f)["used"] for f in fr[6:9]] == [129, 129, 127]
        assert cases.reference(fr[9]) is None and cases.reference(fr[9], 4)["used"] == 4
        for f in fr[3:]:
            r = cases.reference(f, 4)
            assert np.abs(r["R"] - f["R"]).max() < 1e-4 * max(1.0, r["kappa"] / 100), f["name"]


def test_tolerance_factor_follows_its_rule():
    """F = 4 x the worst err / (kappa^2 u) of the f64 emulation of the kernel against the yardstick, rounded up to a power of two."""
    worst, name = 0.0, None
    for f in cases.well_posed_frames():
        r = cases.reference(f, cases.min_points_of(f))
        if r is None:
            continue
        e = cases.emulation(f, cases.min_points_of(f))
        assert e["used"] == r["used"], f["name"]
        ratio = max(cases.pose_errors(e["R"], e["t"], r))
        if ratio > worst:
            worst, name = ratio, f["name"]
    print(f"emulate_f64 against solve: worst err / (kappa^2 u) = {worst:.3g} ({name}); F = {cases.F}")
    assert cases.F == 2.0 ** math.ceil(math.log2(4 * worst)), (worst, cases.F)


def test_the_pose_has_the_corners_in_front_whatever_the_origins_depth():
    """h33 = 1 ties the homography's sign to the depth of the board's ORIGIN.  The board whose origin is 100 m away in its own plane
    is in view with that origin behind the camera's plane (t_z < 0): the pose is -H's, the one with positive summed depth."""
    f = next(f for f in cases.conditioning_frames() if f["name"] == "origin-100m")
    assert f["t"][2] < 0 and ((f["X"].astype(np.float64) @ f["R"].T + f["t"])[:, 2] > 0.05).all()
    for got in (cases.reference(f), cases.emulation(f)):
        assert np.abs(got["R"] - f["R"]).max() < 1e-3 and np.abs(got["t"] - f["t"]).max() < 1e-3 * np.linalg.norm(f["t"])
