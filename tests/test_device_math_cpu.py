"""CPU: the named inputs of tests/device_math_cases.py claim what they say, and the mpmath yardstick of tests/device_math_ref.py
is right on its own (against math / numpy, and for SO3 against expm and the identities that pin J_l).  No GPU, no library."""
import math

import mpmath as mp
import numpy as np
import pytest

import device_math_cases as cases
import device_math_ref as ref

NAMES = [c.name for c in cases.LISTS]


def test_every_op_has_lists_and_names_are_unique():
    assert len(set(NAMES)) == len(NAMES)
    for op in ref.OPS:
        assert cases.of_op(op), op
    for c in cases.LISTS:
        v = c.inputs()
        assert v.ndim == 2 and v.shape[1] == ref.N_IN[c.op] and 0 < v.shape[0] <= 5000, (c.name, v.shape)
        assert np.isfinite(v).all(), c.name
        assert c.why
        np.testing.assert_array_equal(v, np.asarray(c.build(np.random.default_rng(c.seed))).reshape(v.shape))    # seeded


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_inside_the_contract(name):
    c = cases.by_name(name)
    v = c.inputs()
    if c.op == "RCP":
        assert (np.abs(v) >= 2.0 ** -500).all() and (np.abs(v) <= 2.0 ** 500).all()
        assert (v > 0).any() and (v < 0).any()                                  # both signs
    elif c.op == "SQRT_RSQRT":
        assert (v >= 2.0 ** -500).all() and (v <= 2.0 ** 500).all()
    elif c.op == "SINCOS":
        assert (np.abs(v) <= 1e5).all()
    elif c.op == "ATAN2_POS":
        assert (v[:, 0] > 0).all()
    elif c.op == "SO3":
        n = np.sqrt((v.astype(np.longdouble) ** 2).sum(1))
        assert (n <= 40.0).all()
    elif not c.claims.get("outside"):
        s, d = v[:, 0], v[:, 1]
        assert (d > 0).all() and (s > d * d).all()
        with mp.workdps(ref.DPS):
            assert all(mp.mpf(float(a)) <= mp.mpf(10) ** 12 * mp.mpf(float(b)) ** 2 for a, b in v)
    else:
        s, d = v[:, 0], v[:, 1]
        assert ((d <= 0) | (s == d * d)).all()                                  # the pinned cases outside the contract


def test_exponent_range_and_the_seed_table_neighbours():
    for op_prefix in ("rcp", "sqrt"):
        e = np.frexp(np.abs(cases.by_name(f"{op_prefix}_exponents").inputs()[:, 0]))[1] - 1
        assert set(range(-500, 500)) <= set(e.tolist())
        p = np.abs(cases.by_name(f"{op_prefix}_pow2").inputs()[:, 0])
        m, ex = np.frexp(p)
        assert set(range(-500, 501)) <= set((ex[m == 0.5] - 1).tolist())
        assert np.nextafter(1.0, 2.0) in p and np.nextafter(1.0, 0.0) in p
        m = np.frexp(np.abs(cases.by_name(f"{op_prefix}_mantissa_steps").inputs()[:, 0]))[0] * 2        # [1, 2)
        for target in (1.0, 2.0, math.sqrt(2.0)):
            near = np.abs(m - target) <= 9 * 2.0 ** -52
            assert near.sum() >= 8 * 9, target
        assert (m < math.sqrt(2.0)).any() and (m > math.sqrt(2.0)).any() and (m == 1.0).any()


@pytest.mark.parametrize("name", [c.name for c in cases.LISTS if "straddle" in c.claims])
def test_seam_lists_straddle_their_seam(name):
    c = cases.by_name(name)
    v = c.inputs()
    side = np.asarray(c.claims["straddle"](v))
    assert side.any() and (~side).any()
    if c.op == "ATAN2_POS":
        ratio = v[:, 0] / np.abs(v[:, 1])
        assert (np.abs(ratio / c.claims["ratio"] - 1) < 8 * 2.0 ** -52).all()
        for neg in (False, True):                                               # both sides at both signs of z
            m = (v[:, 1] < 0) == neg
            assert side[m].any() and (~side[m]).any()
    else:
        t2 = (v ** 2).sum(1)
        assert (np.abs(t2 / cases.SO3_SERIES_T2 - 1) < 16 * 2.0 ** -52).all()


def test_atan2_lists_reach_every_octant_case():
    v = cases.by_name("atan2_log").inputs()
    big, sel = cases.sel_of(v)
    neg = v[:, 1] < 0
    k = np.where(sel, np.where(neg, 3, 1), np.where(big, 2, np.where(neg, 4, 0)))
    assert set(k.tolist()) == {0, 1, 2, 3, 4}
    assert (sel & big & neg).any() and (sel & ~big & neg).any() and (sel & big & ~neg).any() and (sel & ~big & ~neg).any()
    z = cases.by_name("atan2_z_zero").inputs()[:, 1]
    assert (z == 0).sum() >= 2 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert (np.abs(z[z != 0]) == np.finfo(np.float64).tiny).all()
    r = cases.by_name("atan2_kb4_threshold").inputs()[:, 0]
    assert (r == np.nextafter(1e-8, 1.0)).all()
    e = cases.by_name("atan2_extreme_ratio").inputs()
    lr = np.log2(e[:, 0] / np.abs(e[:, 1]))
    assert (lr > 198).any() and (lr < -198).any() and (np.abs(lr) > 198).all() and (e[:, 1] < 0).any()


def test_so3_seam_generic_is_at_the_seam():
    v = cases.by_name("so3_seam_generic").inputs()
    assert (np.abs((v ** 2).sum(1) / cases.SO3_SERIES_T2 - 1) < 16 * 2.0 ** -52).all()
    assert ((cases.by_name("so3_small").inputs() ** 2).sum(1) < cases.SO3_SERIES_T2).all()
    assert ((cases.by_name("so3_above_seam").inputs() ** 2).sum(1) > cases.SO3_SERIES_T2).all()
    z = cases.by_name("so3_zero_components").inputs()
    nz = (z == 0).sum(1)
    assert set(nz.tolist()) == {1, 2}
    a = cases.by_name("so3_angles").inputs()
    t = np.sqrt((a ** 2).sum(1))
    for ang in cases.SO3_ANGLES:
        assert (np.abs(t - ang) < 1e-13 * max(1.0, ang)).sum() == 23, ang
    assert (cases.by_name("so3_zero").inputs() == 0).all()


@pytest.mark.parametrize("name", [c.name for c in cases.LISTS if "k_of" in c.claims or "tie" in c.claims])
def test_sincos_lists_fall_in_the_k_they_name(name):
    c = cases.by_name(name)
    x = c.inputs()[:, 0]
    with mp.workdps(ref.DPS):
        q = [mp.mpf(float(a)) * 2 / mp.pi for a in x]
        if "k_of" in c.claims:
            k = c.claims["k_of"](c.inputs())
            assert len(k) == len(x)
            for qi, ki, xi in zip(q, k, x):
                assert mp.nint(qi) == int(ki), (xi, ki)
                assert abs(mp.mpf(float(xi)) - int(ki) * mp.pi / 2) <= 2.5 * float(np.spacing(abs(xi))), (xi, ki)
            assert len(set(int(a) for a in k)) >= 30 and (min(k) <= -8 or max(k) >= 63661)
        else:
            for qi, xi in zip(q, x):
                frac = abs(qi - mp.floor(qi) - mp.mpf(1) / 2)                  # distance from a tie, in units of pi/2
                assert frac * mp.pi / 2 <= 4.5 * float(np.spacing(abs(xi))), xi


def test_sincos_dense_reaches_the_quadrants_the_suite_never_did():
    k = np.rint(cases.by_name("sincos_dense").inputs()[:, 0] * (2 / np.pi)).astype(int)
    assert set(range(0, 9)) <= set(k.tolist())
    k = np.rint(cases.by_name("sincos_coarse").inputs()[:, 0] * (2 / np.pi)).astype(int)
    assert set(range(-8, 9)) <= set(k.tolist())


def test_huber_edges():
    for kk in (0, 1, 2):
        v = cases.by_name(f"huber_edge_{kk}").inputs()
        assert sorted(v[:, 1].tolist()) == sorted(cases.HUBER_DELTAS)
        for s, d in v:
            assert s == cases.step(d * d, kk) and (s > d * d) == (kk > 0)
    v = cases.by_name("huber_log").inputs()
    assert (v[:, 0] / v[:, 1] ** 2).max() > 1e11 and (v[:, 0] / v[:, 1] ** 2 - 1).min() < 1e-13
    for c in cases.LISTS:
        if c.claims.get("exact_one"):
            assert all(r[0] == 1 for r in c.reference()), c.name


# ---- the yardstick on its own -----------------------------------------------------------------------------------------------
def _libm(op, v):
    if op == "RCP":
        return (1.0 / v[:, 0])[:, None]
    if op == "SQRT_RSQRT":
        return np.stack([np.sqrt(v[:, 0]), 1.0 / np.sqrt(v[:, 0])], 1)
    if op == "SINCOS":
        return np.stack([np.sin(v[:, 0]), np.cos(v[:, 0])], 1)
    if op == "ATAN2_POS":
        return np.array([math.atan2(r, z) for r, z in v])[:, None]
    s, d = v[:, 0], v[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((d > 0) & (s > d * d), np.sqrt(d / np.sqrt(s)), 1.0)[:, None]


@pytest.mark.parametrize("name", [c.name for c in cases.LISTS if c.op != "SO3"])
def test_yardstick_agrees_with_libm_to_2_ulp(name):
    c = cases.by_name(name)
    got, want = _libm(c.op, c.inputs()), c.reference()
    worst = max(ref.ulps(g, w) for grow, wrow in zip(got, want) for g, w in zip(grow, wrow))
    assert worst <= 2.0, worst


def test_ulps_measure():
    with mp.workdps(ref.DPS):
        one = mp.mpf(1)
        assert ref.ulps(1.0, one) == 0.0
        assert ref.ulps(1.0 + 2.0 ** -52, one) == 1.0
        assert ref.ulps(1.0 - 2.0 ** -53, one) == 0.5                       # the spacing of the reference's binade, [1, 2)
        assert ref.ulps(0.75, mp.mpf(0.75) + mp.mpf(2) ** -54) == 0.5       # [0.5, 1): spacing 2^-53
        assert ref.ulps(float("nan"), one) == math.inf
        assert ref.spacing(one * 2 - mp.mpf(2) ** -80) == 2.0 ** -51        # rounds to 2.0: the correctly rounded reference's binade


@pytest.mark.parametrize("name", [c.name for c in cases.LISTS if c.op == "SO3"])
def test_so3_yardstick_is_a_rotation_its_expm_and_its_left_jacobian(name):
    c = cases.by_name(name)
    v = c.inputs()
    pick = np.unique(np.linspace(0, len(v) - 1, 40).astype(int))           # expm at 60 digits is the slow part
    rows = c.reference()
    with mp.workdps(ref.DPS):
        tol = mp.mpf(10) ** -30
        for i, (w, row) in enumerate(zip(v, rows)):
            wm = [mp.mpf(float(a)) for a in w]
            R, J, W = mp.matrix(3, 3), mp.matrix(3, 3), ref.skew(wm)
            for a in range(3):
                for b in range(3):
                    R[a, b], J[a, b] = row[3 * a + b], row[9 + 3 * a + b]
            assert mp.norm(R * R.T - mp.eye(3), mp.inf) < tol and abs(mp.det(R) - 1) < tol
            # J_l W = R - I fixes J_l on the plane across w, J_l w = w along it: together all of J_l
            scale = 1 + mp.norm(W, mp.inf)
            assert mp.norm(J * W - (R - mp.eye(3)), mp.inf) < tol * scale
            assert mp.norm(J * mp.matrix(wm) - mp.matrix(wm), mp.inf) < tol * scale
            if i in pick:
                assert mp.norm(mp.expm(W, method="taylor") - R, mp.inf) < tol
    if c.claims.get("identity"):
        assert all([float(a) for a in row] == [1, 0, 0, 0, 1, 0, 0, 0, 1] * 2 for row in rows)
