"""CPU: the exact reference of validation()'s statistics (tests/order_stats_ref.py) against brute force and against the oracle, and
every named case (tests/order_stats_cases.py) against the properties it claims.  The device side: tests/test_gpu_order_stats.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import order_stats_cases as cases
import order_stats_ref as ref

IDS = [c.name for c in cases.CASES]
FINITE_INPUT = [c.name for c in cases.CASES if "inf" not in c.name and "nan" not in c.name]
# (a NaN has no place in the oracle's std::sort: those cases are held to brute force's definition on the device side only)
FINITE_MEAN = [c.name for c in cases.CASES if c.claims["mean"] in ("finite", "zero", "exact") and "nan" not in c.name]


def test_case_names_are_unique_and_every_contested_case_has_both_forms():
    assert len(set(IDS)) == len(IDS)
    for stem in ("contested_m31", "contested_m20", "contested_m13", "contested_m9", "wide_first_digit", "edge_median_ones_k_zeros",
                 "edge_median_zeros_k_ones", "zero_at_median", "all_denormal", "terms_below_lsb", "terms_straddle_lsb", "exact_grid",
                 "inf_above_rank", "inf_at_rank", "nan_above_rank", "nan_at_rank", "out_of_range_at_rank", "ties_k_b_5_copies"):
        forms = {c.claims["form"] for c in cases.CASES if c.name.startswith(stem + "_n")}
        assert forms == {"one", "general"}, (stem, forms)


def test_no_case_leaves_the_input_contract():
    """values >= +0: no sign bit anywhere (-0.0 included)"""
    for c in cases.CASES:
        assert not (c.values().view(np.uint64) >> np.uint64(63)).any(), c.name


@pytest.mark.parametrize("name", IDS)
def test_case_has_the_properties_it_claims(name):
    assert cases.check_claims(cases.by_name(name)) == []


@pytest.mark.parametrize("name", FINITE_INPUT)
def test_reference_equals_brute_force(name):
    c = cases.by_name(name)
    r = c.ref()
    med, mean = ref.brute_force(c.values())
    assert int(np.float64(med).view(np.uint64)) == r.median_bits
    if r.mean_kind == "finite":
        assert mean == r.mean
    else:
        assert mean is None and r.mean_kind == "inf"


@pytest.mark.parametrize("name", FINITE_MEAN)
def test_reference_against_the_oracle(name, oracle):
    """oracle_validation_stats sorts and adds e / n99 in doubles.  Median: equal.  Mean: one rounding per term on either side
    (fl(e * fl(1 / n99)) here, fl(e / n99) there), recursive summation over n99 terms, the truncation of n99 terms to 2^-80:
    |oracle - S| <= (n99 + 2) 2^-53 S + n99 2^-80 with S the exact mean."""
    c = cases.by_name(name)
    r = c.ref()
    v = np.ascontiguousarray(c.values())
    a, m = C.c_double(), C.c_double()
    dp = C.POINTER(C.c_double)
    assert oracle.load().oracle_validation_stats(v.ctypes.data_as(dp), v.size, C.byref(a), C.byref(m)) == 0
    assert int(np.float64(m.value).view(np.uint64)) == r.median_bits
    S = r.mean
    bound = (r.n99 + 2) * Fraction(1, 1 << 53) * S + r.n99 * Fraction(1, 1 << 80)
    assert abs(Fraction(a.value) - S) <= bound, (a.value, float(S), float(bound))


def test_to_fixed_restates_the_conversion():
    b = lambda x: int(np.float64(x).view(np.uint64))
    assert ref.to_fixed(b(1.0)) == 1 << 80
    assert ref.to_fixed(b(2.0 ** -80)) == 1 and ref.to_fixed(b(np.nextafter(2.0 ** -80, 0.0))) == 0
    assert ref.to_fixed(b(1.5 * 2.0 ** -80)) == 1                               # a right shift drops bits
    assert ref.to_fixed(b(0.0)) == 0 and ref.to_fixed(1) == 0 and ref.to_fixed((1 << 52) - 1) == 0
    assert ref.to_fixed(b(np.nextafter(2.0 ** 40, 0.0))) == ((1 << 53) - 1) << 67
    assert ref.to_fixed(b(2.0 ** 40)) is None and ref.to_fixed(b(np.inf)) is None and ref.to_fixed(cases.QNAN) is None
    assert ref.to_fixed(b(-0.0)) is None and ref.to_fixed(b(-1.0)) is None
    # exponent field 0: the shift is 1 - 1075 + 80 = -994, far beyond 64 - a denormal term is 0 whatever its mantissa is taken
    # to be.  (So "denormals get the implicit bit" is NOT an observable change of the device conversion: no input tells it apart.)
    assert (1 - 1075 + ref.FRAC_BITS) <= -64


def test_fixed_sum_equals_the_sum_of_to_fixed():
    rng = np.random.default_rng(5)
    ex = rng.integers(1023 - 150, 1023 + 40, 4000, dtype=np.uint64)
    bits = (ex << np.uint64(52)) | rng.integers(0, 1 << 52, 4000, dtype=np.uint64)
    bits[:50] = rng.integers(0, 1 << 52, 50, dtype=np.uint64)                   # denormals, +0.0 among them
    bits[0] = 0
    assert ref.fixed_sum(bits) == sum(ref.to_fixed(int(x)) for x in bits)


def test_the_scale_literal_of_from_fixed_is_two_to_the_minus_80():
    assert float("8.271806125530277e-25") == 2.0 ** -80
    assert float("18446744073709551616.0") == 2.0 ** 64


def test_empty_99_percent_gives_zero():
    r = ref.reference(np.array([0.75]))
    assert (r.n99, r.mean, r.median_bits) == (0, 0, int(np.float64(0.75).view(np.uint64)))


def test_reference_refuses_values_outside_the_contract():
    for bad in (-1.0, -0.0):
        with pytest.raises(AssertionError):
            ref.reference(np.array([0.5, bad, 1.0]))


# The reference-side versions of two of the kernel mutants this suite was tried against (rank + 1 -> rank, keys < K -> keys <= K): a reference that is
# wrong in the same way must disagree with the right one on some case - else no device test could see that mutant.
def _mutant_mean(c, drop_one_copy=False, count_all_copies=False):
    r = c.ref()
    if r.mean_kind != "finite" or r.n99 == 0:
        return None
    kterm = ref.to_fixed(int(np.float64(np.uint64(r.k_bits).view(np.float64) * np.float64(r.inv)).view(np.uint64)))
    if drop_one_copy:                                   # rank + 1 copies -> rank copies
        return r.T - kterm
    if count_all_copies:                                # keys < K -> keys <= K: the copies beyond the rank come in as well
        total = int(np.count_nonzero(c.values().view(np.uint64) == np.uint64(r.k_bits)))
        return r.T + total * kterm
    return r.T


@pytest.mark.parametrize("kw", [{"drop_one_copy": True}, {"count_all_copies": True}])
def test_reference_side_mutants_are_visible(kw):
    seen = []
    for c in cases.CASES:
        t = _mutant_mean(c, **kw)
        if t is None:
            continue
        T = c.ref().T
        if abs(t - T) * (1 << 53) > 3 * T:              # beyond the device test's bound
            seen.append(c.name)
    assert len(seen) >= 20, seen
