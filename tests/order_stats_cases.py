"""Named inputs for the radix select of validation() (TEST INFRASTRUCTURE: tests/test_order_stats_cpu.py checks every case's
claimed properties against tests/order_stats_ref.py, tests/test_gpu_order_stats.py feeds the cases to the device).

Every case has a fixed seed and a dict of the properties it claims - why it is in the list.  Keys are built from bit patterns
(`view(np.uint64)`) where a digit has to be hit on purpose.  The values are handed over in a seeded random order.

INPUT CONTRACT: values are >= +0 (errors are norms).  Negative values and -0.0 are outside the contract and no case holds one.

Claims (all checked by `check_claims` from the reference's counts, which come from the sorted keys):
    n99                      n * 99 // 100
    form                     "one" (n <= 8192: the one-launch kernel) or "general" (a launch per digit)
    workgroups               of the general form: min(256, ceil(n / 2048))
    contested: p             pass p, at BOTH ranks: >= 64 occupied bins over >= 2 lanes' ranges, and the lane that holds the rank
                             has >= 2 occupied bins in front of the answer (the shuffle scan and the in-register walk both decide)
    single_before: p         passes < p see one candidate key at both ranks
    pass0_bins_min, pass1_candidates_min
    median_bits, k_bits      the bit patterns at the two ranks
    ones: t / zeros: t       the key at rank t has digits 1..5 all ones (lane 63, last bin) / all zeros (lane 0, first bin)
    copies, below            copies of K at or below the 99 % rank, keys below K
    median_copies_min        copies of the median key
    mean                     "finite" | "zero" (T == 0) | "inf" | "nan" | "exact" (inv, every term and the sum are exact)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import order_stats_ref as R

ONE_MAX = 8192                       # kSelOneMax
K0 = 0x3FD0000000000000              # bits of 0.25
QNAN = 0x7FF8000000000000            # the positive quiet NaN
INF = float("inf")


def _f(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def _b(x) -> int:
    return int(np.float64(x).view(np.uint64))


@dataclass
class Case:
    name: str
    seed: int
    build: object                    # rng -> float64 array (any order)
    claims: dict = field(default_factory=dict)

    def values(self) -> np.ndarray:
        if self.name not in _VALUES:
            rng = np.random.default_rng(self.seed)
            v = np.ascontiguousarray(self.build(rng), dtype=np.float64)
            v = v[rng.permutation(v.size)]
            v.setflags(write=False)
            _VALUES[self.name] = v
        return _VALUES[self.name]

    def ref(self) -> R.Ref:
        if self.name not in _REFS:
            _REFS[self.name] = R.reference(self.values())
        return _REFS[self.name]


_VALUES: dict = {}
_REFS: dict = {}
CASES: list = []


def _add(name, seed, build, **claims):
    CASES.append(Case(name, seed, build, claims))


def by_name(name) -> Case:
    return next(c for c in CASES if c.name == name)


def _form(n):
    return {"form": "one"} if n <= ONE_MAX else {"form": "general", "workgroups": min(256, (n + 2047) // 2048)}


# ---- sizes: distinct random values in (0, 4) px -------------------------------------------------------------------------
def _distinct(n):
    def build(rng):
        v = np.unique(rng.uniform(0.0, 4.0, n + 64))
        v = v[v > 0.0]
        assert v.size >= n
        return rng.permutation(v)[:n]
    return build


for _n, _n99 in ((1, 0), (2, 1), (3, 2), (99, 98), (100, 99), (101, 99), (199, 197), (200, 198), (1023, 1012), (1024, 1013),
                 (1025, 1014), (8191, 8109), (8192, 8110), (8193, 8111), (10241, 10138), (16550, 16384), (600001, 594000)):
    _add(f"size_{_n}", 1000 + _n % 997, _distinct(_n), n99=_n99, mean="finite", **_form(_n))


# ---- contested digits: K0 + U[0, 2^m) -----------------------------------------------------------------------------------
def _contested(n, m):
    return lambda rng: _f(np.uint64(K0) + rng.integers(0, 1 << m, n, dtype=np.uint64))


# (m, contested pass, n of the one-launch form, its seed, n of the general form, its seed); the seeds are the first ones at
# which the claimed property holds at both ranks (tests/test_order_stats_cpu.py keeps checking it)
for _m, _p, _n1, _s1, _n2, _s2 in ((31, 3, 8000, 0, 12000, 0), (20, 4, 8000, 0, 12000, 0), (13, 5, 8000, 6, 12000, 0),
                                   (9, 5, 8000, 1, 12000, 2)):
    for _n, _s in ((_n1, _s1), (_n2, _s2)):
        extra = {"copies_min": 2, "median_copies_min": 2} if _m == 9 else {}
        _add(f"contested_m{_m}_n{_n}", _s, _contested(_n, _m), contested=_p, single_before=_p if _m != 13 else 4,
             mean="finite", **extra, **_form(_n))


# ---- a wide first digit: log-uniform from the denormal range up to 2^39 ---------------------------------------------------
def _log_uniform(n):
    def build(rng):
        ex = rng.integers(0, 1023 + 39, n, dtype=np.uint64)              # exponent field 0 (denormal) .. 2^38's
        man = rng.integers(0, 1 << 52, n, dtype=np.uint64)
        return _f((ex << np.uint64(52)) | man)
    return build


for _n, _s in ((8000, 0), (20000, 0)):
    _add(f"wide_first_digit_n{_n}", _s, _log_uniform(_n), pass0_bins_min=501, pass1_candidates_min=4, pass1_occupied_min=4,
         mean="finite", **_form(_n))


# ---- digit edges ----------------------------------------------------------------------------------------------------------
def _cluster(center_bits, width):
    return np.arange(center_bits - width, center_bits + width + 1, dtype=np.uint64)


def _edges(n, med_bits, k_bits, width=40):
    """The key at the median rank is med_bits, the key at the 99 % rank k_bits; each sits in a run of 2 * width + 1 consecutive
    bit patterns (neighbours one ulp apart); random filler elsewhere."""
    def build(rng):
        n99 = n * 99 // 100
        cm, ck = _cluster(med_bits, width), _cluster(k_bits, width)
        lo_m, hi_k = _f(cm[0]), _f(ck[-1])
        n_low = n // 2 - width                                       # in front of the median's run
        n_mid = (n99 - 1 - width) - (n // 2 + width + 1)              # between the runs
        n_top = n - (n99 - 1 + width + 1)
        assert min(n_low, n_mid, n_top) >= 0
        low = rng.uniform(0.0, float(lo_m) * 0.99, n_low)
        mid = rng.uniform(float(_f(cm[-1])) * 1.01, float(_f(ck[0])) * 0.99, n_mid)
        top = rng.uniform(float(hi_k) * 1.01, 4.0, n_top)
        return np.concatenate([low, _f(cm), mid, _f(ck), top])
    return build


ONES_2 = _b(np.nextafter(2.0, 0.0))          # 0x3FFFFFFFFFFFFFFF: digits 1..5 all ones
ZEROS_2 = _b(2.0)                            # 0x4000000000000000: digits 1..5 all zeros
ONES_H = _b(np.nextafter(0.5, 0.0))          # 0x3FDFFFFFFFFFFFFF
ZEROS_H = _b(0.5)                            # 0x3FE0000000000000
for _n in (4001, 9001):
    _add(f"edge_median_ones_k_zeros_n{_n}", 7, _edges(_n, ONES_H, ZEROS_2), median_bits=ONES_H, k_bits=ZEROS_2, ones=0, zeros=1,
         mean="finite", **_form(_n))
    _add(f"edge_median_zeros_k_ones_n{_n}", 8, _edges(_n, ZEROS_H, ONES_2), median_bits=ZEROS_H, k_bits=ONES_2, zeros=0, ones=1,
         mean="finite", **_form(_n))


def _zero_median(n):
    def build(rng):
        nz = n // 2 + 1                                              # +0.0 up to and including the median rank
        den = _f(np.arange(1, 41, dtype=np.uint64))                  # the smallest denormals right above
        rest = rng.uniform(0.01, 2.0, n - nz - den.size)
        return np.concatenate([np.zeros(nz), den, rest])
    return build


for _n in (101, 9001):
    _add(f"zero_at_median_n{_n}", 9, _zero_median(_n), median_bits=0, median_copies_min=_n // 2 + 1, mean="finite", **_form(_n))


# ---- ties at the ranks ------------------------------------------------------------------------------------------------------
A, B = 0.3, 0.7


def _two(na, nb):
    return lambda rng: np.concatenate([np.full(na, A), np.full(nb, B)])


for _scale in (1, 10):                                               # n = 1000 (n99 = 990) and n = 10 000 (n99 = 9900)
    _n = 1000 * _scale
    _add(f"ties_k_b_5_copies_n{_n}", 1, _two(985 * _scale, 15 * _scale), n99=990 * _scale, k_bits=_b(B), copies=5 * _scale,
         below=985 * _scale, median_bits=_b(A), mean="finite", **_form(_n))
    _add(f"ties_k_a_all_copies_n{_n}", 1, _two(990 * _scale, 10 * _scale), k_bits=_b(A), copies=990 * _scale, below=0,
         median_bits=_b(A), mean="finite", **_form(_n))
    _add(f"ties_k_b_1_copy_n{_n}", 1, _two(990 * _scale - 1, 10 * _scale + 1), k_bits=_b(B), copies=1, below=990 * _scale - 1,
         median_bits=_b(A), mean="finite", **_form(_n))
    _add(f"ties_median_last_a_n{_n}", 1, _two(_n // 2 + 1, _n // 2 - 1), median_bits=_b(A), k_bits=_b(B), mean="finite", **_form(_n))
    _add(f"ties_median_first_b_n{_n}", 1, _two(_n // 2, _n // 2), median_bits=_b(B), k_bits=_b(B), mean="finite", **_form(_n))
for _n in (1, 5000, 9000):
    _add(f"all_equal_n{_n}", 1, (lambda n: lambda rng: np.full(n, 0.4375))(_n), median_bits=_b(0.4375),
         copies=_n * 99 // 100, below=0, mean="finite", **_form(_n))


# ---- fixed-point edges --------------------------------------------------------------------------------------------------------
def _denormals(n):
    return lambda rng: _f(rng.integers(1, 1 << 52, n, dtype=np.uint64))


def _pow2_range(n, lo, hi):
    """log-uniform in [2^lo, 2^hi)"""
    def build(rng):
        ex = rng.integers(1023 + lo, 1023 + hi, n, dtype=np.uint64)
        return _f((ex << np.uint64(52)) | rng.integers(0, 1 << 52, n, dtype=np.uint64))
    return build


def _one_big(n, big, above):
    """small values, `big` as the key at the 99 % rank with the double right below it in front, `above` beyond the rank"""
    def build(rng):
        n99 = n * 99 // 100
        return np.concatenate([rng.uniform(0.01, 2.0, n99 - 2), [np.nextafter(big, 0.0), big], np.full(n - n99, above)])
    return build


def _grid(n):
    return lambda rng: rng.permutation(1 << 20)[:n].astype(np.float64) / 1024.0


for _n in (3000, 9000):
    _add(f"all_denormal_n{_n}", 11, _denormals(_n), mean="zero", **_form(_n))
    # n99 >= 2^11: values below 2^-70 scale to terms below 2^-80 - every term is exactly 0
    _add(f"terms_below_lsb_n{_n}", 12, _pow2_range(_n, -100, -70), mean="zero", **_form(_n))
    # terms of 2^-86 .. 2^-52: the conversion drops up to all of a term's 53 bits
    _add(f"terms_straddle_lsb_n{_n}", 13, _pow2_range(_n, -74, -40), mean="finite", truncating=True, **_form(_n))
BIG = float(np.nextafter(2.0 ** 40, 0.0))


def _largest_in_range(n99):
    """the largest double whose term fl(v * fl(1 / n99)) is still below 2^40"""
    inv, v = 1.0 / n99, 2.0 ** 40 * n99
    while v * inv >= 2.0 ** 40:
        v = float(np.nextafter(v, 0.0))
    return v


for _n in (200, 10000):
    _n99 = _n * 99 // 100
    # a value just under 2^40 below the rank, far larger ones beyond it
    _add(f"value_under_2p40_n{_n}", 14, _one_big(_n, BIG, 2.0 ** 45), k_bits=_b(BIG), copies=1, mean="finite",
         **_form(_n))
    # ... and a value whose SCALED term is the last double under 2^40 (the next one up is bad: out_of_range_* below)
    _add(f"term_under_2p40_n{_n}", 15, _one_big(_n, _largest_in_range(_n99), 2.0 ** 60), copies=1, mean="finite",
         term_limit=True, **_form(_n))
for _n, _n99 in ((4138, 4096), (16550, 16384)):
    _add(f"exact_grid_n{_n}", 16, _grid(_n), n99=_n99, mean="exact", **_form(_n))


# ---- non-finite and out of range: what the kernel documents ---------------------------------------------------------------------
def _top(n, n_top, top_bits):
    """n - n_top random values in (0, 2), then n_top copies of the bit pattern top_bits (the largest keys)"""
    def build(rng):
        return np.concatenate([rng.uniform(0.01, 2.0, n - n_top), _f(np.full(n_top, top_bits, dtype=np.uint64))])
    return build


for _n in (1000, 10000):
    _above, _at = _n // 200, _n // 100 + _n // 200          # 0.5 % of the keys: beyond the rank; 1.5 %: reach down to it
    _add(f"inf_above_rank_n{_n}", 21, _top(_n, _above, R.INF_BITS), mean="finite", **_form(_n))
    _add(f"inf_at_rank_n{_n}", 22, _top(_n, _at, R.INF_BITS), k_bits=R.INF_BITS, mean="inf", **_form(_n))
    _add(f"out_of_range_at_rank_n{_n}", 23, _top(_n, _at, _b(2.0 ** 41 * (_n * 99 // 100))), mean="inf", **_form(_n))
    _add(f"nan_above_rank_n{_n}", 24, _top(_n, _above, QNAN), mean="finite", **_form(_n))
    _add(f"nan_at_rank_n{_n}", 25, _top(_n, _at, QNAN), k_bits=QNAN, mean="nan", **_form(_n))


def _inf_below_nan(n):
    def build(rng):
        k = n // 100 + n // 200
        return np.concatenate([rng.uniform(0.01, 2.0, n - 2 * k), np.full(k, INF), _f(np.full(k, QNAN, dtype=np.uint64))])
    return build


for _n in (1000, 10000):
    _add(f"nan_at_rank_inf_below_n{_n}", 27, _inf_below_nan(_n), k_bits=QNAN, mean="nan", **_form(_n))
_add("out_of_range_below_rank_n1000", 26,
     lambda rng: np.concatenate([rng.uniform(0.01, 2.0, 980), [2.0 ** 41 * 990], np.full(19, 2.0 ** 62)]), mean="inf", **_form(1000))


# ---- claims ---------------------------------------------------------------------------------------------------------------------
def check_claims(case: Case) -> list:
    """The claims of `case` that do not hold (empty: all hold)."""
    ref, c, bad = case.ref(), case.claims, []

    def want(ok, what):
        if not ok:
            bad.append(f"{case.name}: {what}")

    n = ref.n
    want(c["form"] == ("one" if n <= ONE_MAX else "general"), "form")
    if "workgroups" in c:
        want(c["workgroups"] == min(256, -(-n // 2048)), "workgroups")
    if "n99" in c:
        want(ref.n99 == c["n99"], f"n99 {ref.n99}")
    ranks = range(2 if ref.n99 else 1)
    if "contested" in c:
        p = c["contested"]
        for t in ranks:
            pc = ref.passes[p][t]
            want(pc.occupied >= 64 and pc.lanes >= 2 and pc.before_in_lane >= 2, f"pass {p} rank {t}: {pc}")
    if "single_before" in c:
        for p in range(c["single_before"]):
            for t in ranks:
                want(ref.passes[p][t].occupied == 1, f"pass {p} rank {t} occupied {ref.passes[p][t].occupied}")
    if "pass0_bins_min" in c:
        want(ref.passes[0][0].occupied >= c["pass0_bins_min"], f"pass 0 occupied {ref.passes[0][0].occupied}")
    for t in ranks:
        if "pass1_candidates_min" in c:
            want(ref.passes[1][t].candidates >= c["pass1_candidates_min"], f"pass 1 rank {t} candidates {ref.passes[1][t].candidates}")
        if "pass1_occupied_min" in c:
            want(ref.passes[1][t].occupied >= c["pass1_occupied_min"], f"pass 1 rank {t} occupied {ref.passes[1][t].occupied}")
    if "median_bits" in c:
        want(ref.median_bits == c["median_bits"], f"median {ref.median_bits:#x}")
    if "k_bits" in c:
        want(ref.k_bits == c["k_bits"], f"K {ref.k_bits:#x}")
    for key, lane_of, bin_of in (("ones", lambda per: 63, lambda per: per - 1), ("zeros", lambda per: 0, lambda per: 0)):
        if key in c:
            t = c[key]
            for p in range(1, 6):
                pc, per = ref.passes[p][t], (1 << R.DIGIT_BITS[p]) // 64
                want(pc.lane == lane_of(per) and pc.bin_in_lane == bin_of(per), f"{key}: pass {p} rank {t}: {pc}")
            want(ref.passes[5][t].occupied >= 32, f"{key}: rank {t} last digit occupied {ref.passes[5][t].occupied}")
    if "copies" in c:
        want(ref.copies == c["copies"], f"copies {ref.copies}")
    if "copies_min" in c:
        want(ref.copies >= c["copies_min"], f"copies {ref.copies}")
    if "below" in c:
        want(ref.below == c["below"], f"below {ref.below}")
    if "median_copies_min" in c:
        got = int(np.count_nonzero(case.values().view(np.uint64) == np.uint64(ref.median_bits)))
        want(got >= c["median_copies_min"], f"median copies {got}")
    kind = c["mean"]
    want(ref.mean_kind == {"zero": "finite", "exact": "finite"}.get(kind, kind), f"mean kind {ref.mean_kind}")
    if kind == "zero":
        want(ref.T == 0 and ref.n99 > 0 and case.values().min() > 0.0, "T == 0 from positive values")
    if kind == "exact":
        v = np.sort(case.values())[:ref.n99]
        s = sum(Fraction(x) for x in v.tolist()) / ref.n99
        want(ref.n99 & (ref.n99 - 1) == 0 and ref.mean == s and Fraction(float(s)) == s, "exact mean")
    if c.get("truncating"):
        v = np.sort(case.values())[:ref.n99]
        exact = sum(Fraction(float(x) * ref.inv) for x in v.tolist())
        want(0 < ref.T and ref.mean < exact, "truncation drops bits")
    if c.get("term_limit"):
        big = float(np.sort(case.values())[ref.n99 - 1])
        up = float(np.nextafter(big, INF))
        want(big * ref.inv < 2.0 ** 40 <= up * ref.inv, f"largest term {big * ref.inv!r}")
    return bad
