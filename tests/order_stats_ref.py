"""The exact reference of validation()'s two statistics (numpy and Python integers only; TEST INFRASTRUCTURE).

Written from the definition (src/util.rs:778-795 as csrc/ccal_kernels_stats.hip restates it), not from the kernel's passes:

    sorted  = the n values in ascending order (values >= +0: the order of their bit patterns)
    median  = sorted[n // 2]                                             a bit pattern
    n99     = n * 99 // 100,   inv = fl(1 / n99),   K = sorted[n99 - 1]
    T       = sum_{i < n99} trunc( fl(sorted[i] * inv) / 2^-80 )          an exact Python integer
    mean    = T / 2^80                                                   a Fraction;  0 when n99 == 0 (the sum of an empty iterator)

`trunc` restates the documented fixed-point conversion (`to_fixed`): the mantissa with its implicit bit (a denormal: none, exponent 1),
shifted; a right shift drops bits, a right shift of 64 or more gives 0; a set sign bit or an exponent >= 1023 + 40 makes the term
"bad".  A bad term makes the mean +inf, a NaN among the first n99 values makes it NaN.

INPUT CONTRACT: reprojection errors are norms, so values are >= +0.  Negative values and -0.0 are outside the contract (their bit
patterns do not order like their values); `reference` refuses them and no test feeds one to the device.

Beside the two statistics `reference` returns, per pass of the kernel's digit split (11+11+11+11+11+9 bits, most significant
first) and per rank (0: the median's, 1: the 99 % key's), how contested that digit is - computed from the SORTED KEYS, not from
histograms: tests/order_stats_cases.py states each case's properties with them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

FRAC_BITS = 80
DIGIT_BITS = (11, 11, 11, 11, 11, 9)
EXP_LIMIT = 1023 + 40
INF_BITS = 0x7FF0000000000000
_MASK52 = (1 << 52) - 1


def to_fixed(bits: int):
    """trunc(v / 2^-80) of the double with bit pattern `bits`, or None when the term is bad."""
    ex = (bits >> 52) & 0x7FF
    man = (bits & _MASK52) | ((1 << 52) if ex else 0)
    if (bits >> 63) or ex >= EXP_LIMIT:
        return None
    sh = (ex if ex else 1) - 1075 + FRAC_BITS                # value = man * 2^(ex - 1075)
    if sh >= 0:
        return man << sh
    return 0 if -sh >= 64 else man >> (-sh)


def _exact_sum(a: np.ndarray) -> int:
    """Sum of a uint64 array as a Python integer (two 32-bit halves: no wrap below 2^32 elements)."""
    a = np.asarray(a, dtype=np.uint64)
    return (int(np.sum(a >> np.uint64(32), dtype=np.uint64)) << 32) + int(np.sum(a & np.uint64(0xFFFFFFFF), dtype=np.uint64))


def fixed_sum(term_bits: np.ndarray) -> int:
    """sum of to_fixed over an array of bit patterns, none of them bad: grouped by shift, every group summed exactly."""
    b = np.asarray(term_bits, dtype=np.uint64)
    ex = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    man = (b & np.uint64(_MASK52)) | np.where(ex != 0, np.uint64(1 << 52), np.uint64(0))
    sh = np.where(ex != 0, ex, 1) - 1075 + FRAC_BITS
    total = 0
    for s in np.unique(sh):
        s = int(s)
        m = man[sh == s]
        if s >= 0:
            total += _exact_sum(m) << s
        elif -s < 64:
            total += _exact_sum(m >> np.uint64(-s))
    return total


@dataclass
class PassCounts:
    """One pass, one rank: the keys that share every more significant digit with the key at the rank."""
    candidates: int          # how many keys
    occupied: int            # distinct values of this pass's digit among them
    lanes: int               # distinct lanes' ranges (a lane owns bins / 64 consecutive bins) among them
    lane: int                # the lane whose range holds the rank
    bin_in_lane: int         # the answer's bin inside that lane's range
    before_in_lane: int      # occupied bins of that lane in front of the answer
    digit: int


@dataclass
class Ref:
    n: int
    n99: int
    inv: float
    median_bits: int
    k_bits: int | None                   # None when n99 == 0
    T: int | None                        # None when the mean is not finite
    mean_kind: str                       # "finite" | "inf" | "nan"
    copies: int                          # copies of K at or below the rank (0 when n99 == 0)
    below: int                           # keys below K
    passes: list = field(default_factory=list)      # [pass][rank] -> PassCounts (rank 1 absent when n99 == 0)

    @property
    def mean(self) -> Fraction:
        assert self.T is not None
        return Fraction(self.T, 1 << FRAC_BITS)


def _pass_counts(keys: np.ndarray, target: int) -> list:
    out = []
    above = 0                                   # bits above this pass's digit
    for bits in DIGIT_BITS:
        lo_bits = 64 - above - bits             # bits below the digit
        if above == 0:
            cand = keys
        else:
            p = target >> (64 - above)
            a = np.searchsorted(keys, np.uint64(p << (64 - above)), side="left")
            hi = ((p + 1) << (64 - above)) - 1
            b = np.searchsorted(keys, np.uint64(hi), side="right")
            cand = keys[a:b]
        nb = 1 << bits
        per = nb // 64
        digits = np.unique(((cand >> np.uint64(lo_bits)) & np.uint64(nb - 1)).astype(np.int64))
        d = (target >> lo_bits) & (nb - 1)
        lane = d // per
        out.append(PassCounts(candidates=int(cand.size), occupied=int(digits.size), lanes=int(np.unique(digits // per).size),
                              lane=lane, bin_in_lane=d % per,
                              before_in_lane=int(np.count_nonzero((digits >= lane * per) & (digits < d))), digit=d))
        above += bits
    return out


def reference(vals) -> Ref:
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    n = int(vals.size)
    assert n > 0
    keys = np.sort(vals.view(np.uint64))
    assert int(keys[-1]) >> 63 == 0, "negative values and -0.0 are outside the contract"
    srt = keys.view(np.float64)
    n99 = n * 99 // 100
    median_bits = int(keys[n // 2])
    counts = [[c] for c in _pass_counts(keys, median_bits)]
    if n99 == 0:
        return Ref(n, 0, 0.0, median_bits, None, 0, "finite", 0, 0, counts)
    inv = float(np.float64(1.0) / np.float64(n99))
    k_bits = int(keys[n99 - 1])
    for p, c in enumerate(_pass_counts(keys, k_bits)):
        counts[p].append(c)
    below = int(np.searchsorted(keys, np.uint64(k_bits), side="left"))
    copies = n99 - below
    with np.errstate(all="ignore"):
        terms = (srt[:n99] * np.float64(inv)).view(np.uint64)
    if np.isnan(srt[:n99]).any():
        T, kind = None, "nan"
    elif ((terms >> np.uint64(52)) >= np.uint64(EXP_LIMIT)).any():
        T, kind = None, "inf"
    else:
        T, kind = fixed_sum(terms), "finite"
    return Ref(n, n99, inv, median_bits, k_bits, T, kind, copies, below, counts)


def brute_force(vals):
    """The same definition the slow way, with no bit arithmetic: np.sort on the VALUES (finite input), every term as the exact
    rational of the rounded product, floored to a multiple of 2^-80.  (median value, Fraction mean; None: a term >= 2^40)."""
    srt = np.sort(np.ascontiguousarray(vals, dtype=np.float64))
    assert np.isfinite(srt).all()
    n = srt.size
    n99 = n * 99 // 100
    med = float(srt[n // 2])
    if n99 == 0:
        return med, Fraction(0)
    inv = 1.0 / float(n99)
    total = 0
    for v in srt[:n99].tolist():
        t = v * inv                                     # Python floats: IEEE doubles, round to nearest
        if t >= 2.0 ** 40:
            return med, None
        num, den = t.as_integer_ratio()
        total += (num << FRAC_BITS) // den
    return med, Fraction(total, 1 << FRAC_BITS)
