"""The EXACT operands of tests/test_gemm_dispatch_gpu.py, stated and checked on the CPU (numpy, no GPU): operands chosen so that every
partial product and every partial sum of a product C = op(A) op(B) is representable in fp32 in whatever order a kernel forms it - the
result then equals the int64 / float64 reference bit for bit in every precision mode, and a fault in one bf16 plane of a split shows
as a wrong integer instead of hiding inside a rounding tolerance.

  small   integers in [-7, 7]: three significand bits, they live in the high bf16 plane alone; sum |a b| <= 49 K < 2^24 up to
          K = 342,392
  wide    one operand WIDE, the other from {-1, 0, 1} with at most MAX_NNZ = 16 non-zeros per output element:
            fp32, bf16x6   odd integers in [2^18, 2^19) - 19 significand bits.  The three-way split x = h + m + l (tests/test_split6.py
                           split3) holds them exactly, h and m are never zero, and l is non-zero for the 3/4 of them whose first
                           residual needs more than eight bits (|x - h| >= 256).  Odd integers below 2^18 - 2^8 leave l = 0: an
                           eight-bit plane holds every integer up to 256 and rounding to nearest gives each plane one more bit, so
                           the third plane only starts at the 18th bit.
            bf16x3         odd integers in [2^15, 2^16): the two-way split x = hi + lo (lo = bf16(x - hi)) holds them exactly and
                           both planes are non-zero for every one of them
          sum |a b| < 16 * 2^19 = 2^23.
"""
import numpy as np

from test_split6 import bf16_rne, split3

SMALL_MAX = 7
MAX_NNZ = 16
EXACT_LIMIT = 2 ** 24                 # integers of magnitude <= 2^24 are fp32 values
WIDE_RANGE = {"fp32": (2 ** 18, 2 ** 19), "bf16x6": (2 ** 18, 2 ** 19), "bf16x3": (2 ** 15, 2 ** 16)}
ALL_PLANES_SHARE = {"fp32": 0.74, "bf16x6": 0.74, "bf16x3": 1.0}       # stated share of the pool that is non-zero in EVERY plane


def split2(x):
    """the bf16x3 mode's two planes: hi = bf16(x), lo = bf16(x - hi); -> hi, lo, what is left"""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    lo = bf16_rne(r)
    return hi, lo, (r - lo).astype(np.float32)


def wide_pool(mode):
    lo, hi = WIDE_RANGE[mode]
    return np.arange(lo + 1, hi, 2, dtype=np.int64)


def planes(mode, values):
    """-> (the planes of the mode's split, the residual nothing holds), as float64"""
    x = np.asarray(values, dtype=np.float32)
    assert np.array_equal(x.astype(np.int64), np.asarray(values, dtype=np.int64))
    if mode == "bf16x3":
        hi, lo, rest = split2(x)
        return [hi.astype(np.float64), lo.astype(np.float64)], rest.astype(np.float64)
    h, m, lo, r2 = split3(x)
    return [h.astype(np.float64), m.astype(np.float64), lo.astype(np.float64)], (r2 - lo).astype(np.float64)


def check_pool(mode, values):
    """the values split exactly into the mode's planes, every plane holds an integer, and the stated share of them is non-zero in
    every plane; both signs.  -> that share"""
    v = np.asarray(values, dtype=np.int64)
    share = 1.0
    for sign in (1, -1):
        pl, rest = planes(mode, sign * v)
        assert not rest.any(), "a residual is left over"
        assert np.array_equal(sum(pl), (sign * v).astype(np.float64)), "the planes do not add up to the value"
        for p in pl:
            assert np.array_equal(p, np.round(p))
        share = min(share, float(np.all([p != 0 for p in pl], axis=0).mean()))
    assert share >= ALL_PLANES_SHARE[mode], (mode, share)
    return share


def check_small():
    v = np.arange(-SMALL_MAX, SMALL_MAX + 1)
    for mode in ("bf16x6", "bf16x3"):
        pl, rest = planes(mode, v)
        assert not rest.any() and np.array_equal(pl[0], v.astype(np.float64)) and not any(p.any() for p in pl[1:])


def check_sum_bound(max_a, max_b, terms, extra=0):
    """sum |a b| over the non-zero terms of one output element, plus the epilogue's integers, stays an fp32 integer"""
    bound = int(max_a) * int(max_b) * int(terms) + int(extra)
    assert bound < EXACT_LIMIT, (max_a, max_b, terms, extra, bound)
    return bound
