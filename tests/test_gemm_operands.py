"""CPU side of tests/test_gemm_dispatch_gpu.py: the exact operands really are exact (tests/gemm_operands.py), checked with the split
restatements of tests/test_split6.py over the WHOLE pool each kind draws from."""
import numpy as np
import pytest

import gemm_operands as G
from test_split6 import split3


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "bf16x3"])
def test_wide_pool_splits_exactly_and_fills_every_plane(mode):
    pool = G.wide_pool(mode)
    assert (pool % 2 == 1).all() and pool.min() >= G.WIDE_RANGE[mode][0] and pool.max() < G.WIDE_RANGE[mode][1]
    share = G.check_pool(mode, pool)
    assert share == pytest.approx(0.75, abs=0.01) if mode != "bf16x3" else share == 1.0
    G.check_sum_bound(pool.max(), 1, G.MAX_NNZ, extra=3 * G.SMALL_MAX)          # + bias + bias2 + C0


def test_seventeen_bit_integers_leave_the_low_plane_empty():
    """why the wide operands of the three-plane modes have 19 bits: odd integers in [2^16, 2^17) split as h + m with l == 0 throughout"""
    v = np.arange(2 ** 16 + 1, 2 ** 17, 2).astype(np.float32)
    h, m, lo, _ = split3(v)
    assert h.all() and m.all() and not lo.any()


def test_small_integers_live_in_the_high_plane():
    G.check_small()
    G.check_sum_bound(G.SMALL_MAX, G.SMALL_MAX, 340000, extra=3 * G.SMALL_MAX)
    with pytest.raises(AssertionError):
        G.check_sum_bound(G.SMALL_MAX, G.SMALL_MAX, 343000)


def test_wide_times_sign_partial_products_are_integers_in_every_plane():
    """each plane of a wide value times a sign is an integer below 2^19: whatever order a kernel adds the plane products in, every
    partial sum of at most MAX_NNZ terms is an integer below 2^24"""
    for mode in ("bf16x6", "bf16x3"):
        pl, _ = G.planes(mode, G.wide_pool(mode))
        assert sum(np.abs(p).max() for p in pl) * G.MAX_NNZ < G.EXACT_LIMIT
