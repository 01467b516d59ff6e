"""tests/stream_compact_restate.py pinned by hand-written cases, no device: the stable partition, -1 behind the live entries, the
bitwise carry gather, the k hand-over (retired slots only, an out-of-range origin skipped) and the cache row gather."""
import numpy as np

import stream_compact_restate as R


def test_a_hand_written_plan():
    active = [1, 0, 2, 0, -1, 0]
    origin = [10, 11, 12, 13, 14, 15]
    carry = np.array([-0.5, -1.5, -0.0, -3.5, np.nan, -5.5])
    k = [0, 7, 0, 9, 0, 3]
    k_full = np.full(16, -7, np.int32)
    p = R.plan(active, origin, carry, k, k_full)
    assert p["n_live"] == 3
    assert p["slot_src"].tolist() == [0, 2, 4, -1, -1, -1] and p["origin"].tolist() == [10, 12, 14, -1, -1, -1]
    assert p["carry"].view(np.uint64).tolist() == carry[[0, 2, 4]].view(np.uint64).tolist()
    assert np.signbit(p["carry"][1]) and np.isnan(p["carry"][2])
    want = np.full(16, -7, np.int32)
    want[[11, 13, 15]] = [7, 9, 3]
    assert p["k_full"].tolist() == want.tolist() and k_full.tolist() == [-7] * 16          # a copy: the input is not written


def test_identity_origin_none_and_all_retired():
    p = R.plan([1, 1, 1])
    assert p["n_live"] == 3 and p["slot_src"].tolist() == [0, 1, 2] and p["origin"].tolist() == [0, 1, 2]
    assert p["carry"] is None and p["k_full"] is None
    p = R.plan([0, 0, 0], None, np.array([1.0, 2.0, 3.0]), [4, 5, 6], np.zeros(3, np.int32))
    assert p["n_live"] == 0 and p["slot_src"].tolist() == [-1] * 3 and p["origin"].tolist() == [-1] * 3
    assert p["carry"].size == 0 and p["k_full"].tolist() == [4, 5, 6]
    p = R.plan([5, 5], None, np.array([1.0, 2.0]), [4, 5], np.array([8, 9], np.int32))
    assert p["n_live"] == 2 and p["carry"].tolist() == [1.0, 2.0] and p["k_full"].tolist() == [8, 9]      # nobody retired: untouched


def test_an_origin_out_of_range_is_skipped():
    k_full = np.array([50, 51, 52, 53], np.int32)
    p = R.plan([0, 0, 0, 1], [4, -1, 2, 99], None, [7, 8, 9, 1], k_full)
    assert p["k_full"].tolist() == [50, 51, 9, 53]
    assert p["origin"].tolist() == [99, -1, -1, -1]                                       # a live slot's origin is copied as it is
    p = R.plan([0, 0], [1, 3], None, [7, 8], k_full, B_full=2)                            # B_full below the array's length
    assert p["k_full"].tolist() == [50, 7, 52, 53]


def test_a_second_plan_composes_with_the_first():
    first = R.plan([1, 0, 1, 1, 0, 1])
    n = first["n_live"]
    second = R.plan([0, 1, 1, 0], first["origin"][:n])
    assert second["origin"][:second["n_live"]].tolist() == [2, 3]
    assert second["slot_src"].tolist() == [1, 2, -1, -1]


def test_cache_gather_by_hand():
    t0, B_src, B_dst, W = 2, 3, 2, 4
    src = np.arange(3 * B_src * W, dtype=np.float32).reshape(3 * B_src, W)                 # one rank more than t0
    src[1, 0] = np.float32(-0.0)
    src.view(np.uint32)[5, 1] = 0x7FC12345                                                # a NaN payload
    dst = np.full((3 * B_dst, W), -9.0, np.float32)
    out = R.gather_cache(src, [2, 1], t0, B_src, B_dst, dst)
    assert np.array_equal(out.view(np.uint32)[[0, 1, 2, 3]], src.view(np.uint32)[[2, 1, 5, 4]])
    assert out.view(np.uint32)[2, 1] == 0x7FC12345 and np.signbit(out[1, 0])
    assert (out[4:] == -9.0).all() and (dst == -9.0).all()                                 # behind t0*B_dst; dst itself is not written
    out = R.gather_cache(src, [-1, 3], t0, B_src, B_dst, dst)
    assert (out == -9.0).all()                                                            # both entries out of range
