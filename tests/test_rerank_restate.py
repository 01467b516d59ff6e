"""tests/rerank_restate.py pinned without a GPU: the order is a bijection on NaN, +-inf, +-0 and ties, it is the order the header
states, and the DCG over a whole re-ranked list is the CPU reference's task metric."""
import numpy as np
import pytest

import rerank_restate as RR


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 300])
def test_bijection_and_inverse(kind, S):
    v = RR.inputs(kind, 4, S, seed=1)
    p, r, sv, (moved,) = RR.rerank(v, np.arange(4 * S, dtype=np.float32).reshape(4, S))
    ar = np.tile(np.arange(S), (4, 1))
    assert np.array_equal(np.sort(p, axis=1), ar)
    assert np.array_equal(np.take_along_axis(r, p, axis=1), ar) and np.array_equal(np.take_along_axis(p, r, axis=1), ar)
    assert np.array_equal(sv.view(np.uint32), np.take_along_axis(v, p.astype(np.int64), axis=1).view(np.uint32))
    assert np.array_equal(moved, p + (np.arange(4) * S)[:, None])


def test_the_stated_order():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    v = np.array([[nan, 1.0, -inf, 0.0, inf, -0.0, 1.0, nan, -3.0, inf]], dtype=np.float32)
    #             0    1    2     3    4    5     6    7    8     9
    assert RR.perm(v)[0].tolist() == [4, 9, 1, 6, 3, 5, 8, 2, 0, 7]
    assert RR.perm(np.zeros((1, 5), np.float32))[0].tolist() == [0, 1, 2, 3, 4]
    assert RR.perm(np.arange(5, dtype=np.float32)[None])[0].tolist() == [4, 3, 2, 1, 0]
    for kind in ("equal", "descending", "zeros"):
        assert np.array_equal(RR.perm(RR.inputs(kind, 3, 70)), np.tile(np.arange(70), (3, 1)))
    sp = RR.inputs("specials", 3, 130)
    p = RR.perm(sp)
    sv = np.take_along_axis(sp, p.astype(np.int64), axis=1)
    for row, order in zip(sv, p):
        n_nan = int(np.isnan(row).sum())
        assert n_nan >= 2 and np.isnan(row[len(row) - n_nan:]).all() and not np.isnan(row[:len(row) - n_nan]).any()
        assert np.all(np.diff(order[len(row) - n_nan:]) > 0)                  # the NaNs in their original order
        nums = row[:len(row) - n_nan]
        assert np.all(nums[:-1] >= nums[1:]) and nums[0] == np.inf and nums[-1] == -np.inf


def test_whole_list_dcg_is_the_reference_task_metric():
    from oracle import metrics as om
    rng = np.random.default_rng(5)
    for B, S in ((1, 1), (3, 7), (5, 64), (4, 300)):
        y = rng.integers(0, 2, (B, S)).astype(np.float32)
        pred = rng.standard_normal((B, S)).astype(np.float32)
        pred[:, ::3] = np.round(pred[:, ::3])
        _, _, _, (y_rr,) = RR.rerank(pred, y)
        mine = RR.dcg_terms(y_rr).sum(axis=1).mean()
        assert abs(mine - om.taskr_metric(y, pred)) <= 1e-12 * S
