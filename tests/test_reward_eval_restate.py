"""tests/reward_eval_restate.py pinned without a GPU: F_1 on 0/1 labels against the truncation-baseline restatement, the curve
and `better` against brute-force loops, ties at the maximum, all-zero lists and all-negative gain rows."""
import numpy as np
import pytest

import baseline_restate as BR
import reward_any_restate as R
import reward_eval_restate as E


def _ulps(a, b):
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _labels01(B, S, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random((B, S)) < 0.3).astype(np.float32)
    y[0] = 0.0                                      # no relevant document: every F1 is 0, the best cut is k = 0
    if B > 1:
        y[1] = 1.0
    return y


@pytest.mark.parametrize("S", [1, 2, 3, 40, 129, 300])
def test_fbeta_one_is_the_f1_of_the_truncation_baselines(S):
    """Best cut positions identical over k = 0..S, best values within one fp32 ulp.  Where a list's largest F1 is reached at
    several cuts IN EXACT ARITHMETIC (2 c / (N + k) equal for two (c, k)), cal_F1's three roundings can break the tie by a
    float64 ulp and move ITS argmax to a later cut; the reward's single correctly rounded division keeps the tie, and np.argmax
    takes the first.  So the ground truth is the exact rational maximiser: the restatement must give the first one on EVERY
    list, the baseline restatement must give the same position on every list whose maximiser is unique and one of the exact
    maximisers elsewhere.  (S = 40, seed 40, list 17: cuts 26 and 40 tie exactly; cal_F1 prefers 40.)"""
    y = _labels01(23, S, S)
    r64 = R.reward64(y, R.fbeta(1.0))
    f1, _dcg = BR.per_k(y)
    got = E.evaluate(r64, allow_empty=True)
    exact = E.exact_f1_maximisers(y)
    assert [int(k) for k in got["best_k"]] == [m[0] for m in exact]
    unique = np.array([len(m) == 1 for m in exact])
    assert unique.sum() >= len(y) - 2 or S <= 3         # short lists tie often; from S = 40 on at most two lists do
    assert np.array_equal(got["best_k"][unique], f1.argmax(1)[unique])
    assert all(int(k) in m for k, m in zip(f1.argmax(1), exact))
    assert _ulps(got["best"], f1.max(1)).max() <= 1                     # values within one fp32 ulp
    assert got["best_k"][0] == 0 and got["best"][0] == 0.0
    got32 = E.spec_evaluate(y, R.fbeta(1.0))
    assert _ulps(got32["best"], f1.max(1)).max() <= 1


@pytest.mark.parametrize("allow_empty", [True, False])
def test_curve_and_better_against_loops(allow_empty):
    rng = np.random.default_rng(5)
    B, S, T = 7, 19, 5
    y = rng.integers(0, 3, (B, S)).astype(np.float32)
    r = R.reward(y, R.gain((-1.0, 1.0, 3.0)))
    k = rng.integers(-2, S + 3, (B, T))
    got = E.evaluate(r, k, allow_empty)
    kmin = 0 if allow_empty else 1
    curve = [0.0] * (S + 1)
    for b in range(B):
        for j in range(1, S + 1):
            curve[j] += float(r[b, j - 1])
    assert np.array_equal(got["curve"], np.array(curve)) and got["curve"][0] == 0.0
    n_clamped = 0
    for b in range(B):
        vals = [0.0] + [float(v) for v in r[b]]
        for t in range(T):
            kc = min(max(int(k[b, t]), 0), S)
            n_clamped += kc != k[b, t]
            assert got["r_at"][b, t] == vals[kc]
            assert got["better"][b, t] == sum(1 for j in range(kmin, S + 1) if vals[j] > vals[kc])
    assert got["sums"][0] == B and got["sums"][2] == n_clamped
    assert np.array_equal(got["sums"][5::3], got["better"].sum(0))
    assert got["best_hist"].sum() == B


def test_ties_zero_lists_and_negative_rows():
    S = 6
    tie = np.array([[0.5, 1.0, 0.25, 1.0, 1.0, 0.0]], dtype=np.float32)        # the maximum three times: the first wins
    for ae in (True, False):
        got = E.evaluate(tie, [[2, 4, 5, 1]], ae)
        assert got["best_k"][0] == 2 and got["best"][0] == 1.0
        assert list(got["better"][0]) == [0, 0, 0, 3] and got["sums"][4] == 1 and got["sums"][7] == 1 and got["sums"][13] == 0
    zero = np.zeros((2, S), dtype=np.float32)                                   # all-zero lists: k = 0 ties with every cut
    assert list(E.evaluate(zero, None, True)["best_k"]) == [0, 0]
    assert list(E.evaluate(zero, None, False)["best_k"]) == [1, 1]
    neg = R.reward(np.zeros((1, S), dtype=np.float32), R.gain((-1.0, 1.0)))     # all-negative gain row
    assert (neg < 0).all()
    a, b = E.evaluate(neg, [[0, 1, S]], True), E.evaluate(neg, [[0, 1, S]], False)
    assert a["best_k"][0] == 0 and a["best"][0] == 0.0 and a["best_hist"][0] == 1
    assert b["best_k"][0] == 1 and b["best"][0] == neg[0, 0] and b["best_hist"][1] == 1
    assert list(a["better"][0]) == [0, 1, S] and list(b["better"][0]) == [0, 0, S - 1]
    assert list(a["r_at"][0]) == [0.0, neg[0, 0], neg[0, -1]]


def test_greedy_k():
    rng = np.random.default_rng(9)
    tr = R.reward(rng.integers(0, 2, (9, 12)).astype(np.float32), R.ndcg())
    te = R.reward(rng.integers(0, 2, (5, 12)).astype(np.float32), R.ndcg())
    val, k = E.greedy_k(tr, te)
    means = [0.0] + [float(tr[:, j].astype(np.float64).sum() / 9) for j in range(12)]
    assert k == max(range(13), key=lambda j: (means[j], -j))
    assert val == (0.0 if k == 0 else float(te[:, k - 1].astype(np.float64).sum() / 5))
