"""Pins tests/compare_restate.py - the float64 restatement the device pass of csrc/compare.hip is tested against - to things
that do not depend on it: exhaustive enumeration of the sign vectors, the statistics of its draws, scipy for the two closed-form
tests, a hand-worked Holm example.  Also the host-side formulas of utils/compare.py and the join of compare_reports.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import compare_restate as R


# (seed, r, c) -> rlt_mix32(c), rlt_row_hash(seed, r), draw(seed, r, c): printed once by a host program compiled from csrc/common.h
# (the two C functions themselves, combined as the header comment of csrc/compare.hip states)
C_VALUES = (((0, 0, 0), 0x00000000, 0xAE6F80F1, 0xE12B0355),
            ((1, 2, 3), 0x53F1E9DD, 0x230069CE, 0xE0B12478),
            ((0xFFFFFFFF, 0xFFFFF, 0x3FFFFFF), 0x45C88D7A, 0x1694E7E1, 0xC4111731),
            ((12345, 999, 0xFFFFFFFF), 0x6768824A, 0xDA7F2DF8, 0x1FD60E23))
C_BOOT_SEED_OF_5 = 0x97309AED           # rlt_mix32(5 ^ 0xA511E9B3)


def test_generator_matches_values_computed_by_the_c_functions():
    for (seed, r, c), mixed, key, drawn in C_VALUES:
        assert int(R.mix32(c)) == mixed and int(R.row_hash(seed, r)) == key and int(R.draw(seed, r, c)) == drawn
    assert int(R.boot_seed(5)) == C_BOOT_SEED_OF_5


def test_generator_matches_a_second_transcription_in_python_integers():
    def mix(x):
        x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
        return x
    def rowh(seed, row):
        return mix((seed + mix((row + 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    for seed, r, c in ((0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 0xFFFFF, 0x3FFFFFF), (12345, 999, 0xFFFFFFFF), (77, 1 << 20, 1 << 26)):
        want = mix(rowh(seed, r) ^ mix((c + 0x7F4A7C15) & 0xFFFFFFFF))
        assert int(R.draw(seed, r, c)) == want
    assert int(R.mix32(0)) == 0 and R.boot_seed(5) == mix(5 ^ 0xA511E9B3)
    assert len(set(R.draw(3, 4, np.arange(100000)).tolist())) == 100000          # a bijection in c


def test_monte_carlo_p_against_full_enumeration():
    """Q = 12: all 2^12 sign vectors give the exact two-sided p; the restatement's p at R = 20,000 (seed 2) must lie within
    4 sqrt(p (1 - p) / R).  Measured: p_exact 0.05371, p_mc 0.05540, z = 1.06."""
    d = np.round((np.random.RandomState(102).randint(-512, 513, size=12) / 1024.0 + 0.18) * 1024) / 1024
    flips = np.array(list(itertools.product([1.0, -1.0], repeat=12)))
    t_obs = d.sum()
    p_exact = float((np.abs(flips @ d) >= abs(t_obs)).mean())
    Rn = 20000
    recs, rand, _ = R.compare(np.zeros(12, np.float32), d.astype(np.float32)[None, :], Rn, 2)
    assert recs[0][R.T_OBS] == t_obs
    p_mc = recs[0][R.RAND_GE] / Rn
    z = (p_mc - p_exact) / math.sqrt(p_exact * (1 - p_exact) / Rn)
    print(f"p_exact {p_exact:.5f} p_mc {p_mc:.5f} z {z:.2f}")
    assert 0.01 < p_exact < 0.2 and abs(z) <= 4.0
    assert R.randomization_p(recs[0][R.RAND_GE], Rn) == (recs[0][R.RAND_GE] + 1) / (Rn + 1)


def test_sign_bits_are_fair():
    """Mean of R * Q = 1.2 million signs within 4 / sqrt(R Q) of 0 (measured z = 0.39), and no position or replicate is stuck."""
    s = R.signs(7, np.arange(4000), 300)
    z = s.mean() * math.sqrt(s.size)
    print(f"z {z:.2f}")
    assert abs(z) <= 4.0
    assert np.abs(s.mean(axis=0)).max() < 5 / math.sqrt(4000) and np.abs(s.mean(axis=1)).max() < 5 / math.sqrt(300)
    assert np.array_equal(R.signs(7, [5], 300)[0, :64], R.signs(7, [5], 64)[0])          # a function of (seed, r, q) only


def test_bootstrap_indices_are_uniform():
    """Chi-square of the index counts over Q = 300 cells, R = 4000 replicates: within 4 sqrt(2 (Q - 1)) of Q - 1 (measured z = 1.24);
    every index is inside [0, Q), also at the largest Q."""
    Q, Rn = 300, 4000
    idx = R.indices(7, np.arange(Rn), Q)
    assert idx.min() >= 0 and idx.max() < Q
    cnt = np.bincount(idx.ravel(), minlength=Q)
    e = idx.size / Q
    chi = float(((cnt - e) ** 2 / e).sum())
    z = (chi - (Q - 1)) / math.sqrt(2 * (Q - 1))
    print(f"chi2 {chi:.1f} z {z:.2f}")
    assert abs(z) <= 4.0
    u = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint64)
    top = (u * np.uint64(1 << 26)) >> np.uint64(32)
    assert top.tolist() == [0, 0, (1 << 26) - 1]


def test_bootstrap_mean_has_the_right_spread():
    """Standard deviation of the bootstrap mean within 5 % of std(d) / sqrt(Q) (measured 0.05834 against 0.05902)."""
    Q, Rn = 300, 4000
    d = np.random.RandomState(3).randn(Q)
    _, boot = R.replicate_stats(d[None, :], 7, Rn)
    got, want = float((boot[0] / Q).std()), float(d.std() / math.sqrt(Q))
    print(f"{got:.5f} against {want:.5f}")
    assert abs(got - want) <= 0.05 * want


def test_exact_operands_make_every_sum_exact():
    for Q in (1, 31, 33, 300, 20481):
        base, sys = R.exact_operands(Q, 3, Q)
        assert np.abs(base).max() <= 0.5 and np.abs(sys).max() <= 0.5
        d, ok = R.differences(base, sys)
        assert ok.all()
        k = np.round(d * 1024).astype(np.int64)
        assert np.array_equal(k / 1024.0, d) and (k.sum(axis=1) % Q == 0).all()


def test_closed_form_tests_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    from utils import compare as C
    for w, l in ((3, 9), (10, 10), (0, 5), (40, 61), (7, 0), (0, 0), (3000, 3200), (2100, 2000)):
        want = stats.binomtest(w, w + l, 0.5).pvalue if w + l else 1.0
        assert C.sign_test_p(w, l) == pytest.approx(want, rel=1e-9)
        if w + l <= 1000:
            assert R.sign_test_p(w, l) == pytest.approx(want, rel=1e-12)
    d = np.random.RandomState(5).randn(57) + 0.3
    want = stats.ttest_1samp(d, 0.0)
    t, df = R.t_statistic(d)
    assert df == 56 and t == pytest.approx(want.statistic, rel=1e-12)
    mean = d.sum() / d.size
    t2, df2 = C.t_statistic(mean, ((d - mean) ** 2).sum(), d.size)
    assert df2 == 56 and t2 == pytest.approx(want.statistic, rel=1e-12)
    # zero variance
    assert C.t_statistic(0.0, 0.0, 9) == (0.0, 8) and C.t_statistic(0.5, 0.0, 9) == (math.inf, 8)
    assert C.t_statistic(-0.5, 0.0, 9) == (-math.inf, 8) and R.t_statistic(np.full(9, -0.5)) == (-math.inf, 8)


def test_holm_on_a_hand_worked_example():
    """p = (0.01, 0.04, 0.03, 0.5): sorted 0.01, 0.03, 0.04, 0.5 times 4, 3, 2, 1 = 0.04, 0.09, 0.08, 0.5; running maximum 0.04,
    0.09, 0.09, 0.5; back in the order given."""
    from utils import compare as C
    want = [0.04, 0.09, 0.09, 0.5]
    assert C.holm([0.01, 0.04, 0.03, 0.5]) == pytest.approx(want, abs=1e-15)
    assert R.holm([0.01, 0.04, 0.03, 0.5]) == pytest.approx(want, abs=1e-15)
    assert C.holm([0.6, 0.9]) == [1.0, 1.0] and C.holm([]) == []


def test_percentile_interval_indices():
    from utils import compare as C
    s = np.arange(10000, dtype=np.float64)
    assert C.percentile_interval(s, 0.95) == (250.0, 9749.0)
    assert R.percentile_interval(s[::-1] * 4, 4, 0.95) == (250.0, 9749.0)
    assert C.percentile_interval([3.0], 0.9) == (3.0, 3.0)


def _write_report(path, qids, lengths, f1, best):
    np.savez(path, qid=np.asarray(qids), length=np.asarray(lengths, dtype=np.int32), f1=np.asarray(f1, dtype=np.float64),
             dcg=np.asarray(f1, dtype=np.float64) * 2, best_f1=np.asarray(best, dtype=np.float64))


def test_compare_reports_refuses_mismatched_query_sets(tmp_path):
    from utils import compare as C
    a, b, c, d = (str(tmp_path / f"{n}.npz") for n in "abcd")
    _write_report(a, ["q1", "q2", "q3"], [300, 300, 40], [0.1, 0.2, 0.3], [0.5, 0.5, 0.5])
    _write_report(b, ["q1", "q2", "q4"], [300, 300, 40], [0.1, 0.2, 0.3], [0.5, 0.5, 0.5])
    _write_report(c, ["q1", "q2", "q3"], [300, 40, 40], [0.1, 0.2, 0.3], [0.5, 0.5, 0.5])          # same qids, another length
    _write_report(d, ["q1", "q2"], [300, 300], [0.1, 0.2], [0.5, 0.5])
    for other in (b, c, d):
        with pytest.raises(ValueError, match="query set differs"):
            C.compare_reports([a, other], metric="f1", baseline=0, resamples=10)
    with pytest.raises(ValueError, match="metric"):
        C.compare_reports([a, a], metric="ndcg")
    with pytest.raises(ValueError, match="baseline"):
        C.compare_reports([a], metric="f1", baseline=0)
