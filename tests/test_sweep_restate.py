"""The float64 numpy restatement of the cut sweep (tests/sweep_restate.py) pinned to oracle/metrics.py on the committed cut-report
fixtures (tests/golden/report_*.npz: the `output` and `labels` the reference produced), and to the properties the rules'
definitions imply.

F1@k is formed from the same integers by the same operations as oracle.metrics.f1_per_list: exact.  DCG@k here is a running
sum in position order, the oracle's a numpy sum of the same k terms gain / log2(j + 2): S * 2^-53 * sum|term| bounds the
reordering of at most S terms, and is asserted."""
import glob
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_restate as W  # noqa: E402
from oracle import metrics as OM  # noqa: E402

FIXTURES = sorted(f for f in glob.glob(os.path.join(REPO, "tests", "golden", "report_*.npz")) if "bicut" not in f)
BICUT = os.path.join(REPO, "tests", "golden", "report_bicut_s40.npz")
TAUS = np.linspace(0.05, 0.95, 19)


def test_fixtures_present():
    assert len(FIXTURES) == 4 and os.path.exists(BICUT)


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_f1_and_dcg_equal_the_oracle_at_the_same_k(path):
    d = np.load(path)
    p, y = d["output"], d["labels"].astype(np.float32)
    B, S = y.shape
    k = W.cuts(p, TAUS, W.QUANTILE)
    assert k.min() >= 1 and k.max() <= S
    pl = W.per_list(y, k)
    absterm = np.abs(W.dcg_terms(y))
    for t in range(len(TAUS)):
        assert np.array_equal(pl["f1"][:, t], OM.f1_per_list(y, k[:, t]))
        ref = OM.dcg_per_list(y, k[:, t])
        scale = np.array([absterm[b, :k[b, t]].sum() for b in range(B)])
        err = np.abs(pl["dcg"][:, t] - ref)
        assert np.all(err <= S * 2.0 ** -53 * scale), (t, (err / scale).max() * 2.0 ** 53)
    # another penalty, one column
    assert np.all(np.abs(W.per_list(y, k[:, 9:10], penalty=-0.5)["dcg"][:, 0] - OM.dcg_per_list(y, k[:, 9], -0.5))
                  <= S * 2.0 ** -53 * np.array([absterm[b, :k[b, 9]].sum() for b in range(B)]))


def test_k0_columns_are_zero():
    y = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=np.float32)
    k = np.zeros((3, 2), dtype=np.int32)
    pl = W.per_list(y, k)
    for name in ("k", "f1", "dcg", "precision", "recall", "fbeta", "uncut"):
        assert np.all(pl[name] == 0.0), name
    assert np.all(pl["n_lists"] == 1.0)
    c = W.curve(y, k)
    assert np.array_equal(c[7], [3.0, 3.0]) and np.all(c[:7] == 0.0)
    # the score rule reaches k = 0: a threshold above every score
    v = np.array([[3.0, 2.0, 2.0, 1.0]], dtype=np.float32)
    assert W.cuts(v, [4.0, 2.0, 0.5, 3.0], W.FIRST_BELOW).tolist() == [[0, 3, 4, 1]]


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_quantile_is_monotone_and_meets_its_ends(path):
    p = np.load(path)["output"]
    B, S = p.shape
    taus = np.concatenate([[-1.0, 0.0], TAUS, [1.0]])
    k = W.cuts(p, taus, W.QUANTILE)
    assert np.all(np.diff(k, axis=1) >= 0)
    assert np.all(k[:, 0] == 1) and np.all(k[:, 1] == 1)            # tau <= 0: no prefix is below the target
    positive = p[:, -1] > 0
    assert positive.any()
    assert np.all(k[positive, -1] == S)                              # tau = 1: every C_j, j < S, is below C_S when the last p is positive
    # the definition: the smallest k whose mass reaches the share tau
    C = W.prefix(p)
    for b in range(B):
        for t, tau in enumerate(TAUS):
            kk = k[b, 2 + t]
            assert kk == S or C[b, kk - 1] >= tau * C[b, -1]
            assert kk == 1 or C[b, kk - 2] < tau * C[b, -1]


def test_degenerate_rows():
    v = np.zeros((1, 6), dtype=np.float32)
    assert W.cuts(v, [0.0, 0.5, 1.0], W.QUANTILE).tolist() == [[1, 1, 1]]       # total 0: every comparison is false
    v[0, 3] = np.nan
    assert W.cuts(v, [0.0, 0.5, 1.0], W.QUANTILE).tolist() == [[1, 1, 1]]       # total NaN
    assert W.cuts(v, [0.0], W.FIRST_BELOW).tolist() == [[3]]                    # NaN >= tau is false
    assert W.cuts(v, [0.5], W.FIRST_ABOVE).tolist() == [[6]]                    # no position reaches tau: S
    assert W.cuts(v, [0.0], W.FIRST_ABOVE).tolist() == [[1]]


def test_first_above_at_one_half_is_bicuts_rule():
    """Where the two class values of a position sum to exactly 1.0f, class 0 >= 0.5 is `class 0 >= class 1`, the pair rule's
    argmax with its tie to class 0.  The committed fixture holds 8 x 40 = 320 positions, 276 of which qualify (asserted);
    the predicate is compared on all of those, and the cut on the 6 lists all of whose positions up to the cut qualify."""
    out = np.load(BICUT)["output2"]
    B, S = out.shape[:2]
    exact = (out[:, :, 0] + out[:, :, 1]) == np.float32(1.0)
    assert (int(exact.sum()), exact.size) == (276, 320)
    k_rule = W.cuts(out[:, :, 0], [0.5], W.FIRST_ABOVE)[:, 0]
    k_ref = OM.bicut_cut_positions(out)
    # per position: the rule's predicate against the pair rule's, wherever the sum is exact
    above = out[:, :, 0].astype(np.float64) >= 0.5
    prefers0 = np.argmax(out, axis=2) == 0
    assert np.array_equal(above[exact], prefers0[exact])
    lists = [b for b in range(B) if exact[b, :max(k_rule[b], k_ref[b])].all()]
    assert len(lists) == 6
    assert np.array_equal(k_rule[lists], k_ref[lists])


def test_best_takes_the_first_maximum():
    assert W.best(np.array([0.1, 0.7, 0.7, 0.2]), [0.2, 0.4, 0.6, 0.8]) == (0.4, 1, 0.7)
