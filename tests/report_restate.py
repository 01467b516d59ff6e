"""Float64 numpy restatement of the cut report (rlt_cut_report, utils/report.py): the cut rules, the metrics at the cut, the
fp32-free reward and the two curves of the reference's `Trainer.plot` (run.py:242-298).  Independent of the library and of
torch; the tests compare the device against it and it against the reference's own fixtures (tests/golden/report_*.npz)."""
import numpy as np


def cut_argmax(p):
    """k = first maximum + 1 (run.py:141-142)."""
    return np.argmax(np.asarray(p), axis=1).astype(np.int32) + 1


def cut_pair(p2):
    """BiCut's rule (run.py:131-136) on (B,S,2): S when every position says continue, else the first truncate position + 1;
    np.argmax over the two classes sends a tie to class 0."""
    pred = np.argmax(np.asarray(p2), axis=2)
    S = pred.shape[1]
    return np.array([S if row.sum() == S else int(np.argmin(row)) + 1 for row in pred], dtype=np.int32)


def margin_argmax(p):
    p = np.asarray(p, dtype=np.float32)
    if p.shape[1] == 1:
        return np.zeros(p.shape[0], dtype=np.float32)
    top = np.sort(p, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]).astype(np.float32)


def reward(y, metric, penalty=-1.0):
    """(B,S) float64: Metric_for_Loss.f1 / .dcg of every (list, k), k = 1..S (utils/metrics.py:85-101)."""
    y = np.asarray(y, dtype=np.float64)
    S = y.shape[1]
    if metric == "f1":
        c = np.cumsum(y, axis=1)
        n = y.sum(1, keepdims=True)
        k = np.arange(1, S + 1, dtype=np.float64)[None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(c > 0, 2.0 * c / (k + n), 0.0)
    gain = np.where(y == 1.0, 1.0, float(penalty)) / np.log2(np.arange(S) + 2.0)[None]
    return np.cumsum(gain, axis=1)


def softmax64(x, scale):
    x = np.asarray(x).astype(np.float64) / scale
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def pred_curve(p, sharpen):
    """Sum over the lists of softmax_j(p_j / sharpen), float64, row maximum subtracted."""
    return softmax64(p, sharpen).sum(0)


def reward_curve(r, tau):
    """Sum over the lists of softmax_j(r_j / tau) for a reward matrix r (any float type), float64."""
    return softmax64(r, tau).sum(0)


def tail_fix(curve):
    """run.py:283: the figure's last three prediction values are overwritten with the fourth from the end."""
    c = np.array(curve, copy=True)
    if c.shape[0] >= 4:
        c[-3:] = c[-4]
    return c
