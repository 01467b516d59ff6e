"""An independent float64 numpy restatement of the truncation baselines (cumulative sums, not the notebooks' loops), shared by
tests/test_baselines_abi.py and tests/test_baselines_gpu.py."""
import numpy as np


def per_k(labels, penalty=-1.0):
    """(F1, DCG), each (B, S+1) float64 for k = 0..S; F1 in cal_F1's operation order, so exact ties are bit-identical."""
    y = np.asarray(labels, dtype=np.float64)
    B, S = y.shape
    c = np.cumsum(y, axis=1)
    n = c[:, -1:]
    k = np.arange(1, S + 1, dtype=np.float64)
    p = c / k
    r = np.divide(c, n, out=np.zeros_like(c), where=n != 0)
    den = p + r
    f1 = np.divide(2 * p * r, den, out=np.zeros_like(c), where=den != 0)
    gain = np.where(y == 1, 1.0, float(penalty)) / np.log2(np.arange(S) + 2.0)
    dcg = np.cumsum(gain, axis=1)
    z = np.zeros((B, 1))
    return np.hstack([z, f1]), np.hstack([z, dcg])


def curves(labels, penalty=-1.0, chunk=16384):
    """Sums over lists of F1@k, DCG@k and c_k (3, S+1), the sums of the per-list bests (2,), and the per-list best values
    and first-maximum k (np.argmax) - in chunks of lists, for large sets."""
    y = np.asarray(labels)
    B, S = y.shape
    sums = np.zeros((3, S + 1))
    best = [np.empty(B), np.empty(B, dtype=np.int64), np.empty(B), np.empty(B, dtype=np.int64)]
    for lo in range(0, B, chunk):
        yc = y[lo:lo + chunk].astype(np.float64)
        f1, dcg = per_k(yc, penalty)
        sums[0] += f1.sum(0)
        sums[1] += dcg.sum(0)
        sums[2, 1:] += np.cumsum(yc, axis=1).sum(0)
        best[0][lo:lo + chunk], best[1][lo:lo + chunk] = f1.max(1), f1.argmax(1)
        best[2][lo:lo + chunk], best[3][lo:lo + chunk] = dcg.max(1), dcg.argmax(1)
    return sums, np.array([best[0].sum(), best[2].sum()]), best


def irrelevant_share(labels):
    """countp: (L k - sum over lists of c_k) / (L k), k = 1..S."""
    y = np.asarray(labels, dtype=np.float64)
    L, S = y.shape
    lk = L * np.arange(1, S + 1, dtype=np.float64)
    return (lk - np.cumsum(y, axis=1).sum(0)) / lk
