"""Float64 numpy restatement of the reward losses, the cut / task metrics and the multi-task terms (utils/losses.py,
utils/metrics.py), written from their semantics and vectorised over (B,S).  Independent of the library and of the oracle;
tests/test_loss_restate.py pins it to the reference's own fixtures, tests/test_scan_dispatch_gpu.py compares the device
against it."""
import numpy as np

EXPECT, CE, KL, JS = 0, 1, 2, 3


def reward(y, metric, penalty=-1.0):
    """(B,S): Metric_for_Loss.f1 / .dcg of every (list, k), k = 1..S (utils/metrics.py:85-101)."""
    y = np.asarray(y, dtype=np.float64)
    S = y.shape[1]
    if metric == "f1":
        hits = np.cumsum(y, axis=1)
        n_rel = y.sum(1, keepdims=True)
        k = np.arange(1, S + 1, dtype=np.float64)[None]
        prec = hits / k
        rec = np.divide(hits, n_rel, out=np.zeros_like(hits), where=n_rel != 0)
        tot = prec + rec
        return np.divide(2.0 * prec * rec, tot, out=np.zeros_like(tot), where=tot != 0)
    gain = np.where(y == 1.0, 1.0, float(penalty)) / np.log2(np.arange(S) + 2.0)[None]
    return np.cumsum(gain, axis=1)


def reward_distribution(r, tau):
    """q = exp(r / tau) / sum_j exp(r_j / tau) (utils/losses.py:226-228).  The row maximum is subtracted: the same quotient,
    finite for every r."""
    x = np.asarray(r, dtype=np.float64) / float(tau)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _xlogx(x):
    return np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0)), 0.0)


def reward_loss(p, y, metric, kind, tau=1.0, penalty=-1.0):
    """-> (per_list (B), loss = sum(per_list) / B, dloss/dp (B,S), r, q).  kind EXPECT: -sum p r (ChoopyLoss); CE: -sum q ln p
    (AttnCutLoss); KL: sum q (ln q - ln p) (DivLoss kl, batchmean); JS: (KL(q || m) + KL(p || m)) / 2, m = (p + q) / 2, the
    gradient flowing through ln m and the target p (DivLoss js)."""
    p = np.asarray(p, dtype=np.float64)
    B = p.shape[0]
    r = reward(y, metric, penalty)
    q = reward_distribution(r, tau)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.log(p)
        if kind == EXPECT:
            terms, dp = -(p * r), -r
        elif kind == CE:
            terms, dp = np.where(q > 0, -q * lp, 0.0), -q / p
        elif kind == KL:
            terms, dp = _xlogx(q) - np.where(q > 0, q * lp, 0.0), -q / p
        elif kind == JS:
            lm = np.log((p + q) / 2.0)
            terms = 0.5 * ((_xlogx(q) - np.where(q > 0, q * lm, 0.0)) + (_xlogx(p) - np.where(p > 0, p * lm, 0.0)))
            dp = 0.5 * (lp - lm)
        else:
            raise ValueError(kind)
    per = terms.sum(1)
    return per, per.sum() / B, dp / B, r, q


def cut_positions(p):
    """k = first maximum + 1 (run.py:141-142)."""
    return np.argmax(np.asarray(p), axis=1).astype(np.int64) + 1


def f1_at(y, k):
    """Metric.f1 per list (utils/metrics.py:15-24)."""
    y = np.asarray(y, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    head = np.arange(y.shape[1])[None] < k[:, None]
    hits, n_rel = (y * head).sum(1), y.sum(1)
    prec = hits / k
    rec = np.divide(hits, n_rel, out=np.zeros_like(hits), where=n_rel != 0)
    tot = prec + rec
    return np.divide(2.0 * prec * rec, tot, out=np.zeros_like(tot), where=tot != 0)


def dcg_at(y, k, penalty=-1.0):
    """Metric.dcg per list (utils/metrics.py:26-38): sum over the first k positions of (+1 | penalty) / log2(j + 2)."""
    y = np.asarray(y)
    head = np.arange(y.shape[1])[None] < np.asarray(k)[:, None]
    gain = np.where(y == 1, 1.0, float(penalty)) / np.log2(np.arange(y.shape[1]) + 2.0)[None]
    return (gain * head).sum(1)


def task_dcg(y, pred):
    """taskr_metric per list (utils/metrics.py:40-57): +1 (relevant) | -1 over log2(i + 2) at the stable descending rank i."""
    y, pred = np.asarray(y), np.asarray(pred)
    order = np.argsort(-pred.astype(np.float64), axis=1, kind="stable")
    gain = np.where(np.take_along_axis(y, order, axis=1) != 0, 1.0, -1.0)
    return (gain / np.log2(np.arange(y.shape[1]) + 2.0)[None]).sum(1)


def task_auc(y, pred, chunk=4):
    """taskc_metric per list (utils/metrics.py:59-76): (pairs of a relevant and a non-relevant document ranked correctly +
    half the tied pairs) / all such pairs; -1 for a list with one class.  Lists are taken `chunk` at a time to bound the
    (chunk,S,S) pair tables."""
    y, pred = np.asarray(y), np.asarray(pred)
    out = np.full(y.shape[0], -1.0)
    for lo in range(0, y.shape[0], chunk):
        yy, pp = y[lo:lo + chunk], pred[lo:lo + chunk]
        pos, neg = yy != 0, yy == 0
        pair = pos[:, :, None] & neg[:, None, :]
        gt = np.count_nonzero((pp[:, :, None] > pp[:, None, :]) & pair, axis=(1, 2))
        eq = np.count_nonzero((pp[:, :, None] == pp[:, None, :]) & pair, axis=(1, 2))
        n = pos.sum(1).astype(np.float64) * neg.sum(1)
        out[lo:lo + chunk] = np.where(n > 0, (gt + 0.5 * eq) / np.where(n > 0, n, 1.0), -1.0)
    return out


def mt_terms(rerank, cls, y, margin):
    """-> [hinge, bce, dhinge/ds of a y == 1 entry, of a y == 0 entry].  RerankLoss (utils/losses.py:99-141): max(0, mean of the
    y == 0 scores - mean of the y == 1 scores + margin) over the whole batch, 0 with zero gradients when a class is empty
    or the argument is not positive; nn.BCELoss: mean, both logs clamped at -100."""
    y = np.asarray(y, dtype=np.float64).ravel()
    hinge = gpos = gneg = bce = 0.0
    if rerank is not None:
        s = np.asarray(rerank, dtype=np.float64).ravel()
        n_pos, n_neg = int((y == 1).sum()), int((y == 0).sum())
        if n_pos and n_neg:
            gap = s[y == 0].sum() / n_neg - s[y == 1].sum() / n_pos + float(margin)
            if gap > 0:
                hinge, gpos, gneg = gap, -1.0 / n_pos, 1.0 / n_neg
    if cls is not None:
        c = np.asarray(cls, dtype=np.float64).ravel()
        with np.errstate(divide="ignore"):
            l1, l0 = np.maximum(np.log(c), -100.0), np.maximum(np.log1p(-c), -100.0)
        bce = float(-(y * l1 + (1.0 - y) * l0).mean())
    return np.array([hinge, bce, gpos, gneg])


def mt_terms_bwd(cls, y, terms, w_rerank, w_class, gscale=1.0):
    """-> (d_rerank, d_class), both of y's shape: w_r * terms[2 | 3] by label; w_c * torch's binary_cross_entropy_backward
    (c - y) / max((1 - c) c, eps) / n with eps the float32 nearest 1e-12, which torch uses at every dtype; both times
    gscale."""
    y = np.asarray(y, dtype=np.float64)
    d_rerank = np.where(y == 1, terms[2], np.where(y == 0, terms[3], 0.0)) * w_rerank * gscale
    d_class = None
    if cls is not None:
        c = np.asarray(cls, dtype=np.float64)
        d_class = (c - y) / np.maximum((1.0 - c) * c, float(np.float32(1e-12))) * (w_class * gscale / y.size)
    return d_rerank, d_class
