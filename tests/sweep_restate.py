"""Float64 numpy restatement of the cut sweep (rlt_cut_sweep, ops.cut_sweep, utils/sweep.py): the three threshold rules as plain
Python loops over the positions, C = np.cumsum in position order, and the eight columns of the curve.  Independent of the
library and of torch; the tests compare the device against it and it against oracle/metrics.py."""
import numpy as np

QUANTILE, FIRST_BELOW, FIRST_ABOVE = 0, 1, 2
ROWS = ("k", "f1", "dcg", "precision", "recall", "fbeta", "uncut", "n_lists")


def prefix(v):
    """C (B,S) float64: the inclusive prefix sums of v in position order."""
    return np.cumsum(np.asarray(v).astype(np.float64), axis=1)


def cut_quantile(v, taus):
    """k = 1 + #{ j in 1..S-1 : C_j < tau * C_S }: the smallest k whose mass reaches the share tau.  (B,T) int32."""
    C = prefix(v)
    B, S = C.shape
    k = np.zeros((B, len(taus)), dtype=np.int32)
    for b in range(B):
        row = C[b].tolist()                         # Python floats: the same float64 values, quicker to loop over
        for t, tau in enumerate(taus):
            target = tau * row[S - 1]
            n = 1
            for j in range(S - 1):
                if row[j] < target:
                    n += 1
            k[b, t] = n
    return k


def cut_first_below(v, taus):
    """k = the number of leading positions with v_j >= tau (0..S)."""
    v = np.asarray(v).astype(np.float64)
    B, S = v.shape
    k = np.zeros((B, len(taus)), dtype=np.int32)
    for b in range(B):
        row = v[b].tolist()
        for t, tau in enumerate(taus):
            n = 0
            while n < S and row[n] >= tau:
                n += 1
            k[b, t] = n
    return k


def cut_first_above(v, taus):
    """k = the first position j (1-based) with v_j >= tau, S if there is none."""
    v = np.asarray(v).astype(np.float64)
    B, S = v.shape
    k = np.zeros((B, len(taus)), dtype=np.int32)
    for b in range(B):
        row = v[b].tolist()
        for t, tau in enumerate(taus):
            n = S
            for j in range(S):
                if row[j] >= tau:
                    n = j + 1
                    break
            k[b, t] = n
    return k


CUTS = {QUANTILE: cut_quantile, FIRST_BELOW: cut_first_below, FIRST_ABOVE: cut_first_above}


def cuts(v, taus, rule):
    with np.errstate(invalid="ignore"):
        return CUTS[rule](v, [float(t) for t in taus])


def near_ties(v, taus, rel=2.0 ** -40):
    """(B,T) bool: QUANTILE pairs with min_j |C_j - tau * C_S| <= rel * C_S, which another summation order may flip."""
    C = prefix(v)
    target = np.asarray(taus, dtype=np.float64)[None, :] * C[:, -1:]
    with np.errstate(invalid="ignore"):
        gap = np.abs(C[:, :, None] - target[:, None, :]).min(axis=1)
        return gap <= rel * C[:, -1:]


def dcg_terms(labels, penalty=-1.0):
    """(B,S) float64: (label == 1 ? 1 : penalty) / log2(j + 2)."""
    y = np.asarray(labels)
    return np.where(y == 1, 1.0, float(penalty)) / np.log2(np.arange(y.shape[1]) + 2.0)[None, :]


def per_list(labels, k, penalty=-1.0, beta=1.0):
    """The eight values of every (list, threshold): dict of (B,T) float64 arrays keyed by ROWS; k (B,T) in 0..S."""
    y = np.asarray(labels)
    k = np.asarray(k)
    B, S = y.shape
    rel = (y == 1).astype(np.int64)
    terms = dcg_terms(y, penalty)
    out = {n: np.zeros(k.shape, dtype=np.float64) for n in ROWS}
    b2 = float(beta) * float(beta)
    for b in range(B):
        N = int(rel[b].sum())
        cnt = [0] + np.cumsum(rel[b]).tolist()
        dpre = [0.0] + np.cumsum(terms[b]).tolist()     # np.cumsum adds in position order, as a loop over j would
        for t in range(k.shape[1]):
            kk = int(k[b, t])
            c = float(cnt[kk])
            prec = c / kk if kk > 0 else 0.0
            rec = c / N if N != 0 else 0.0
            f1 = 2 * prec * rec / (prec + rec) if prec + rec != 0 else 0.0
            den = b2 * prec + rec
            fb = (1.0 + b2) * prec * rec / den if den != 0 else 0.0
            dcg = dpre[kk]
            out["k"][b, t] = kk
            out["f1"][b, t] = f1
            out["dcg"][b, t] = dcg
            out["precision"][b, t] = prec
            out["recall"][b, t] = rec
            out["fbeta"][b, t] = fb
            out["uncut"][b, t] = 1.0 if kk == S else 0.0
            out["n_lists"][b, t] = 1.0
    return out


def curve(labels, k, penalty=-1.0, beta=1.0):
    """(8,T) float64: the sums over the lists, in list order."""
    pl = per_list(labels, k, penalty, beta)
    return np.stack([pl[n].sum(axis=0) for n in ROWS])


def dcg_abs_terms(labels, k, penalty=-1.0):
    """(T,) float64: sum over lists and positions j <= k of |term| - the scale of the DCG row's rounding error."""
    a = np.abs(dcg_terms(labels, penalty))
    k = np.asarray(k)
    ca = np.concatenate([np.zeros((a.shape[0], 1)), np.cumsum(a, axis=1)], axis=1)
    return np.take_along_axis(ca, k.astype(np.int64), axis=1).sum(axis=0)


def best(curve_row, taus):
    """The first maximum of a curve row: (tau*, index, value)."""
    i = int(np.argmax(np.asarray(curve_row)))
    return float(taus[i]), i, float(curve_row[i])
