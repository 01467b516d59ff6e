"""numpy restatement of rlt_rerank_lists: per list, np.argsort(-v, kind="stable") on float32 and its inverse.

numpy's sort puts every NaN behind every number and a stable sort keeps equal keys (+0 == -0 included) and the NaNs in their
original order, which is the order the header states."""
import numpy as np


def perm(pred):
    """(B,S) float32 -> (B,S) int32: perm[b,i] = the original index of the document at new position i."""
    pred = np.asarray(pred, dtype=np.float32)
    return np.stack([np.argsort(-row, kind="stable") for row in pred]).astype(np.int32)


def inverse(p):
    """rank[b, perm[b,i]] = i."""
    p = np.asarray(p)
    r = np.empty_like(p)
    rows = np.arange(p.shape[0])[:, None]
    r[rows, p] = np.arange(p.shape[1], dtype=p.dtype)[None, :]
    return r


def rerank(pred, *arrays):
    """-> (perm, rank, sorted pred, [arrays in the new order]); the moved arrays keep their bits."""
    p = perm(pred)
    take = lambda a: np.take_along_axis(np.asarray(a), p.astype(np.int64), axis=1)
    return p, inverse(p), take(np.asarray(pred, dtype=np.float32)), [take(a) for a in arrays]


def dcg_terms(labels_rr):
    """The S float64 terms of the task metric's DCG over a re-ranked list: (label ? 1 : -1) / log2(i + 2)."""
    lab = np.asarray(labels_rr)
    return np.where(lab != 0, 1.0, -1.0) / np.log2(np.arange(lab.shape[-1]) + 2.0)


# ---- the inputs the GPU tests sort ----------------------------------------------------------------------------------------------
KINDS = ("randn", "ties", "equal", "descending", "ascending", "zeros", "specials")


def inputs(kind, B, S, seed=0):
    """(B,S) float32 head values of one kind: random; heavy ties from {0,1,2}; all equal; already descending / ascending;
    +0 / -0 mixed; NaN, +inf and -inf at position 0, at S-1 and at the 64-lane boundaries of a random row."""
    rng = np.random.default_rng(seed * 7919 + S * 31 + B)
    if kind == "randn":
        return rng.standard_normal((B, S)).astype(np.float32)
    if kind == "ties":
        return rng.integers(0, 3, (B, S)).astype(np.float32)
    if kind == "equal":
        return np.full((B, S), 0.25, dtype=np.float32)
    if kind in ("descending", "ascending"):
        row = np.arange(S, dtype=np.float32)
        return np.tile(row[::-1] if kind == "descending" else row, (B, 1)).copy()
    if kind == "zeros":
        return np.where(rng.integers(0, 2, (B, S)) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    if kind == "specials":
        v = rng.standard_normal((B, S)).astype(np.float32)
        v[:, ::5] = np.round(v[:, ::5])                         # some ties among the numbers too
        spots = sorted({p for p in [0, S - 1] + [e + d for e in range(64, S, 64) for d in (-1, 0)] if 0 <= p < S})
        vals = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        for b in range(B):
            for n, p in enumerate(spots):
                v[b, p] = vals[(n + b) % 3]
        nan2 = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]       # a negative NaN with a payload
        if S > 2:
            v[:, 1] = nan2
        return v
    raise ValueError(kind)
