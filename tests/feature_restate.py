"""Independent numpy / scipy.sparse restatement of AttnCut's neighbour-similarity statistics, float64 throughout: the CPU
yardstick of tests/test_features_abi.py (against the notebook fixtures) and tests/test_features_gpu.py (against the device).

    sim(a, b) = (a . b) / (|a| |b|), 0 when the denominator is 0 or the quotient is NaN
    position 0: sim(0, 1); position S-1: sim(S-2, S-1); position i in between: (sim(i-1, i) + sim(i, i+1)) / 2

Nothing here shares code with the device path: the tf-idf rows go through scipy.sparse, the doc2vec rows through einsum."""
import numpy as np
import scipy.sparse as sp


def pair_sims(dots, sq_norms_a, sq_norms_b):
    """Cosine from dot products and squared norms, with the zero-denominator and NaN rules."""
    with np.errstate(all="ignore"):
        denom = np.sqrt(sq_norms_a) * np.sqrt(sq_norms_b)
        sim = np.where(denom != 0, dots / np.where(denom != 0, denom, 1.0), 0.0)
    return np.where(np.isnan(sim), 0.0, sim)


def neighbor_mean(pair):
    """pair (B, S-1): sim of positions (i, i+1) -> (B, S) statistics."""
    B, P = pair.shape
    out = np.empty((B, P + 1), dtype=np.float64)
    out[:, 0] = pair[:, 0]
    out[:, -1] = pair[:, -1]
    out[:, 1:-1] = (pair[:, :-1] + pair[:, 1:]) / 2
    return out


def dense_column(ids, d2v):
    """ids (B, S) rows of d2v (n, D) float32 -> (B, S) float64."""
    x = np.asarray(d2v, dtype=np.float64)
    with np.errstate(all="ignore"):
        sq = np.einsum("nd,nd->n", x, x)
        a, b = ids[:, :-1], ids[:, 1:]
        dots = np.einsum("bpd,bpd->bp", x[a], x[b])
    return neighbor_mean(pair_sims(dots, sq[a], sq[b]))


def sparse_column(ids, indptr, indices, values, n_terms=None):
    """ids (B, S) rows of the CSR table -> (B, S) float64."""
    n = len(indptr) - 1
    n_terms = int(n_terms if n_terms is not None else (indices.max() + 1 if len(indices) else 1))
    m = sp.csr_matrix((np.asarray(values, dtype=np.float64), np.asarray(indices), np.asarray(indptr)), shape=(n, n_terms))
    sq = np.asarray(m.multiply(m).sum(axis=1)).ravel()
    a, b = ids[:, :-1].ravel(), ids[:, 1:].ravel()
    dots = np.asarray(m[a].multiply(m[b]).sum(axis=1)).ravel()
    pair = pair_sims(dots, sq[a], sq[b]).reshape(ids.shape[0], ids.shape[1] - 1)
    return neighbor_mean(pair)


def features(ids, indptr=None, indices=None, values=None, d2v=None):
    """(B, S, columns) float64: the tf-idf column first, then the doc2vec one; a missing table leaves its column out."""
    cols = []
    if indptr is not None:
        cols.append(sparse_column(ids, indptr, indices, values))
    if d2v is not None:
        cols.append(dense_column(ids, d2v))
    return np.stack(cols, axis=2)


def random_rows(rs, lens, n_terms):
    """A CSR table for the tests' generated cases: row i holds about lens[i] distinct terms (a repeated draw is kept once),
    ascending, weights in (0, 1): (indptr int64, indices int32, values float64)."""
    lens = np.asarray(lens, dtype=np.int64)
    rows = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    keys = np.unique(rows * n_terms + rs.randint(0, n_terms, len(rows)))
    indptr = np.zeros(len(lens) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(keys // n_terms, minlength=len(lens)))
    return indptr, (keys % n_terms).astype(np.int32), rs.uniform(0.01, 1.0, len(keys))
