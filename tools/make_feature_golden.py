#!/usr/bin/env python3
"""Generate tests/golden/features_*.npz by RUNNING THE REFERENCE'S data_prep/ notebooks' own functions on generated documents.

CPU only; run in the build container, where the reference is mounted read-only (RLT_REFERENCE, default /root/reference).
The notebooks are read at run time: from their code cells only the function definitions iv2dense, cos_simi, ranked_list,
simi_docs, simi_list (data_review.ipynb) and cos_similarity, neighbor_sim (document_statics.ipynb) are executed, each notebook
into a namespace of its own that holds the generated `tfidf_dense` / `doc2vec` dictionaries, with tqdm stubbed.  Nothing from
the reference is written into this repository: the fixtures hold the generated tables and lists and what the notebook code
returned for them (data).

    python tools/make_feature_golden.py        # regenerates every tests/golden/features_*.npz

Each file holds one document table
    indptr (n+1) int64, indices int32 (ascending per row), values float64     the tf-idf rows, CSR;  n_terms
    d2v (n, 200) float32                                                        the doc2vec rows
and per list length S the lists and the notebooks' results
    ids_s<S> (B, S) int32        rows of the table, rank order
    tfidf_s<S> (B, S) float64    the tf-idf column as the notebook returned it
    d2v_s<S> (B, S) float32      the doc2vec column as the notebook returned it (it computes that one in float32)
features_robust_s300.npz goes through data_review.ipynb's simi_list (which knows 300 positions only), features_edge_s40.npz
through document_statics.ipynb's neighbor_sim (any length: 40 and 2).

When a file is written, the notebook's float32 doc2vec column must lie within 3 (D + 2) 2^-24 of a float64 evaluation of the
same formula (the bound tests/test_features_gpu.py grants the fixture); an input for which it does not is to be changed, not
the bound."""
import ast
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RLT_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")
WANTED = {"data_review": {"iv2dense", "cos_simi", "ranked_list", "simi_docs", "simi_list"},
          "document_statics": {"cos_similarity", "neighbor_sim"}}
D = 200
U = 2.0 ** -24


def notebook_namespace(name, **extra):
    """The wanted function definitions of data_prep/<name>.ipynb executed into a fresh namespace."""
    with open(os.path.join(REF, "data_prep", name + ".ipynb")) as f:
        nb = json.load(f)
    defs = []
    for cell in nb["cells"]:
        if cell["cell_type"] != "code":
            continue
        try:
            tree = ast.parse("".join(cell["source"]))
        except SyntaxError:                 # notebook-only syntax in cells we do not need
            continue
        defs += [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED[name]]
    assert {d.name for d in defs} == WANTED[name], sorted(d.name for d in defs)
    ns = {"np": np, "tqdm": lambda it, **kw: it}
    ns.update(extra)
    exec(compile(ast.Module(body=defs, type_ignores=[]), f"data_prep/{name}.ipynb", "exec"), ns)
    return ns


def robust_like_table(rs, n_docs, n_terms, empty_share=0.02):
    """tf-idf rows that look like robust04's: most below 64 entries, a tail of a few hundred, some empty; popular terms are
    drawn more often, so neighbouring documents share some.  (indptr int64, indices int32 ascending per row, values float64).
    Vectorised: tools/bench_kernels.py draws 131,072 rows with it."""
    lens = np.minimum(rs.lognormal(3.3, 0.6, n_docs).astype(np.int64) + 1, 400)
    lens[rs.uniform(size=n_docs) < empty_share] = 0
    rows = np.repeat(np.arange(n_docs, dtype=np.int64), lens)
    terms = (n_terms * rs.uniform(size=len(rows)) ** 2).astype(np.int64)
    keys = np.unique(rows * n_terms + terms)            # a term drawn twice for a row is kept once
    indptr = np.zeros(n_docs + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(keys // n_terms, minlength=n_docs))
    return indptr, (keys % n_terms).astype(np.int32), rs.uniform(0.01, 1.0, len(keys))


def csr_from_rows(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r[0]) for r in rows])
    return (indptr, np.concatenate([np.asarray(r[0], dtype=np.int32) for r in rows]),
            np.concatenate([np.asarray(r[1], dtype=np.float64) for r in rows]))


def as_dicts(indptr, indices, values, d2v):
    """The reference's dictionaries: tfidf[doc] = [(term, weight)], doc2vec[doc] = float32 vector; documents named d<row>."""
    name = lambda i: f"d{i}"
    tfidf = {name(i): [(int(t), float(w)) for t, w in zip(indices[indptr[i]:indptr[i + 1]], values[indptr[i]:indptr[i + 1]])]
             for i in range(len(indptr) - 1)}
    return tfidf, {name(i): d2v[i] for i in range(len(d2v))}


def float64_d2v_column(ids, d2v):
    """The notebook's formula for the doc2vec column evaluated in float64 (the generator's own check)."""
    x = d2v.astype(np.float64)
    with np.errstate(all="ignore"):
        a, b = x[ids[:, :-1]], x[ids[:, 1:]]
        denom = np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1))
        sim = np.where(denom != 0, (a * b).sum(-1) / denom, 0.0)
    sim = np.where(np.isnan(sim), 0.0, sim)
    out = np.empty(ids.shape, dtype=np.float64)
    out[:, 0], out[:, -1] = sim[:, 0], sim[:, -1]
    out[:, 1:-1] = (sim[:, :-1] + sim[:, 1:]) / 2
    return out


def as_float32(col):
    """The notebook's doc2vec column: numpy float32 values, with a python 0 where its zero-denominator / NaN rule answered.
    Every value must BE a float32 value - the notebook computed that column in float32."""
    arr = np.array(col, dtype=np.float64)
    assert np.array_equal(arr.astype(np.float32).astype(np.float64), arr)
    assert any(isinstance(v, np.float32) for row in col for v in row)
    return arr.astype(np.float32)


def check_and_pack(out, S, ids, tf_col, dv_col, d2v):
    tf_col, dv_col = np.asarray(tf_col, dtype=np.float64), np.asarray(dv_col)
    assert dv_col.dtype == np.float32, dv_col.dtype            # the notebooks evaluate this column in float32
    err = float(np.abs(dv_col.astype(np.float64) - float64_d2v_column(ids, d2v)).max())
    assert err <= 3 * (D + 2) * U, (S, err)
    out[f"ids_s{S}"], out[f"tfidf_s{S}"], out[f"d2v_s{S}"] = ids.astype(np.int32), tf_col, dv_col
    return err


def robust_set(rs):
    n_docs, n_terms, S = 150, 4000, 300
    indptr, indices, values = robust_like_table(rs, n_docs, n_terms)
    d2v = (rs.standard_normal((n_docs, D)) * 0.3 + rs.standard_normal((n_docs, 1)) * 0.1).astype(np.float32)
    ids = rs.randint(0, n_docs, (3, S))
    ids[0, 10] = ids[0, 11]                                     # a document next to itself
    ids[1, 0] = ids[1, 1]
    ids[2, S - 1] = ids[2, S - 2]
    tfidf, doc2vec = as_dicts(indptr, indices, values, d2v)
    ns = notebook_namespace("data_review")
    # a score dictionary cannot hold a document twice, and the lists repeat documents: position j of list b holds the alias
    # d<row>@<b>.<j>, a key of its own for the same two vectors, so the notebook's own ranked_list runs on the dictionary
    dense = {d: ns["iv2dense"](iv, n_terms) for d, iv in tfidf.items()}
    alias = [[f"d{i}@{b}.{j}" for j, i in enumerate(row)] for b, row in enumerate(ids)]
    ns["tfidf_dense"] = {al: dense[al.split("@")[0]] for row in alias for al in row}
    ns["doc2vec"] = {al: doc2vec[al.split("@")[0]] for row in alias for al in row}
    dataset = {f"q{b}": {al: float(S - j) for j, al in enumerate(row)} for b, row in enumerate(alias)}
    sl = ns["simi_list"](dataset)
    tf_col = np.array([[p[0] for p in sl[f"q{b}"]] for b in range(len(ids))], dtype=np.float64)
    dv_col = as_float32([[p[1] for p in sl[f"q{b}"]] for b in range(len(ids))])
    out = {"indptr": indptr, "indices": indices, "values": values, "n_terms": np.int64(n_terms), "d2v": d2v}
    err = check_and_pack(out, S, ids, tf_col, dv_col, d2v)
    return out, err


def edge_set(rs):
    n_terms = 6000
    indptr, indices, values = robust_like_table(rs, 24, n_terms, empty_share=0.0)
    rows = [(indices[indptr[i]:indptr[i + 1]], values[indptr[i]:indptr[i + 1]]) for i in range(24)]
    d2v = (rs.standard_normal((24, D)) * 0.3).astype(np.float32)
    d2v[1] = 0.0                                                # an all-zero doc2vec vector
    rows[2] = rows[3] = (np.zeros(0, np.int32), np.zeros(0))    # two empty tf-idf rows
    even, odd = np.arange(0, 120, 2), np.arange(1, 121, 2)      # two documents with disjoint terms
    rows[5], rows[6] = (even, rs.uniform(0.01, 1, len(even))), (odd, rs.uniform(0.01, 1, len(odd)))
    long_terms = np.sort(rs.choice(n_terms, 3000, replace=False))
    rows[7] = (long_terms, rs.uniform(0.01, 1, 3000))           # one row of 3000 entries
    d2v[8, 17] = np.nan                                         # a doc2vec vector holding a NaN
    rows[9] = (long_terms[::7], rs.uniform(0.01, 1, len(long_terms[::7])))   # 429 entries, all shared with the long row
    indptr, indices, values = csr_from_rows(rows)
    tfidf, doc2vec = as_dicts(indptr, indices, values, d2v)
    ns = notebook_namespace("document_statics")
    iv2dense = notebook_namespace("data_review")["iv2dense"]
    dense = {d: iv2dense(iv, n_terms) for d, iv in tfidf.items()}
    head = [4, 2, 3, 4, 5, 6, 7, 0, 7, 7, 9, 7, 8, 0, 1, 0, 1, 1, 2, 2]
    lists = {40: np.array([head + list(rs.randint(0, 24, 20)), list(rs.randint(0, 24, 20)) + head[::-1],
                           list(rs.randint(0, 24, 40))]),
             2: np.array([[2, 3], [0, 1], [7, 0], [0, 0], [8, 0], [5, 6], [3, 4], [7, 9]])}
    out = {"indptr": indptr, "indices": indices, "values": values, "n_terms": np.int64(n_terms), "d2v": d2v}
    errs = []
    for S, ids in lists.items():
        tf_col = [ns["neighbor_sim"]([dense[f"d{i}"] for i in row], "x") for row in ids]
        dv_col = as_float32([ns["neighbor_sim"]([doc2vec[f"d{i}"] for i in row], "x") for row in ids])
        errs.append(check_and_pack(out, S, ids, tf_col, dv_col, d2v))
    return out, max(errs)


def main():
    os.makedirs(OUT, exist_ok=True)
    rs = np.random.RandomState(20261016)
    for name, make in (("features_robust_s300", robust_set), ("features_edge_s40", edge_set)):
        out, err = make(rs)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        nnz = np.diff(out["indptr"])
        print(f"{path}: {os.path.getsize(path)} bytes, {len(nnz)} documents, row lengths median {int(np.median(nnz))} max "
              f"{int(nnz.max())} empty {int((nnz == 0).sum())}; notebook float32 doc2vec column within {err:.3e} "
              f"({err / U:.2f} u) of float64")


if __name__ == "__main__":
    sys.exit(main())
