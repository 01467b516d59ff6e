"""AttnCut's neighbour-similarity statistics, computed instead of read.

The reference makes `<base>/<retrieve_data>/attncut/<name>_{train,test}.pkl` in two notebooks
(data_prep/data_review.ipynb: cos_simi / simi_docs / simi_list; data_prep/document_statics.ipynb: cos_similarity /
neighbor_sim) from two document tables:

    statics/tfidf.pkl      dict[doc_id] -> list[(term_id, weight)], gensim bag-of-words order (term ids ascending)
    statics/doc2vec.pkl    dict[doc_id] -> float32 vector (200 wide)

`DocTable` packs both once - tf-idf as CSR (int64 indptr, int32 term ids, float64 weights), doc2vec as one dense float32
array - restricted to the documents that occur in the given ranked lists (the notebook's `doc_set`), and keeps the
doc_id -> row map.  `neighbor_stats` turns ranked lists into rows of that table and runs rlt_neighbor_features once per list
length; what comes back has the on-disk layout `dict[qid] -> list[S][2]` that rank_data.py reads, column 0 the tf-idf
similarity and column 1 the doc2vec one, as simi_docs orders them.

Two departures from the notebooks, both stated in INTEGRATION.md: the doc2vec column is accumulated in float64 and rounded
once (the notebooks evaluate it in float32), and tf-idf rows stay sparse (the notebooks densify each to 231,448 float64)."""
import pickle

import numpy as np
import torch


def docs_of(*raws):
    """The documents of ranked lists `dict[qid] -> dict[doc_id -> score]`, each once, in order of first occurrence."""
    seen = {}
    for raw in raws:
        for docs in raw.values():
            for d in docs:
                seen.setdefault(d, None)
    return list(seen)


class DocTable:
    """tfidf: dict[doc_id] -> [(term, weight)] or None; doc2vec: dict[doc_id] -> vector or None (not both None);
    docs: the documents to keep, in row order (docs_of(train, test)).  Host arrays until `.to(device)`."""

    def __init__(self, tfidf, doc2vec, docs):
        if tfidf is None and doc2vec is None:
            raise ValueError("DocTable: give tfidf, doc2vec or both")
        docs = list(docs)
        if not docs:
            raise ValueError("DocTable: no documents")
        self.row = {d: i for i, d in enumerate(docs)}
        if len(self.row) != len(docs):
            raise ValueError("DocTable: a document is listed twice")
        self.n_docs = len(docs)
        self.indptr = self.indices = self.values = self.d2v = None
        self.device = None
        self._host = None
        if tfidf is not None:
            indptr = np.zeros(self.n_docs + 1, dtype=np.int64)
            idx, val = [], []
            for i, d in enumerate(docs):
                if d not in tfidf:
                    raise KeyError(f"document {d!r} has no tf-idf row")
                row = tfidf[d]
                terms = np.fromiter((t for t, _ in row), dtype=np.int64, count=len(row))
                if terms.size and (terms.min() < 0 or terms.max() >= 2 ** 31):
                    raise ValueError(f"document {d!r}: term id outside int32")
                if terms.size > 1 and not (np.diff(terms) > 0).all():
                    raise ValueError(f"document {d!r}: term ids must be strictly ascending (unsorted or duplicate term)")
                idx.append(terms.astype(np.int32))
                val.append(np.fromiter((w for _, w in row), dtype=np.float64, count=len(row)))
                indptr[i + 1] = indptr[i] + len(row)
            self.indptr = indptr
            self.indices = np.concatenate(idx) if indptr[-1] else np.zeros(0, dtype=np.int32)
            self.values = np.concatenate(val) if indptr[-1] else np.zeros(0, dtype=np.float64)
        if doc2vec is not None:
            width = None
            for d in docs:
                if d not in doc2vec:
                    raise KeyError(f"document {d!r} has no doc2vec vector")
                w = np.asarray(doc2vec[d]).shape
                if len(w) != 1 or w[0] < 1 or w[0] > 1024:
                    raise ValueError(f"document {d!r}: doc2vec vector of shape {w}, expected one dimension of 1..1024")
                if width is None:
                    width = w[0]
                elif w[0] != width:
                    raise ValueError(f"document {d!r}: doc2vec vector of width {w[0]}, the documents before it have {width}")
            self.d2v = np.stack([np.asarray(doc2vec[d], dtype=np.float32) for d in docs])

    @classmethod
    def from_pickles(cls, tfidf_path, doc2vec_path, *raws):
        """The reference's statics/tfidf.pkl and statics/doc2vec.pkl (either path may be None), restricted to the documents of
        the ranked lists `raws`."""
        load = lambda p: None if p is None else pickle.load(open(p, "rb"))
        return cls(load(tfidf_path), load(doc2vec_path), docs_of(*raws))

    @property
    def n_columns(self):
        return (self.indptr is not None) + (self.d2v is not None)

    def to(self, device):
        """Move the arrays to `device` (once; the table is returned itself)."""
        device = torch.device(device)
        if self.device != device:
            if self._host is None:
                self._host = (self.indptr, self.indices, self.values, self.d2v)
            # an empty CSR still needs addresses the kernel may be handed: one unused entry
            conv = lambda a: None if a is None else torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(device)
            self.indptr, self.indices, self.values, self.d2v = (conv(a) for a in self._host)
            self.device = device
        return self

    def rows_of(self, raw, qids):
        """(len(qids), S) int32 rows of the lists `qids` of `raw` (all of one length)."""
        try:
            return np.array([[self.row[d] for d in raw[q]] for q in qids], dtype=np.int32)
        except KeyError as e:
            raise KeyError(f"document {e.args[0]!r} of a ranked list is not in the table") from None


def neighbor_stats(raw, table, device=None):
    """raw: dict[qid] -> dict[doc_id -> score] in rank order -> dict[qid] -> list[S][columns] (python floats: what the
    reference pickles), computed on the GPU: lists bucketed by length as rank_data._pack does, one kernel pass per bucket."""
    from rlt_hip import ops
    device = torch.device(device if device is not None else (table.device or "cuda"))
    table.to(device)
    by_len = {}
    for q, docs in raw.items():
        by_len.setdefault(len(docs), []).append(q)
    out = {}
    for s, qids in by_len.items():
        if s < 2:
            raise ValueError(f"query {qids[0]}: a ranked list of {s} documents has no neighbours (at least 2 needed)")
        ids = torch.from_numpy(table.rows_of(raw, qids)).to(device)
        feats = ops.neighbor_features(ids, table, validate=False).cpu().numpy()       # rows come from the table's own map
        for i, q in enumerate(qids):
            out[q] = feats[i].tolist()
    return {q: out[q] for q in raw}
