"""BiCut's bag-of-words document input, kept sparse.

The reference builds it in data_prep/document_statics.ipynb (sections "bicut统计数据获取" and "Bicut输入数据"): per ranked
document `[token count, distinct-token count, bag-of-words vector over the 231,448-term dictionary]`;
dataloader/split_bicut_data.py:21-24 puts the retrieval score in front and dataloader/bicut_dataloader.py reads the result back
one densified query (300 x 231,451 numbers) at a time.  Here the statistics file the notebook starts from,

    statics/bicut_stats.pkl    dict[doc_id] -> [token_count, distinct_count, [(term_id, count), ...]]   (term ids ascending)

is packed ONCE into `BowTable`: the bag-of-words rows of the documents of the ranked lists as CSR (int64 indptr, int32 term
ids, float32 counts - the reference's loader ends in `.float()`, and counts are exact in float32), the leading scalar
statistics as one small dense array, and the table's static term -> rows index that the weight-gradient kernel walks
(rlt_sparse_inproj_bwd, include/rlt_hip.h).  A batch is then `Dn` dense columns (score + the scalar statistics) and one table
row number per ranked document: `ops.SparseBatch`.  The input width is taken from the data: I = Dn + V."""
import os
import pickle

import numpy as np
import torch

from . import rank_data
from .doc_features import docs_of

CHUNK = 256          # RLT_SPARSE_CHUNK of include/rlt_hip.h


def term_index(indptr, indices, values, V):
    """The static term -> rows index of a CSR table: (col_ptr (V+1) int64, col_rows int32, col_vals float32, chunk_col int32,
    chunk_ptr (V+1) int32, multi_cols int32) - the table by term, rows ascending, every term owning
    max(1, ceil(entries / CHUNK)) consecutive chunks."""
    n_docs = len(indptr) - 1
    rows = np.repeat(np.arange(n_docs, dtype=np.int32), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    counts = np.bincount(indices, minlength=V).astype(np.int64)
    col_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    k = np.maximum(1, (counts + CHUNK - 1) // CHUNK)
    if int(k.sum()) >= 2 ** 31:
        raise ValueError("the term index needs 2^31 chunks or more")
    chunk_ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    chunk_col = np.repeat(np.arange(V, dtype=np.int32), k)
    multi_cols = np.flatnonzero(k > 1).astype(np.int32)
    return col_ptr, rows[order], values[order].astype(np.float32), chunk_col, chunk_ptr, multi_cols


class BowTable:
    """stats: dict[doc_id] -> [scalar statistics..., [(term, count), ...]] (the reference: token count, distinct-token count,
    then the bag of words); docs: the documents to keep, in row order (docs_of(train, test)); vocab: the dictionary size V, or
    None for 1 + the largest term id of the WHOLE file.  Host arrays until `.to(device)`."""

    _ARRAYS = ("indptr", "indices", "values", "col_ptr", "col_rows", "col_vals", "chunk_col", "chunk_ptr", "multi_cols")

    def __init__(self, stats, docs, vocab=None):
        docs = list(docs)
        if not docs:
            raise ValueError("BowTable: no documents")
        self.row = {d: i for i, d in enumerate(docs)}
        if len(self.row) != len(docs):
            raise ValueError("BowTable: a document is listed twice")
        if vocab is None:
            vocab = 1 + max((row[-1][-1][0] for row in stats.values() if len(row) and len(row[-1])), default=0)
        self.V = int(vocab)
        self.n_docs = len(docs)
        indptr = np.zeros(self.n_docs + 1, dtype=np.int64)
        idx, val, scal = [], [], []
        for i, d in enumerate(docs):
            if d not in stats:
                raise KeyError(f"document {d!r} has no bag-of-words statistics")
            *lead, bow = stats[d]
            if scal and len(lead) != len(scal[0]):
                raise ValueError(f"document {d!r}: {len(lead)} scalar statistics, the documents before it have {len(scal[0])}")
            terms = np.fromiter((t for t, _ in bow), dtype=np.int64, count=len(bow))
            if terms.size and (terms.min() < 0 or terms.max() >= 2 ** 31):
                raise ValueError(f"document {d!r}: term id outside int32")
            if terms.size > 1 and not (np.diff(terms) > 0).all():
                raise ValueError(f"document {d!r}: term ids must be strictly ascending (unsorted or duplicate term)")
            if terms.size and terms.max() >= self.V:
                raise ValueError(f"document {d!r}: term id {int(terms.max())} outside the dictionary of {self.V} terms")
            idx.append(terms.astype(np.int32))
            val.append(np.fromiter((c for _, c in bow), dtype=np.float32, count=len(bow)))
            scal.append([float(v) for v in lead])
            indptr[i + 1] = indptr[i] + len(bow)
        if not 0 < self.V < 2 ** 31 - 16:
            raise ValueError(f"BowTable: dictionary size {self.V} outside int32")
        self.scalars = np.asarray(scal, dtype=np.float32).reshape(self.n_docs, -1)        # (n_docs, Dn - 1)
        if not 1 <= self.Dn <= 16:
            raise ValueError(f"BowTable: {self.Dn} dense columns (score + scalar statistics); the kernels take 1..16")
        self._set_csr(indptr, np.concatenate(idx) if indptr[-1] else np.zeros(0, np.int32),
                      np.concatenate(val) if indptr[-1] else np.zeros(0, np.float32))

    def _set_csr(self, indptr, indices, values):
        self.indptr, self.indices, self.values = indptr, indices, values
        self.col_ptr, self.col_rows, self.col_vals, self.chunk_col, self.chunk_ptr, self.multi_cols = \
            term_index(indptr, indices, values, self.V)
        self.n_chunks, self.n_multi = int(len(self.chunk_col)), int(len(self.multi_cols))
        self.device = None
        self._host = None

    @classmethod
    def from_csr(cls, indptr, indices, values, V, scalars=None):
        """A table from packed arrays (fixtures, benchmarks): rows are documents 0 .. n_docs-1."""
        t = cls.__new__(cls)
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        t.n_docs, t.V = len(indptr) - 1, int(V)
        t.row = {i: i for i in range(t.n_docs)}
        t.scalars = np.zeros((t.n_docs, 0), np.float32) if scalars is None else np.asarray(scalars, np.float32).reshape(t.n_docs, -1)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        if indices.size and (indices.min() < 0 or indices.max() >= t.V):
            raise ValueError(f"BowTable: term id outside the dictionary of {t.V} terms")
        t._set_csr(indptr, indices, np.ascontiguousarray(values, dtype=np.float32))
        return t

    @classmethod
    def from_pickle(cls, path, *raws, vocab=None):
        """The reference's statics/bicut_stats.pkl, restricted to the documents of the ranked lists `raws`."""
        with open(path, "rb") as f:
            return cls(pickle.load(f), docs_of(*raws), vocab)

    @property
    def Dn(self):
        """Dense columns of a batch: the retrieval score, then the scalar statistics."""
        return 1 + self.scalars.shape[1]

    @property
    def n_features(self):
        return self.Dn + self.V

    def to(self, device):
        """Move the arrays to `device` (once; the table is returned itself)."""
        device = torch.device(device)
        if self.device != device:
            if self._host is None:
                self._host = tuple(getattr(self, a) for a in self._ARRAYS)
            # an empty array still needs an address the kernel may be handed: one unused entry
            conv = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(device)
            for name, a in zip(self._ARRAYS, self._host):
                setattr(self, name, conv(a))
            self.device = device
        return self

    def rows_of(self, raw, qids):
        """(len(qids), S) int32 rows of the lists `qids` of `raw` (all of one length)."""
        try:
            return np.array([[self.row[d] for d in raw[q]] for q in qids], dtype=np.int32)
        except KeyError as e:
            raise KeyError(f"document {e.args[0]!r} of a ranked list is not in the table") from None


def _pack_sparse(raw, table, gt):
    """As rank_data._pack, with x (n, S, Dn + 1) float32 = [score, scalar statistics..., table row]: the row number travels
    as the BIT PATTERN of an int32 in the last column (gathers and copies move bits), so that the unchanged BatchLoader
    stages one array per batch."""
    out = {}
    for s, (x, y, qids) in rank_data._pack(raw, None, gt).items():
        rows = table.rows_of(raw, qids)
        xs = np.empty((len(qids), s, table.Dn + 1), dtype=np.float32)
        xs[..., 0] = x[..., 0]
        xs[..., 1:table.Dn] = table.scalars[rows]
        xs[..., table.Dn] = rows.view(np.float32)
        out[s] = (xs, y, qids)
    return out


class BicutData(rank_data.RankData):
    """The splits of `<base>/<retrieve_data>` with BiCut's sparse input: buckets as RankData's, x as _pack_sparse makes it."""

    def __init__(self, retrieve_data="robust04", dataset_name="bm25", base=None, stats=None, vocab=None):
        if stats is None:
            raise ValueError("BicutData: give the path of bicut_stats.pkl (stats=...)")
        base = os.path.join(base or rank_data.DATASET_BASE, retrieve_data)
        gt = rank_data._load_gt(base)
        raws = {split: rank_data._load(os.path.join(base, f"{dataset_name}_{split}.pkl")) for split in ("train", "test")}
        self.table = stats if isinstance(stats, BowTable) else BowTable.from_pickle(stats, raws["train"], raws["test"], vocab=vocab)
        self.buckets = {split: {s: (rank_data._pin(torch.from_numpy(x)), rank_data._pin(torch.from_numpy(y)), qids)
                                for s, (x, y, qids) in sorted(_pack_sparse(raw, self.table, gt).items())}
                        for split, raw in raws.items()}

    @property
    def n_features(self):
        return self.table.n_features


class SparseBatchLoader:
    """A BatchLoader over _pack_sparse buckets -> (ops.SparseBatch, labels): per batch only the `Dn` dense columns and the row
    numbers move to the device; the table is resident there."""

    def __init__(self, loader, table):
        self.loader, self.table = loader, table

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from rlt_hip import ops
        Dn = self.table.Dn
        for x, y in self.loader:
            yield ops.SparseBatch(x[..., :Dn].contiguous(), x[..., Dn].contiguous().view(torch.int32), self.table), y


def bicut_dataloader(retrieve_data="robust04", dataset_name="bm25", batch_size=20, device=None, base=None, seed=None,
                     stats=None, vocab=None):
    """dataloader/bicut_dataloader.py:43-60 (`dataloader(dataset_name, batch_size)`) on the sparse table."""
    data = BicutData(retrieve_data, dataset_name, base, stats, vocab)
    if device is not None:
        data.table.to(device)
    train, test, _ = rank_data._loaders(data, batch_size, device, seed)
    return SparseBatchLoader(train, data.table), SparseBatchLoader(test, data.table), data
