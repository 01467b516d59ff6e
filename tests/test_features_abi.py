"""AttnCut's neighbour-similarity statistics (rlt_neighbor_features, dataloader/doc_features.py, prepare_features.py) without a
GPU: the C ABI is declared, bound and exported, its argument errors are answered before any launch, DocTable packs the
reference's dictionaries and names the document of a bad row, the script offers its flags, and the committed notebook fixtures
agree with the independent numpy restatement of tests/feature_restate.py.

The entry point takes no workspace (one launch, nothing between launches to keep), so there is no workspace query and no
undersized-workspace error to answer.

Notebook fixtures against the float64 restatement, as measured here: tf-idf column at most 2.2e-16 apart (both float64);
doc2vec column (the notebook's own float32 arithmetic) at most 1.2e-7 = 2.0 u apart, u = 2^-24, under the granted
3 (D + 2) u = 3.6e-5."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_restate as R  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "features_*.npz")))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbol_declared_bound_exported(native):
    assert "rlt_neighbor_features" in native.EXPORTS
    assert hasattr(native.load(), "rlt_neighbor_features")
    assert native.load().rlt_abi_version() == 5


def test_argument_errors_before_any_launch(native):
    lib = native.load()
    buf = (ctypes.c_uint8 * (1 << 16))()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    x = ctypes.c_void_p(base)
    at = lambda off: ctypes.c_void_p(base + off)

    def call(ids=x, B=4, S=40, n_docs=10, d2v=x, D=200, ld=200, indptr=x, indices=x, values=x, out=x, ld_out=3, col=1):
        return lib.rlt_neighbor_features(ids, B, S, n_docs, d2v, D, ld, indptr, indices, values, out, ld_out, col, None)

    assert call(S=1) == -1 and call(S=0) == -1                                    # the notebooks index positions 0 and 1
    assert call(B=0) == -1 and call(B=-1) == -1
    assert call(n_docs=0) == -1
    assert call(ids=None) == -1 and call(out=None) == -1
    assert call(D=0) == -1
    assert call(D=1025, ld=1025) == -2
    assert call(D=200, ld=199) == -1                                              # row stride below the row width
    assert call(d2v=None, indptr=None, indices=None, values=None) == -1          # both tables NULL
    assert call(indptr=None) == -1 and call(values=None) == -1 and call(indices=None) == -1      # a partial CSR table
    assert call(B=1 << 20, S=1 << 11) == -2                                       # B * S >= 2^31
    assert call(col=-1) == -1
    assert call(ld_out=2, col=1) == -1                                            # two columns do not fit
    assert call(values=at(4)) == -4                                               # float64 weights off an 8-byte boundary
    assert call(indptr=at(4)) == -4
    assert call(d2v=at(2)) == -4 and call(out=at(2)) == -4 and call(ids=at(1)) == -4 and call(indices=at(2)) == -4


def test_prepare_features_help_lists_the_flags():
    res = subprocess.run([sys.executable, os.path.join(REPO, "ranked-list-truncation_amd", "prepare_features.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    for flag in ("--dataset-base", "--retrieve-data", "--dataset-name", "--tfidf", "--doc2vec"):
        assert flag in res.stdout


def test_loader_signatures_keep_their_positional_arguments():
    import inspect
    from dataloader import rank_data
    assert list(inspect.signature(rank_data.attncut_dataloader).parameters) == [
        "retrieve_data", "dataset_name", "batch_size", "device", "base", "seed", "doc_table"]
    assert list(inspect.signature(rank_data.RankData.__init__).parameters) == [
        "self", "retrieve_data", "dataset_name", "with_stats", "base", "stats_dir", "doc_table"]
    assert inspect.signature(rank_data.attncut_dataloader).parameters["doc_table"].default is None


# ------------------------------------------------------------------------------ DocTable
def _dicts():
    tfidf = {"a": [(0, 0.5), (7, 0.25)], "b": [], "c": [(3, 1.0)], "unused": [(1, 1.0)]}
    d2v = {"a": np.array([1, 2, 3], np.float32), "b": np.zeros(3, np.float32), "c": [0.5, 0.5, 0.5],
           "unused": np.ones(3, np.float32)}
    return tfidf, d2v


def test_doctable_packs_the_documents_of_the_lists():
    from dataloader.doc_features import DocTable, docs_of
    tfidf, d2v = _dicts()
    raw = {"q1": {"c": 3.0, "a": 2.0}, "q2": {"a": 9.0, "b": 1.0}}
    docs = docs_of(raw)
    assert docs == ["c", "a", "b"]                          # first occurrence; `unused` stays out
    t = DocTable(tfidf, d2v, docs)
    assert t.n_docs == 3 and t.row == {"c": 0, "a": 1, "b": 2} and t.n_columns == 2
    assert t.indptr.dtype == np.int64 and t.indices.dtype == np.int32 and t.values.dtype == np.float64
    assert t.indptr.tolist() == [0, 1, 3, 3] and t.indices.tolist() == [3, 0, 7] and t.values.tolist() == [1.0, 0.5, 0.25]
    assert t.d2v.dtype == np.float32 and t.d2v.shape == (3, 3) and t.d2v[1].tolist() == [1.0, 2.0, 3.0]
    assert t.rows_of(raw, ["q2", "q1"]).tolist() == [[1, 2], [0, 1]] and t.rows_of(raw, ["q1"]).dtype == np.int32
    assert DocTable(None, d2v, docs).n_columns == 1 and DocTable(tfidf, None, docs).indptr is not None


def test_doctable_errors_name_the_document():
    from dataloader.doc_features import DocTable
    tfidf, d2v = _dicts()
    with pytest.raises(ValueError, match="'a'.*ascending"):
        DocTable({**tfidf, "a": [(7, 0.25), (0, 0.5)]}, d2v, ["c", "a"])              # unsorted
    with pytest.raises(ValueError, match="'a'.*ascending"):
        DocTable({**tfidf, "a": [(3, 0.25), (3, 0.5)]}, d2v, ["c", "a"])              # duplicate term
    with pytest.raises(KeyError, match="'zz'.*tf-idf"):
        DocTable(tfidf, d2v, ["a", "zz"])
    with pytest.raises(KeyError, match="'b'.*doc2vec"):
        DocTable(tfidf, {k: v for k, v in d2v.items() if k != "b"}, ["a", "b"])
    with pytest.raises(ValueError, match="'c'.*width 4"):
        DocTable(tfidf, {**d2v, "c": np.zeros(4, np.float32)}, ["a", "c"])
    with pytest.raises(ValueError):
        DocTable(None, None, ["a"])
    with pytest.raises(ValueError):
        DocTable(tfidf, d2v, [])
    t = DocTable(tfidf, d2v, ["a", "b"])
    with pytest.raises(KeyError, match="'c'.*not in the table"):
        t.rows_of({"q": {"a": 1.0, "c": 0.5}}, ["q"])


def test_ops_rejects_bad_arguments_without_a_gpu():
    import torch
    from rlt_hip import ops
    from dataloader.doc_features import DocTable
    tfidf, d2v = _dicts()
    t = DocTable(tfidf, d2v, ["a", "b", "c"])
    with pytest.raises(ValueError, match="int32"):
        ops.neighbor_features(torch.zeros((2, 3), dtype=torch.int64), t)
    with pytest.raises(ValueError, match="at least 2"):
        ops.neighbor_features(torch.zeros((2, 1), dtype=torch.int32), t)


# ------------------------------------------------------------------------------ fixtures
def test_there_are_two_fixtures():
    assert [os.path.basename(f) for f in FIXTURES] == ["features_edge_s40.npz", "features_robust_s300.npz"]
    for f in FIXTURES:
        assert os.path.getsize(f) < 440 * 1024


def _lengths(d):
    return sorted(int(k[5:]) for k in d.files if k.startswith("ids_s"))


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_fixtures_agree_with_the_numpy_restatement(path):
    d = np.load(path)
    D = d["d2v"].shape[1]
    assert D == 200 and d["d2v"].dtype == np.float32 and d["values"].dtype == np.float64 and d["indptr"].dtype == np.int64
    for i in range(len(d["indptr"]) - 1):
        row = d["indices"][d["indptr"][i]:d["indptr"][i + 1]]
        assert (np.diff(row) > 0).all()
    for S in _lengths(d):
        ids = d[f"ids_s{S}"]
        assert ids.shape[1] == S and ids.min() >= 0 and ids.max() < len(d["d2v"])
        got = R.features(ids, d["indptr"], d["indices"], d["values"], d["d2v"])
        e_tf = np.abs(got[..., 0] - d[f"tfidf_s{S}"]).max()
        e_dv = np.abs(got[..., 1] - d[f"d2v_s{S}"].astype(np.float64)).max()
        print(f"{os.path.basename(path)} S={S}: tf-idf {e_tf:.3e}, doc2vec {e_dv:.3e} ({e_dv / U:.2f} u)")
        assert e_tf < 1e-12                                     # float64 against float64, sums in another order
        assert e_dv <= 3 * (D + 2) * U                          # the notebook's float32 evaluation: its own error bound
        # where the notebook answered 0 by its zero-denominator / NaN rule at both neighbours, so does the restatement
        assert (got[..., 0][d[f"tfidf_s{S}"] == 0] == 0).all() and (got[..., 1][d[f"d2v_s{S}"] == 0] == 0).all()
        # single-table calls give the same columns
        assert np.array_equal(R.features(ids, d["indptr"], d["indices"], d["values"])[..., 0], got[..., 0])
        assert np.array_equal(R.features(ids, d2v=d["d2v"])[..., 0], got[..., 1])


def test_fixtures_hold_the_cases_they_were_made_for():
    d = np.load(os.path.join(REPO, "tests", "golden", "features_robust_s300.npz"))
    ids = d["ids_s300"]
    assert ids.shape == (3, 300) and (ids[:, 1:] == ids[:, :-1]).any()                  # a document next to itself
    nnz = np.diff(d["indptr"])
    assert (nnz == 0).any() and np.median(nnz) < 64
    e = np.load(os.path.join(REPO, "tests", "golden", "features_edge_s40.npz"))
    nnz = np.diff(e["indptr"])
    assert nnz.max() == 3000 and (nnz == 0).sum() >= 2
    assert _lengths(e) == [2, 40]
    assert np.isnan(e["d2v"]).any(1).sum() == 1 and (e["d2v"] == 0).all(1).sum() == 1
    ids = e["ids_s40"]
    pairs = {(int(a), int(b)) for row in ids for a, b in zip(row[:-1], row[1:])}
    empty = set(np.flatnonzero(nnz == 0))
    assert any(a in empty and b in empty for a, b in pairs) and any((a in empty) != (b in empty) for a, b in pairs)
    rows = lambda i: set(e["indices"][e["indptr"][i]:e["indptr"][i + 1]].tolist())
    assert any(rows(a) and rows(b) and not (rows(a) & rows(b)) for a, b in pairs)       # disjoint terms
    assert (e["tfidf_s40"] == 0).any() and (e["d2v_s40"] == 0).any() and (e["d2v_s2"] == 0).any()


def test_the_restatement_on_a_case_worked_by_hand():
    # three documents: a = (3, 4) on terms 0, 1; b = (4, 3); c empty.  sim(a, b) = 24 / 25, sim(b, c) = 0.
    indptr = np.array([0, 2, 4, 4], dtype=np.int64)
    indices = np.array([0, 1, 0, 1], dtype=np.int32)
    values = np.array([3.0, 4.0, 4.0, 3.0])
    d2v = np.array([[1, 0], [0, 1], [1, 1]], dtype=np.float32)
    got = R.features(np.array([[0, 1, 2]]), indptr, indices, values, d2v)
    np.testing.assert_allclose(got[0, :, 0], [0.96, 0.48, 0.0], rtol=0, atol=1e-15)
    r = 1 / np.sqrt(2)
    np.testing.assert_allclose(got[0, :, 1], [0.0, r / 2, r], rtol=0, atol=1e-15)
