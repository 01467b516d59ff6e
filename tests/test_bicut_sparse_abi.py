"""BiCut on its sparse bag-of-words input (rlt_sparse_inproj_*, rlt_bilstm_sparse_*, models.BiCut(sparse_input=True),
dataloader/bicut_data.py, run.py --bicut-stats) without a GPU: the C ABI is declared, bound and exported, every argument error
is answered before any launch (also under the host-only ASan + UBSan build), BowTable packs the reference's statistics
dictionary and names the document of a bad row, a sparse model keeps the reference's state_dict contract, and the committed
reference fixtures agree with the independent float64 restatement of tests/bicut_sparse_restate.py.

The fixture bounds compare float64 against the REFERENCE's float32 run, so they bound the reference's rounding: out0 1e-6
absolute, k_s identical, losses 1e-6 relative, sampled gradient columns and norms 1e-5 relative to the column's (the matrix's)
norm.  Measured here:
  bicut_sparse_v2048_b6_s40    out0 6.1e-08, losses 5.5e-08 / 6.0e-08, columns 2.9e-07, column norms 5.3e-07, parameters 1.1e-07
  bicut_sparse_v231448_b2_s40  out0 5.0e-08, losses 1.0e-07 / 6.9e-09, columns 6.2e-07, parameters 1.9e-07"""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bicut_sparse_restate as R  # noqa: E402
from golden_util import probe_index  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "bicut_sparse_*.npz")))
NEW = ("rlt_sparse_inproj_workspace", "rlt_sparse_inproj_fwd", "rlt_sparse_inproj_bwd",
       "rlt_bilstm_sparse_workspace", "rlt_bilstm_sparse_fwd", "rlt_bilstm_sparse_bwd")

# the argument errors of the header, as a script: run against the normal library here and against the sanitized one in a child
ERRORS = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/ranked-list-truncation_amd")
from rlt_hip import native as N
lib = N.load()
assert lib.rlt_abi_version() == 5
buf = (ctypes.c_uint8 * (1 << 22))()
base = ctypes.addressof(buf)
base += (-base) % 256
x = ctypes.c_void_p(base)
S, B, Dn, n_docs, V = 3, 5, 3, 10, 64
n_chunks, n_multi = V + 2, 1

def batch(**kw):
    sb = N.SparseBatchPtrs()
    for f in N.SPARSE_POINTERS:
        setattr(sb, f, base)
    sb.Dn, sb.n_docs, sb.V, sb.n_chunks, sb.n_multi = Dn, n_docs, V, n_chunks, n_multi
    for k, v in kw.items():
        setattr(sb, k, v)
    return sb

ws_b = N.query("rlt_sparse_inproj_workspace", S, B, Dn, n_docs, V, n_chunks)
assert ws_b > 0 and ws_b % 256 == 0
for bad in ((0, B, Dn, n_docs, V, n_chunks), (S, 0, Dn, n_docs, V, n_chunks), (S, B, 0, n_docs, V, n_chunks), (S, B, 17, n_docs, V, n_chunks),
            (S, B, Dn, 0, V, n_chunks), (S, B, Dn, n_docs, 0, n_chunks), (S, B, Dn, n_docs, V, V - 1), (1 << 16, 1 << 15, Dn, n_docs, V, n_chunks)):
    assert N.query("rlt_sparse_inproj_workspace", *bad) == 0, bad
    assert N.query("rlt_bilstm_sparse_workspace", *bad) == 0, bad
assert N.query("rlt_bilstm_sparse_workspace", S, B, Dn, n_docs, V, n_chunks) > ws_b

def fwd(sb, S=S, B=B, w=x, bias=x, gates=x):
    return lib.rlt_sparse_inproj_fwd(ctypes.byref(sb) if sb is not None else None, S, B, w, w, bias, bias, bias, bias, gates, None)

def bwd(sb, S=S, B=B, dg=x, dw=x, db=x, ws=x, ws_bytes=ws_b):
    return lib.rlt_sparse_inproj_bwd(ctypes.byref(sb) if sb is not None else None, S, B, dg, dw, dw, db, db, db, db, ws, ws_bytes, None)

at = lambda off: base + off
for call in (fwd, bwd):
    assert call(None) == -1
    assert call(batch(), S=0) == -1 and call(batch(), B=-1) == -1
    for f in ("dense", "ids", "indptr", "indices", "values"):
        assert call(batch(**{f: None})) == -1, f
    assert call(batch(Dn=0)) == -1 and call(batch(V=0)) == -1 and call(batch(n_docs=0)) == -1
    assert call(batch(Dn=17)) == -2
    assert call(batch(), S=1 << 16, B=1 << 15) == -2                              # B * S >= 2^31
    assert call(batch(V=(1 << 31) - 2)) == -2                                     # Dn + V >= 2^31
    assert call(batch(indptr=at(4))) == -4 and call(batch(values=at(2))) == -4    # int64 offsets off 8 bytes, float32 off 4
    assert call(batch(ids=at(1))) == -4 and call(batch(indices=at(2))) == -4 and call(batch(dense=at(3))) == -4
assert fwd(batch(), w=None) == -1 and fwd(batch(), bias=None) == -1 and fwd(batch(), gates=None) == -1
assert fwd(batch(), w=ctypes.c_void_p(at(4))) == -4 and fwd(batch(), gates=ctypes.c_void_p(at(8))) == -4
assert fwd(batch(), bias=ctypes.c_void_p(at(4))) == -4
for f in ("perm", "col_ptr", "col_rows", "col_vals", "chunk_col", "chunk_ptr", "multi_cols"):
    assert bwd(batch(**{f: None})) == -1, f
assert bwd(batch(n_chunks=V - 1)) == -1 and bwd(batch(n_multi=-1)) == -1 and bwd(batch(n_multi=0)) == -1
assert bwd(batch(n_chunks=V, n_multi=1)) == -1                                    # one chunk per term, yet a multi-chunk term
assert bwd(batch(col_ptr=at(4))) == -4 and bwd(batch(perm=at(2))) == -4 and bwd(batch(col_vals=at(1))) == -4
assert bwd(batch(), dg=None) == -1 and bwd(batch(), dw=None) == -1 and bwd(batch(), db=None) == -1 and bwd(batch(), ws=None) == -1
assert bwd(batch(), dw=ctypes.c_void_p(at(4))) == -4 and bwd(batch(), dg=ctypes.c_void_p(at(8))) == -4
assert bwd(batch(), ws=ctypes.c_void_p(at(8))) == -4 and bwd(batch(), db=ctypes.c_void_p(at(2))) == -4
assert bwd(batch(), ws_bytes=ws_b - 1) == -3
# path level: stash / workspace sizes answered before any layout pointer is formed
lw = (N.LstmLayerPtrs * 2)()
for l in range(2):
    for f in ("w_ih", "w_hh", "b_ih", "b_hh"):
        getattr(lw[l], f)[0] = base
        getattr(lw[l], f)[1] = base
st_b = N.query("rlt_workspace_bytes", N.OP_BILSTM_STASH, S, B, 256, 0, 0, 0, 0)
pw_b = N.query("rlt_bilstm_sparse_workspace", S, B, Dn, n_docs, V, n_chunks)
sb = batch()
assert lib.rlt_bilstm_sparse_fwd(ctypes.byref(sb), lw, S, B, x, x, st_b - 1, x, pw_b, 0, None) == -3
assert lib.rlt_bilstm_sparse_fwd(None, lw, S, B, x, x, st_b, x, pw_b, 0, None) == -1
assert lib.rlt_bilstm_sparse_fwd(ctypes.byref(sb), lw, S, B, x, x, st_b, x, pw_b, 7, None) == -1      # no such precision code
assert lib.rlt_bilstm_sparse_bwd(ctypes.byref(sb), lw, x, x, S, B, x, st_b - 1, lw, x, pw_b, 0, None) == -3
assert lib.rlt_bilstm_sparse_bwd(ctypes.byref(sb), lw, x, x, S, B, x, st_b, lw, x, pw_b - 1, 0, None) == -3
assert lib.rlt_bilstm_sparse_bwd(ctypes.byref(sb), lw, x, None, S, B, x, st_b, lw, x, pw_b, 0, None) == -1
bad = batch(Dn=17)
assert lib.rlt_bilstm_sparse_bwd(ctypes.byref(bad), lw, x, x, S, B, x, st_b, lw, x, pw_b, 0, None) == -1
print("errors ok")
"""


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbols_declared_bound_exported(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    for name in NEW:
        assert name in native.EXPORTS and hasattr(native.load(), name), name
    assert native.load().rlt_abi_version() == 5
    assert "#define RLT_SPARSE_CHUNK 256" in header and native.SPARSE_CHUNK == 256
    from dataloader import bicut_data
    assert bicut_data.CHUNK == native.SPARSE_CHUNK


def test_argument_errors_before_any_launch(native):
    res = subprocess.run([sys.executable, "-c", ERRORS, REPO], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "errors ok" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def test_argument_errors_under_asan_ubsan():
    from rlt_hip import build
    rt = build.sanitizer_runtime()
    if rt is None:
        pytest.skip("clang's shared ASan runtime is not in this toolchain")
    lib = build.build_sanitized(verbose=False)
    env = dict(os.environ, LD_PRELOAD=rt, RLT_HIP_LIB=lib,
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=1:detect_odr_violation=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([sys.executable, "-c", ERRORS, REPO], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "errors ok" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]


# ------------------------------------------------------------------------------ BowTable
def _stats():
    return {"a": [10, 2, [(0, 3), (7, 7)]], "b": [0, 0, []], "c": [4, 1, [(3, 4)]], "unused": [1, 1, [(9, 1)]]}


def test_bowtable_packs_the_documents_of_the_lists():
    from dataloader.bicut_data import BowTable
    from dataloader.doc_features import docs_of
    raw = {"q1": {"c": 3.0, "a": 2.0}, "q2": {"a": 9.0, "b": 1.0}}
    t = BowTable(_stats(), docs_of(raw))
    assert t.n_docs == 3 and t.row == {"c": 0, "a": 1, "b": 2} and t.V == 10 and t.Dn == 3 and t.n_features == 13
    assert t.indptr.dtype == np.int64 and t.indices.dtype == np.int32 and t.values.dtype == np.float32
    assert t.indptr.tolist() == [0, 1, 3, 3] and t.indices.tolist() == [3, 0, 7] and t.values.tolist() == [4.0, 3.0, 7.0]
    assert t.scalars.tolist() == [[4.0, 1.0], [10.0, 2.0], [0.0, 0.0]]
    # the static term -> rows index: the table by term, one chunk per term
    assert t.col_ptr.tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3] and t.col_rows.tolist() == [1, 0, 1] and t.col_vals.tolist() == [3.0, 4.0, 7.0]
    assert t.chunk_ptr.tolist() == list(range(11)) and t.chunk_col.tolist() == list(range(10)) and t.n_multi == 0
    assert BowTable(_stats(), ["a"], vocab=231448).V == 231448
    assert t.rows_of(raw, ["q2", "q1"]).tolist() == [[1, 2], [0, 1]]


def test_term_index_cuts_long_columns_into_chunks():
    from dataloader.bicut_data import BowTable
    n = 600                                           # term 1 in every document: 600 entries = 3 chunks
    indptr = np.arange(n + 1, dtype=np.int64) * 2
    indices = np.tile(np.array([1, 4], np.int32), n)
    indices[1::2] = 2 + (np.arange(n) % 3)
    t = BowTable.from_csr(indptr, indices, np.ones(2 * n, np.float32), V=6)
    assert t.chunk_ptr.tolist() == [0, 1, 4, 5, 6, 7, 8] and t.chunk_col.tolist() == [0, 1, 1, 1, 2, 3, 4, 5]
    assert t.multi_cols.tolist() == [1] and t.n_chunks == 8 and t.n_multi == 1
    assert (np.diff(t.col_rows[t.col_ptr[1]:t.col_ptr[2]]) > 0).all()


def test_bowtable_errors_name_the_document():
    from dataloader.bicut_data import BowTable
    s = _stats()
    with pytest.raises(ValueError, match="'a'.*ascending"):
        BowTable({**s, "a": [10, 2, [(7, 7), (0, 3)]]}, ["c", "a"])
    with pytest.raises(ValueError, match="'a'.*ascending"):
        BowTable({**s, "a": [10, 2, [(3, 1), (3, 2)]]}, ["c", "a"])
    with pytest.raises(KeyError, match="'zz'.*bag-of-words"):
        BowTable(s, ["a", "zz"])
    with pytest.raises(ValueError, match="'a'.*int32"):
        BowTable({**s, "a": [10, 2, [(0, 3), (2 ** 31, 7)]]}, ["c", "a"])
    with pytest.raises(ValueError, match="'a'.*term id 7 outside the dictionary of 5"):
        BowTable(s, ["c", "a"], vocab=5)
    with pytest.raises(ValueError, match="'c'.*scalar statistics"):
        BowTable({**s, "c": [4, [(3, 4)]]}, ["a", "c"])
    with pytest.raises(ValueError):
        BowTable(s, [])
    t = BowTable(s, ["a", "b"])
    with pytest.raises(KeyError, match="'c'.*not in the table"):
        t.rows_of({"q": {"a": 1.0, "c": 0.5}}, ["q"])


# ------------------------------------------------------------------------------ model contract
def test_sparse_model_keeps_the_reference_state_dict():
    from models import BiCut
    from oracle import models as om
    I = 3 + 64
    torch.manual_seed(3)
    m = BiCut(input_size=I, dropout=0.0, sparse_input=True)
    torch.manual_seed(3)
    dense = BiCut(input_size=I, dropout=0.0)
    ref = om.BiCut(input_size=I, dropout=0.0)
    assert list(m.state_dict()) == list(ref.state_dict())
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in ref.state_dict().values()]
    for name in ("weight_ih_l0", "weight_ih_l0_reverse"):
        assert getattr(m.bilstm, name).stride() == (1, 512) and getattr(dense.bilstm, name).stride() == (I, 1)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), dense.state_dict().values()))      # same initial values
    ref.load_state_dict(m.state_dict())                                        # into the reference layout ...
    m2 = BiCut(input_size=I, dropout=0.0, sparse_input=True)
    m2.load_state_dict(ref.state_dict())                                       # ... and back
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert m2.bilstm.weight_ih_l0.stride() == (1, 512)


def test_flat_model_keeps_the_strides_of_a_column_major_parameter():
    from models import BiCut
    from rlt_hip.parallel import FlatModel
    m = BiCut(input_size=3 + 64, dropout=0.0, sparse_input=True)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    flat = FlatModel(m)
    for name in ("weight_ih_l0", "weight_ih_l0_reverse"):
        p = getattr(m.bilstm, name)
        assert p.stride() == (1, 512) and p.grad.stride() == (1, 512) and p.grad.shape == p.shape
        assert p.data_ptr() >= flat.flat_param.data_ptr() and p.data_ptr() % 16 == 0
    assert m.bilstm.weight_hh_l0.is_contiguous() and m.fc.weight.grad.is_contiguous()
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())
    # the slot holds the parameter in its OWN memory order: the column-major matrix = the transposed one, row by row
    p = m.bilstm.weight_ih_l0
    off = (p.data_ptr() - flat.flat_param.data_ptr()) // 4
    assert torch.equal(flat.flat_param[off:off + p.numel()], p.detach().t().reshape(-1))


def test_a_model_says_which_input_it_expected():
    from models import BiCut
    from rlt_hip import ops
    sparse, dense = BiCut(input_size=3 + 8, sparse_input=True), BiCut(input_size=3)
    with pytest.raises(TypeError, match="sparse_input=True.*SparseBatch.*dense tensor"):
        sparse(torch.zeros(2, 4, 11))
    batch = ops.SparseBatch(torch.zeros(2, 4, 3), torch.zeros((2, 4), dtype=torch.int32), table=None)
    with pytest.raises(TypeError, match="sparse_input=False.*dense.*SparseBatch"):
        dense(batch)
    with pytest.raises(ValueError, match="int32"):
        ops.SparseBatch(torch.zeros(2, 4, 3), torch.zeros((2, 4), dtype=torch.int64), table=None)
    with pytest.raises(ValueError, match="1..16"):
        ops.SparseBatch(torch.zeros(2, 4, 17), torch.zeros((2, 4), dtype=torch.int32), table=None)


def test_run_help_lists_the_new_flags():
    res = subprocess.run([sys.executable, os.path.join(REPO, "ranked-list-truncation_amd", "run.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "--bicut-stats" in res.stdout and "--bicut-vocab" in res.stdout


def test_loader_signatures():
    import inspect
    from dataloader import bicut_data, rank_data
    assert list(inspect.signature(bicut_data.bicut_dataloader).parameters)[:7] == [
        "retrieve_data", "dataset_name", "batch_size", "device", "base", "seed", "stats"]
    assert list(inspect.signature(rank_data.attncut_dataloader).parameters) == [
        "retrieve_data", "dataset_name", "batch_size", "device", "base", "seed", "doc_table"]
    assert list(inspect.signature(rank_data.choopy_dataloader).parameters) == [
        "retrieve_data", "dataset_name", "batch_size", "device", "base", "seed"]


def test_loader_yields_sparse_batches_on_the_host(tmp_path):
    import pickle
    from dataloader.bicut_data import bicut_dataloader
    from rlt_hip import ops
    base = tmp_path / "robust04"
    base.mkdir()
    docs = [f"d{i}" for i in range(12)]
    stats = {d: [i + 1, 1, [(i % 5, i + 1)]] for i, d in enumerate(docs)}
    lists = lambda qs: {q: {docs[(3 * q + j) % 12]: 5.0 - j for j in range(4)} for q in qs}
    for name, obj in (("bm25_train.pkl", lists(range(5))), ("bm25_test.pkl", lists(range(5, 7))),
                      ("gt.pkl", {q: [docs[(3 * q) % 12]] for q in range(7)})):
        pickle.dump(obj, open(base / name, "wb"))
    pickle.dump(stats, open(tmp_path / "bicut_stats.pkl", "wb"))
    train, test, data = bicut_dataloader("robust04", "bm25", 2, device=None, base=str(tmp_path), seed=1,
                                         stats=str(tmp_path / "bicut_stats.pkl"))
    assert data.n_features == 3 + 5 and data.lengths == [4] and len(train) == 3 and len(test) == 1
    seen = 0
    for batch, y in train:
        assert isinstance(batch, ops.SparseBatch) and batch.ids.dtype == torch.int32 and batch.dense.shape[2] == 3
        assert batch.shape == (batch.ids.shape[0], 4, 8) and batch[0:1].ids.shape == (1, 4)
        rows = batch.ids.numpy()
        assert rows.min() >= 0 and rows.max() < data.table.n_docs
        assert np.array_equal(batch.dense[..., 1:].numpy(), data.table.scalars[rows])          # the scalar statistics of those rows
        assert (y[:, 0] == 1).all() and (y[:, 1:] == 0).all()
        seen += len(rows)
    assert seen == 5


# ------------------------------------------------------------------------------ fixtures
def test_there_are_two_fixtures():
    assert [os.path.basename(f) for f in FIXTURES] == ["bicut_sparse_v2048_b6_s40.npz", "bicut_sparse_v231448_b2_s40.npz"]
    for f in FIXTURES:
        assert os.path.getsize(f) <= 320 * 1024


def test_fixtures_hold_the_cases_they_were_made_for():
    d = np.load(FIXTURES[0])
    V, ids, indptr, indices = int(d["V"]), d["ids"], d["indptr"], d["indices"]
    assert V == 2048 and ids.shape == (6, 40) and d["dense"].shape == (6, 40, 3)
    nnz = np.diff(indptr)
    docs_with = lambda t: {i for i in range(len(nnz)) if t in indices[indptr[i]:indptr[i + 1]]}
    empty = set(np.flatnonzero(nnz == 0))
    assert empty == {0} and 0 in ids                                                       # an empty row, ranked
    assert docs_with(0) == set(range(len(nnz))) - empty and len(docs_with(0)) > 256        # in every other document: two chunks
    assert docs_with(1) == {5} and 5 in ids and not docs_with(2)                           # in exactly one; in none
    assert docs_with(V - 1) & set(ids.reshape(-1).tolist())                                # the last term id, in the batch
    assert (ids[0] == 7).sum() == 2 and 7 in ids[1]                                        # twice in a list, and in two lists
    assert (ids[5] == ids[5, 0]).all()                                                     # one document throughout
    assert {0, 1, 2, V - 1} <= set(d["cols"].tolist()) and len(d["cols"]) <= 24
    for name in R.L0:
        assert d["gcolnorm/" + name].shape == (3 + V,) and d["gcolnorm/" + name][3 + 2] == 0.0
        assert d["gcol/" + name].shape == (512, 3 + len(d["cols"]))
    big = np.load(FIXTURES[1])
    assert int(big["V"]) == 231448 and big["ids"].shape == (2, 40) and 120 < np.diff(big["indptr"]).mean() < 180
    for dd in (d, big):
        for i in range(len(dd["indptr"]) - 1):
            assert (np.diff(dd["indices"][dd["indptr"][i]:dd["indptr"][i + 1]]) > 0).all()
        assert dd["values"].dtype == np.float32 and dd["indptr"].dtype == np.int64 and dd["ids"].dtype == np.int32


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_fixtures_agree_with_the_float64_restatement(path):
    d = dict(np.load(path))
    tag = os.path.basename(path)
    r = R.run(d, grad_crit=str(d["grad_crit"]))
    e_out = np.abs(r["out0"] - d["out0"]).max()
    e_loss = {m: abs(r["loss/" + m] - float(d["loss/" + m])) / abs(float(d["loss/" + m])) for m in ("nci", "f1")}
    print(f"{tag}: out0 {e_out:.2e}, loss nci {e_loss['nci']:.2e}, f1 {e_loss['f1']:.2e}")
    assert e_out <= 1e-6
    assert np.array_equal(r["k_s"], d["k_s"])
    assert e_loss["nci"] <= 1e-6 and e_loss["f1"] <= 1e-6
    Dn, cols = d["dense"].shape[2], d["cols"]
    worst_p = 0.0
    for name, g in r["grads"].items():
        norm = float(d["gnorm/" + name])
        flat_probe = g.reshape(-1)[torch.from_numpy(probe_index(g.numel(), name))].numpy()
        e = max(abs(float(g.norm()) - norm), np.abs(flat_probe - d["gprobe/" + name]).max()) / norm
        worst_p = max(worst_p, e)
        assert e <= 1e-5, (name, e)
        if name not in R.L0:
            continue
        take = np.concatenate([np.arange(Dn), Dn + cols])
        got, ref = g[:, take].numpy(), d["gcol/" + name].astype(np.float64)
        ref_norm = np.sqrt((ref ** 2).sum(0))
        e_col = 0.0
        for c in range(len(take)):
            if ref_norm[c] == 0.0:
                assert (got[:, c] == 0.0).all(), (name, take[c])                    # a term absent from the batch
            else:
                e_col = max(e_col, np.abs(got[:, c] - ref[:, c]).max() / ref_norm[c])
        colnorm = g.pow(2).sum(0).sqrt().numpy()
        assert abs(np.sqrt((colnorm ** 2).sum()) - float(d["gfro/" + name])) <= 1e-5 * float(d["gfro/" + name])
        assert int((colnorm != 0).sum()) == int(d["gnzcols/" + name])
        e_cn = 0.0
        if "gcolnorm/" + name in d:
            refn = d["gcolnorm/" + name]
            assert ((refn == 0) == (colnorm == 0)).all()
            nz = refn != 0
            e_cn = (np.abs(colnorm[nz] - refn[nz]) / refn[nz]).max()
            assert e_cn <= 1e-5, (name, e_cn)
        print(f"{tag} {name}: columns {e_col:.2e}, column norms {e_cn:.2e}")
        assert e_col <= 1e-5, (name, e_col)
    print(f"{tag}: parameters (norm, probes) {worst_p:.2e}")
