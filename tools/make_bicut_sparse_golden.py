#!/usr/bin/env python3
"""Generate tests/golden/bicut_sparse_*.npz by RUNNING THE REFERENCE's BiCut on its own DENSE bag-of-words input.

Only ever run where the reference is mounted (RLT_REFERENCE, default /root/reference).  As in tools/make_golden.py the
reference's `models.BiCut` and `utils.losses.BiCutLoss` are imported unmodified and nothing of the reference is written here:
the fixtures hold a generated table, the batch, and what the reference computed for them; weights are regenerated on every side
by oracle.weights.fill_state_dict.

The dense input is built as the reference builds it: per ranked document `[token count, distinct-token count] + the
bag-of-words vector densified over the V-term dictionary` (data_prep/document_statics.ipynb, "Bicut输入数据": `iv_dense`), then
`np.column_stack((scores, stats))` (dataloader/split_bicut_data.py:21-24), then `.float()` (dataloader/bicut_dataloader.py).

Two fixtures:
  bicut_sparse_v2048_b6_s40     V = 2048, 300 documents; by construction: a document with an empty row (row 0), a term in every
                                other document (term 0: 299 entries, so its column of the term index spans two chunks), a term
                                in exactly one document (term 1, row 5), a term in none (term 2), the last term id V-1, the same
                                document twice in one list and in two lists (row 7), a list whose documents are all one document
                                (list 5, row 9).  Records the float64 L2 norm of EVERY column of both layer-0 input-weight
                                gradients.
  bicut_sparse_v231448_b2_s40   the published width, 2 lists of 40, about 150 terms per document.
For the two layer-0 input weights (too large to store whole) each fixture records: all Dn dense columns and at most 24 chosen
term columns (`cols`), the float64 Frobenius norm and the number of non-zero columns.

Measured on the build machine (8 cores, 62 GB): v2048 1.7 s; v231448 11.7 s, peak resident memory 4.6 GB (the two 474 MB
weights, their gradients, the float64 draws of fill_state_dict and the (2, 40, 231451) dense input).

    python tools/make_bicut_sparse_golden.py
"""
import os
import resource
import sys
import time
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RLT_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle.weights import fill_state_dict, synthetic_lists  # noqa: E402
from golden_util import probe_index  # noqa: E402

CASES = [
    dict(tag="bicut_sparse_v2048_b6_s40", V=2048, n_docs=300, batch=6, seq_len=40, mean_terms=30, seed=191, edge=True),
    dict(tag="bicut_sparse_v231448_b2_s40", V=231448, n_docs=64, batch=2, seq_len=40, mean_terms=205, seed=192, edge=False),
]
L0 = ("bilstm.weight_ih_l0", "bilstm.weight_ih_l0_reverse")
GRAD_CRIT = "nci"


def make_table(case):
    """(indptr, indices, counts float32, ids (B,S) int32): term frequencies Zipf-like (rank^-1 over the dictionary), counts 1..5."""
    rs = np.random.RandomState(case["seed"])
    V, n_docs, B, S = case["V"], case["n_docs"], case["batch"], case["seq_len"]
    p = 1.0 / np.arange(1, V + 1)
    if case["edge"]:
        p[:3] = 0.0                                   # terms 0, 1, 2 are placed by hand
    p /= p.sum()
    rows = []
    for d in range(n_docs):
        n = max(1, int(rs.poisson(case["mean_terms"])))
        terms = set(rs.choice(V, size=n, replace=True, p=p).tolist())
        if case["edge"]:
            terms.add(0)
            if d == 5:
                terms.add(1)
            if d % 37 == 3:
                terms.add(V - 1)
            if d == 0:
                terms = set()
        rows.append(sorted(terms))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]).astype(np.int32)
    counts = rs.randint(1, 6, size=indices.size).astype(np.float32)
    ids = rs.randint(0, n_docs, size=(B, S)).astype(np.int32)
    if case["edge"]:
        ids[0, 3], ids[0, 4], ids[0, 17] = 0, 5, 3    # the empty row, the only document of term 1, a document with term V-1
        ids[0, 10] = ids[0, 22] = 7                   # twice in one list
        ids[1, 0] = 7                                 # and in another
        ids[5, :] = 9                                 # one document throughout
    return indptr, indices, counts, ids


def dense_input(indptr, indices, counts, ids, scores, V):
    """The reference's input: column_stack((scores, [token count, distinct count] + densified bag of words)) per list."""
    B, S = ids.shape
    x = np.zeros((B, S, 3 + V), dtype=np.float64)
    for b in range(B):
        stats = []
        for d in ids[b]:
            lo, hi = indptr[d], indptr[d + 1]
            vec = np.zeros(V)
            vec[indices[lo:hi]] = counts[lo:hi]
            stats.append(np.concatenate([[counts[lo:hi].sum(), hi - lo], vec]))
        x[b] = np.column_stack((scores[b], np.array(stats)))
    return torch.from_numpy(x).float()


def chosen_columns(case, indptr, indices, ids):
    V = case["V"]
    in_batch = np.unique(np.concatenate([indices[indptr[d]:indptr[d + 1]] for d in np.unique(ids)]))
    rs = np.random.RandomState(case["seed"] + 7)
    absent = np.setdiff1d(np.arange(V), in_batch)
    cols = [0, 1, 2, V - 1] if case["edge"] else []
    cols += rs.choice(in_batch, size=14, replace=False).tolist() + rs.choice(absent, size=4, replace=False).tolist()
    if case["edge"]:
        cols += indices[indptr[7]:indptr[7] + 1].tolist() + indices[indptr[9]:indptr[9] + 1].tolist()   # rows 7 and 9: repeated documents
    return np.unique(np.asarray(cols, dtype=np.int64))[:24]


def run(case, ref_models, ref_losses, RefMetric):
    t0 = time.time()
    V, B, S = case["V"], case["batch"], case["seq_len"]
    indptr, indices, counts, ids = make_table(case)
    x1, y = synthetic_lists(B, S, 1, case["seed"] + 1)
    scores = x1[..., 0].numpy()
    x = dense_input(indptr, indices, counts, ids, scores, V)
    dense = x[..., :3].numpy().copy()
    model = ref_models.BiCut(input_size=3 + V, dropout=0.0)
    fill_state_dict(model, case["seed"])
    rec = {"indptr": indptr, "indices": indices, "values": counts, "ids": ids, "dense": dense, "y": y.numpy(),
           "V": np.int64(V), "seed": np.int64(case["seed"])}
    model.train()
    out = model(x)
    rec["out0"] = out.detach().numpy()
    pred = np.argmax(out.detach().numpy(), axis=2)                      # run.py:131-136
    k_s = np.array([S if r.sum() == S else np.argmin(r) + 1 for r in pred], dtype=np.int64)
    rec["k_s"] = k_s
    rec["f1"] = np.float64(RefMetric.f1(y.numpy(), k_s))
    for metric in ("nci", "f1"):
        o = model(x)
        o.retain_grad()
        loss = ref_losses.BiCutLoss(metric=metric)(o, y)
        rec["loss/" + metric] = np.float64(loss.item())
        model.zero_grad()
        loss.backward()
        rec["dout/" + metric] = o.grad.numpy()
        if metric != GRAD_CRIT:
            continue
        cols = chosen_columns(case, indptr, indices, ids)
        rec["cols"] = cols
        for name, prm in model.named_parameters():
            g = prm.grad.detach()
            flat = g.reshape(-1)
            rec["gnorm/" + name] = np.float64(flat.double().norm().item())
            rec["gprobe/" + name] = flat[torch.from_numpy(probe_index(flat.numel(), name))].double().numpy()
            if name in L0:
                rec["gcol/" + name] = g[:, np.concatenate([np.arange(3), 3 + cols])].numpy()          # (512, 3 + len(cols)) float32
                colnorm = g.double().pow(2).sum(0).sqrt().numpy()
                rec["gfro/" + name] = np.float64(np.sqrt((colnorm ** 2).sum()))
                rec["gnzcols/" + name] = np.int64((colnorm != 0).sum())
                if case["edge"]:
                    rec["gcolnorm/" + name] = colnorm
    rec["grad_crit"] = np.array(GRAD_CRIT)
    path = os.path.join(OUT, case["tag"] + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{case['tag']}: k_s={k_s.tolist()} f1={rec['f1']:.6f} nci={float(rec['loss/nci']):.6f} f1loss={float(rec['loss/f1']):.6f} "
          f"nnz={indices.size} nonzero columns={int(rec['gnzcols/' + L0[0]])} | {os.path.getsize(path)} bytes, {time.time() - t0:.1f} s, "
          f"peak {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GB", flush=True)


def main():
    stub = types.ModuleType("numpy.lib.financial")
    stub.irr = None
    sys.modules["numpy.lib.financial"] = stub
    for m in [k for k in sys.modules if k == "utils" or k.startswith("utils.") or k == "models" or k.startswith("models.")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    import models as ref_models
    from utils import losses as ref_losses
    from utils.metrics import Metric as RefMetric
    sys.path.remove(REF)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    for case in CASES:
        if not only or case["tag"] in only:
            run(case, ref_models, ref_losses, RefMetric)


if __name__ == "__main__":
    main()
