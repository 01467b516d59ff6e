"""BiCut on its sparse bag-of-words input on the device: models.BiCut(sparse_input=True) + BiCutLoss against the reference
fixtures (tools/make_bicut_sparse_golden.py), against the project's own dense path on the densified input, bitwise
reproducibility, five optimizer steps sparse against dense, and run.py --bicut-stats end to end.

Tolerances are those the existing BiCut cases are held to (tools/gpu_probe.py, section bicut): out 1e-5 absolute, k_s identical,
F1 1e-4, loss 1e-5 relative, dout 1e-6 relative to its maximum, parameter gradients (norm and probes, relative to the golden
norm floored at 1e-3) 1e-3; the sampled layer-0 columns (relative to the column's norm) and the matrix norms under that same
1e-3; columns of absent terms exactly 0.0; the number of non-zero columns equal.  The five-step trajectories: loss and F1
within 1e-4, cut positions identical (tools/gpu_probe.py, section trajectory).

Measured on an MI355X: fixtures - out 6.0e-8, losses at most 1.1e-7, dout at most 9.3e-8, parameter gradients at most 1.3e-7,
sampled layer-0 columns at most 3.6e-7 of the column norm (both fixtures); sparse against dense at 20 x 300 - out 1.0 x 2^-24,
equal losses, every gradient within 4.8e-8 of its norm; the five-step trajectories agree to the printed six decimals.  The file
takes 9 s of the GPU suite."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ranked-list-truncation_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
L0 = ("bilstm.weight_ih_l0", "bilstm.weight_ih_l0_reverse")


def _model(I, seed, sparse):
    from models import BiCut
    from oracle.weights import fill_state_dict
    m = BiCut(input_size=I, dropout=0.0, sparse_input=sparse)
    fill_state_dict(m, seed)
    return m.to(DEV)


def _batch(table, dense, ids):
    from rlt_hip import ops
    return ops.SparseBatch(torch.from_numpy(np.ascontiguousarray(dense, dtype=np.float32)).to(DEV),
                           torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(DEV), table.to(DEV), validate=True)


def _generated(V, n_docs, B, S, mean_terms, seed):
    """A table with Zipf-like term frequencies (rank^-1), `mean_terms` draws per document, counts 1..5, and a batch over it."""
    from dataloader.bicut_data import BowTable
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, V + 1)
    p /= p.sum()
    rows = [np.unique(rs.choice(V, size=max(1, rs.poisson(mean_terms)), p=p)).astype(np.int32) for _ in range(n_docs)]
    rows[1] = np.zeros(0, np.int32)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows)
    table = BowTable.from_csr(indptr, indices, rs.randint(1, 6, size=indices.size).astype(np.float32), V)
    ids = rs.randint(0, n_docs, size=(B, S)).astype(np.int32)
    dense = np.stack([np.sort(rs.standard_normal((B, S)) * 2.5 + 3.0, axis=1)[:, ::-1],
                      rs.uniform(0, 4, (B, S)), rs.uniform(0, 2, (B, S))], axis=2).astype(np.float32)
    y = (rs.uniform(0, 1, (B, S)) < 0.55 * np.exp(-np.arange(S) / 45.0) + 0.02).astype(np.float32)
    y[:, 0] = np.maximum(y[:, 0], (y.sum(1) == 0))
    return table, dense, ids, torch.from_numpy(y).to(DEV)


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _grad_err(got, ref):
    """max |got - ref| relative to the reference matrix norm floored at 1e-3 (the measure of tools/gpu_probe.py:_grad_err)."""
    scale = max(float(ref.double().norm()), 1e-3)
    return float((got.double() - ref.double()).abs().max()) / scale


@pytest.mark.parametrize("tag", ["bicut_sparse_v2048_b6_s40", "bicut_sparse_v231448_b2_s40"])
def test_fixtures_through_the_sparse_model(tag):
    from dataloader.bicut_data import BowTable
    from utils import losses as hl
    from utils.metrics import Metric
    d = gu.load(tag)
    V, Dn = int(d["V"]), d["dense"].shape[2]
    table = BowTable.from_csr(d["indptr"], d["indices"], d["values"], V)
    model = _model(Dn + V, int(d["seed"]), True)
    batch = _batch(table, d["dense"], d["ids"])
    y = torch.from_numpy(d["y"]).to(DEV)
    model.train()
    out = model(batch)
    e = float(np.abs(out.detach().cpu().numpy() - d["out0"]).max())
    print(f"{tag}: out {e:.2e}")
    assert e <= 1e-5
    k, f1, _ = Metric.evaluate(out, y)
    assert np.array_equal(k.cpu().numpy(), d["k_s"]) and abs(float(f1) - float(d["f1"])) <= 1e-4
    for metric in ("nci", "f1"):
        o = model(batch)
        o.retain_grad()
        loss = hl.BiCutLoss(metric=metric)(o, y)
        model.zero_grad()
        loss.backward()
        refl = float(d["loss/" + metric])
        e_l = abs(loss.item() - refl) / max(1.0, abs(refl))
        e_d = float(np.abs(o.grad.cpu().numpy() - d["dout/" + metric]).max() / max(1e-30, np.abs(d["dout/" + metric]).max()))
        print(f"{tag}: loss {metric} {e_l:.2e}, dout {e_d:.2e}")
        assert e_l <= 1e-5 and e_d <= 1e-6
        if metric != str(d["grad_crit"]):
            continue
        cols = d["cols"]
        for name, prm in model.named_parameters():
            g = prm.grad.detach()
            scale = max(float(d["gnorm/" + name]), 1e-3)
            idx = gu.probe_index(g.numel(), name)
            probes = g[torch.from_numpy(idx // g.shape[-1]).to(DEV), torch.from_numpy(idx % g.shape[-1]).to(DEV)] if g.dim() == 2 \
                else g[torch.from_numpy(idx).to(DEV)]
            norm = float(g.double().pow(2).sum().sqrt())
            e_g = max(abs(norm - float(d["gnorm/" + name])), float(np.abs(probes.double().cpu().numpy() - d["gprobe/" + name]).max())) / scale
            assert e_g <= 1e-3, (name, e_g)
            if name not in L0:
                continue
            assert g.stride() == (1, 512)
            take = torch.from_numpy(np.concatenate([np.arange(Dn), Dn + cols])).to(DEV)
            got, ref = g[:, take].double().cpu().numpy(), d["gcol/" + name].astype(np.float64)
            ref_norm = np.sqrt((ref ** 2).sum(0))
            e_c = 0.0
            for c in range(ref.shape[1]):
                if ref_norm[c] == 0.0:
                    assert (got[:, c] == 0.0).all(), (name, c)
                else:
                    e_c = max(e_c, np.abs(got[:, c] - ref[:, c]).max() / max(ref_norm[c], 1e-3))
            colnorm = g.double().pow(2).sum(0).sqrt().cpu().numpy()
            e_f = abs(np.sqrt((colnorm ** 2).sum()) - float(d["gfro/" + name])) / max(float(d["gfro/" + name]), 1e-3)
            print(f"{tag} {name}: parameter {e_g:.2e}, columns {e_c:.2e}, Frobenius {e_f:.2e}")
            assert e_c <= 1e-3 and e_f <= 1e-3
            assert int((colnorm != 0).sum()) == int(d["gnzcols/" + name])
            if "gcolnorm/" + name in d:
                refn = d["gcolnorm/" + name]
                assert ((refn == 0) == (colnorm == 0)).all()                           # absent terms: exactly 0.0
                assert (np.abs(colnorm - refn) / np.maximum(refn, 1e-3)).max() <= 1e-3


def _pair(V=2048, n_docs=4000, B=20, S=300, mean_terms=40, seed=5):
    table, dense, ids, y = _generated(V, n_docs, B, S, mean_terms, seed)
    sparse = _model(3 + V, 77, True)
    dense_m = _model(3 + V, 77, False)
    batch = _batch(table, dense, ids)
    return sparse, dense_m, batch, batch.to_dense(), y


def test_sparse_against_the_dense_path_at_20_x_300():
    from rlt_hip import ops
    from utils import losses as hl
    sparse, dense_m, batch, x, y = _pair()
    crit = hl.BiCutLoss(metric="nci")
    res = []
    with ops.precision("fp32"):
        for m, inp in ((sparse, batch), (dense_m, x)):
            m.train()
            o = m(inp)
            o.retain_grad()
            loss = crit(o, y)
            m.zero_grad()
            loss.backward()
            res.append((o.detach(), float(loss.detach()), o.grad.detach(), _grads(m)))
    (o_s, l_s, d_s, g_s), (o_d, l_d, d_d, g_d) = res
    e_o = float((o_s - o_d).abs().max())
    print(f"sparse vs dense 20 x 300, V = 2048: out {e_o:.2e} ({e_o / U:.1f} u), loss {abs(l_s - l_d) / max(1.0, abs(l_d)):.2e}")
    assert e_o <= 1e-5 and abs(l_s - l_d) / max(1.0, abs(l_d)) <= 1e-5
    assert float((d_s - d_d).abs().max()) / float(d_d.abs().max()) <= 1e-6
    for name in g_d:
        e = _grad_err(g_s[name], g_d[name])
        print(f"  {name}: {e:.2e} of the norm, max abs {float((g_s[name] - g_d[name]).abs().max()) / U:.1f} u")
        assert e <= 1e-3, (name, e)
    assert ((g_s[L0[0]] == 0).all(0) == (g_d[L0[0]] == 0).all(0)).all()


def test_two_passes_are_bitwise_equal_and_lists_permute():
    from utils import losses as hl
    table, dense, ids, y = _generated(2048, 500, 6, 40, 40, 9)
    ids[2, :] = ids[2, 0]
    ids[3, 5] = ids[3, 9] = ids[0, 0]
    model = _model(3 + 2048, 31, True)
    model.train()
    crit = hl.BiCutLoss(metric="f1")

    def run(order):
        batch = _batch(table, dense[order], ids[order])
        o = model(batch)
        loss = crit(o, y[torch.from_numpy(order).to(DEV)])
        model.zero_grad()
        loss.backward()
        return o.detach().clone(), _grads(model)

    same = np.arange(6)
    o1, g1 = run(same)
    o2, g2 = run(same)
    assert torch.equal(o1, o2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    perm = np.array([4, 2, 0, 5, 1, 3])
    o3, g3 = run(perm)
    # (lists are independent in BiCut: each list's output depends on that list alone)
    assert torch.equal(o3, o1[torch.from_numpy(perm).to(DEV)])
    for n in g1:
        assert _grad_err(g3[n], g1[n]) <= 1e-3, n


def test_five_adam_steps_sparse_against_dense():
    from rlt_hip import ops
    from rlt_hip.parallel import FlatModel, FusedAdam
    from utils import losses as hl
    from utils.metrics import Metric
    sparse, dense_m, batch, x, y = _pair(V=2048, n_docs=800, B=6, S=40, mean_terms=40, seed=13)
    crit = hl.BiCutLoss(metric="nci")
    traj = []
    with ops.precision("fp32"):
        for m, inp in ((sparse, batch), (dense_m, x)):
            opt = FusedAdam(FlatModel(m), lr=1e-3, weight_decay=0.005)
            m.train()
            steps = []
            for _ in range(5):
                opt.zero_grad()
                o = m(inp)
                loss = crit(o, y)
                loss.backward()
                opt.step()
                k, f1, _ = Metric.evaluate(o.detach(), y)
                steps.append((float(loss.detach()), float(f1), k.cpu().numpy()))
            traj.append(steps)
    assert sparse.bilstm.weight_ih_l0.stride() == (1, 512)
    for i, ((l_s, f_s, k_s), (l_d, f_d, k_d)) in enumerate(zip(*traj)):
        print(f"step {i}: loss {l_s:.6f} / {l_d:.6f}, f1 {f_s:.6f} / {f_d:.6f}")
        assert abs(l_s - l_d) <= 1e-4 * max(1.0, abs(l_d)) and abs(f_s - f_d) <= 1e-4 and np.array_equal(k_s, k_d)
    assert traj[0][0][0] != traj[0][4][0]                      # the weights moved


def test_run_py_trains_on_a_statistics_file(tmp_path):
    from dataloader import write_synthetic_robust04
    write_synthetic_robust04(str(tmp_path), "robust04", "bm25", n_train=12, n_test=6, seq_len=40)
    raws = [pickle.load(open(tmp_path / "robust04" / f"bm25_{s}.pkl", "rb")) for s in ("train", "test")]
    rs = np.random.RandomState(3)
    V = 3000
    stats = {}
    for raw in raws:
        for docs in raw.values():
            for doc in docs:
                terms = np.unique(rs.randint(0, V, size=30))
                counts = rs.randint(1, 4, size=terms.size)
                stats[doc] = [int(counts.sum()), int(terms.size), [(int(t), int(c)) for t, c in zip(terms, counts)]]
    pickle.dump(stats, open(tmp_path / "bicut_stats.pkl", "wb"))
    save = tmp_path / "ckpt"
    cmd = [sys.executable, os.path.join(PKG, "run.py"), "--model-name", "bicut", "--retrieve-data", "robust04", "--dataset-name", "bm25",
           "--dataset-base", str(tmp_path), "--use-conf", "0", "--epochs", "1", "--batch-size", "4", "--seed", "1", "--model-persist", "1",
           "--save-path", str(save), "--tensorboard-dir", "", "--baselines", "1"]
    res = subprocess.run(cmd + ["--bicut-stats", str(tmp_path / "bicut_stats.pkl"), "--bicut-vocab", str(V)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    from oracle import models as om
    ref = om.BiCut(input_size=3 + V, dropout=0.0)
    ref.load_state_dict(torch.load(save / "bicut.pkl", map_location="cpu"))
    assert ref.bilstm.weight_ih_l0.shape == (512, 3 + V) and ref.bilstm.weight_ih_l0.is_contiguous()
    # without the flag: the three attncut columns, as before
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    ref3 = om.BiCut(input_size=3, dropout=0.0)
    ref3.load_state_dict(torch.load(save / "bicut.pkl", map_location="cpu"))
