"""The cut report on the MI355X (rlt_cut_report through ops.cut_report, utils/report.py and the models' truncate) against the
entry points it fuses (exact conditions), the float64 numpy restatement (tests/report_restate.py) and the reference's own
fp32 curves (tests/golden/report_*.npz, tools/make_report_golden.py).

Curves against the restatement: with identical inputs to exp (x = v / scale and the row maximum are formed by the same float64
operations on both sides) a term e_j / z differs by the two exp roundings (device and numpy, <= 1 ulp each, twice: term and
normaliser), the S-term sum of the normaliser in another order (S 2^-53 each side) and the division; the sum over B lists in
another order adds B 2^-53 on each side.  Relative to a curve value that is below (S + B + 8) 2^-52.

Curves against the reference's fp32 fixtures: the distance between the reference's result and the float64 restatement is
measured on the CPU in the test (it is the reference's own fp32 rounding) and the device is granted four times that
distance.  Measured distances (max abs over the curve, mean curves): prediction 2.9e-8 (edge_s40), 1.0e-8 (mq2007_s40),
3.1e-9 (losses_edge_s300), 7.1e-10 (robust04_s300); F1 reward 3.3e-9, 2.6e-9, 4.5e-10, 5.0e-10; DCG reward 1.3e-8, 1.0e-8,
3.0e-8, 9.0e-9."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import report_restate as R  # noqa: E402

FIXTURES = sorted(f for f in glob.glob(os.path.join(REPO, "tests", "golden", "report_*.npz")) if "bicut" not in f)
BICUT = os.path.join(REPO, "tests", "golden", "report_bicut_s40.npz")
TAU = 0.9
# the issue's sizes, and S = 700: the one reward layout they leave out (12 positions per lane for 11 rounds, with its zero fill)
SIZES = [(S, B) for S in (1, 7, 40, 64, 65, 300, 384, 385, 700, 1024) for B in (1, 5, 67, 1030)]
METRICS = ("f1", "dcg")


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _random_set(S, B, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0.0, 1.0, size=(B, S)).astype(np.float32)
    p = np.exp(logits - logits.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    if S > 2:                                   # a duplicated maximum in every third list: the first one wins, margin 0
        for b in range(0, B, 3):
            i, j = sorted(rng.choice(S, 2, replace=False))
            p[b, i] = p[b, j] = p[b].max() * np.float32(1.5)
    y = (rng.random((B, S)) < 0.15).astype(np.float32)
    y[0] = 0.0                                  # no relevant document
    if B > 1:
        y[1] = 1.0                              # only relevant documents
    p2 = rng.random((B, S, 2)).astype(np.float32)
    p2[0, :, 1] = p2[0, :, 0] + np.float32(0.5)   # no position prefers class 0: k = S
    if B > 2 and S > 1:
        p2[2, :, 1] = p2[2, :, 0] + np.float32(0.5)
        p2[2, S // 2, 1] = p2[2, S // 2, 0]     # a tie: class 0
    return p, y, p2


def _composition(p, y, metric, k_in=None, penalty=-1.0, mpenalty=-1.0):
    """What the fused pass must reproduce bit for bit, from the entry points it fuses."""
    from rlt_hip import native as N, ops
    pt, yt = (None if p is None else _t(p)), _t(y)
    if k_in is None:
        k, f1, dcg, sums = ops.cut_metrics(pt, yt, penalty=mpenalty)
    else:
        k, f1, dcg, sums = ops.cut_metrics(None, yt, k_in=k_in, penalty=mpenalty)
    _c, _s, best = ops.truncation_curves(yt, mpenalty, per_list=True)
    r = ops.reward_matrix(yt, N.METRIC_F1 if metric == "f1" else N.METRIC_DCG, penalty=penalty)
    torch.cuda.synchronize()
    return (k.cpu().numpy(), f1.cpu().numpy(), dcg.cpu().numpy(), sums.cpu().numpy(), [b.cpu().numpy() for b in best],
            r.cpu().numpy())


def _report(p, y, metric, acc=None, penalty=-1.0, mpenalty=-1.0):
    from rlt_hip import native as N, ops
    per, acc = ops.cut_report(_t(p), None if y is None else _t(y), N.METRIC_F1 if metric == "f1" else N.METRIC_DCG, penalty, mpenalty,
                              TAU, acc=acc)
    return per, acc


def _check_exact(per, acc, p, y, metric, k_in=None, penalty=-1.0, mpenalty=-1.0):
    B, S = y.shape
    k, f1, dcg, sums, best, r = _composition(p, y, metric, k_in, penalty, mpenalty)
    assert np.array_equal(per["k"], k)
    assert np.array_equal(per["f1"].view(np.int64), f1.view(np.int64))
    assert np.array_equal(per["dcg"].view(np.int64), dcg.view(np.int64))
    assert np.array_equal(acc["sums"][:2].view(np.int64), sums.view(np.int64))
    for name, ref in zip(("best_f1", "best_f1_k", "best_dcg", "best_dcg_k"), best):
        assert np.array_equal(per[name], ref) and per[name].dtype == ref.dtype, name
    assert np.array_equal(acc["hist"], np.bincount(k, minlength=S + 1).astype(np.float64))
    rk = r[np.arange(B), k - 1]
    assert np.array_equal(per["better"], (r > rk[:, None]).sum(1).astype(np.int32))
    assert acc["sums"][4] == B
    assert abs(acc["sums"][2] - best[0].sum()) <= 1e-12 * max(1.0, abs(best[0].sum()))
    assert abs(acc["sums"][3] - best[2].sum()) <= 1e-12 * max(1.0, abs(best[2].sum()))
    return r


def _check_curves(acc, p_col, r, S, B):
    bound = (S + B + 8) * 2.0 ** -52
    ref = R.pred_curve(p_col, TAU * 1e-3)
    print("pred curve rel err", np.abs(acc["pred_curve"] / np.where(ref > 0, ref, 1) - (ref > 0)).max(), "bound", bound)
    assert np.all(np.abs(acc["pred_curve"] - ref) <= bound * ref)
    ref = R.reward_curve(r, TAU)
    print("reward curve rel err", np.abs(acc["reward_curve"] / ref - 1).max(), "bound", bound)
    assert np.all(np.abs(acc["reward_curve"] - ref) <= bound * ref)


@pytest.mark.parametrize("S,B", SIZES, ids=[f"s{s}_b{b}" for s, b in SIZES])
def test_random_sets(S, B):
    p, y, p2 = _random_set(S, B, 1000 * S + B)
    labelled = {}
    for metric in METRICS:
        per, acc = map(_np, _report(p, y, metric))
        labelled[metric] = (per, acc)
        r = _check_exact(per, acc, p, y, metric)
        assert np.array_equal(per["k"], R.cut_argmax(p))
        assert np.array_equal(per["p_k"], p[np.arange(B), per["k"] - 1])
        assert np.array_equal(per["margin"], R.margin_argmax(p))
        _check_curves(acc, p, r, S, B)
        # two identical calls are bitwise equal
        per2, acc2 = map(_np, _report(p, y, metric))
        for name in per:
            assert np.array_equal(per[name], per2[name]), name
        for name in acc:
            assert np.array_equal(acc[name].view(np.int64), acc2[name].view(np.int64)), name
    # another penalty pair on the DCG side
    per, acc = map(_np, _report(p, y, "dcg", penalty=-0.5, mpenalty=-0.25))
    _check_exact(per, acc, p, y, "dcg", penalty=-0.5, mpenalty=-0.25)
    # label-free: the same k, p_k, margin, hist and prediction curve
    per0, acc0 = map(_np, _report(p, None, "f1"))
    per, acc = labelled["f1"]
    assert sorted(per0) == ["k", "margin", "p_k"]
    for name in per0:
        assert np.array_equal(per0[name], per[name]), name
    assert np.array_equal(acc0["hist"], acc["hist"])
    assert np.array_equal(acc0["pred_curve"].view(np.int64), acc["pred_curve"].view(np.int64))
    assert acc0["sums"][4] == B and not acc0["sums"][:4].any() and not acc0["reward_curve"].any()
    # accumulate over two halves against one call on the whole set
    if B > 1:
        h = B // 2
        _, a = _report(p[:h], y[:h], "dcg")
        _, a = _report(p[h:], y[h:], "dcg", acc=a)
        a = _np(a)
        whole = labelled["dcg"][1]
        assert np.array_equal(a["hist"], whole["hist"])
        for name in ("pred_curve", "reward_curve", "sums"):
            scale = np.maximum(np.abs(whole[name]), 1.0)
            assert np.all(np.abs(a[name] - whole[name]) <= 2.0 ** -52 * (B + 8) * scale), name
    # the PAIR rule: k as the torch rule of Metric.evaluate and as the reference's loop
    from utils.metrics import Metric
    k_torch, _f1, _dcg = Metric.evaluate(_t(p2), _t(y))
    per, acc = map(_np, _report(p2, y, "f1"))
    assert np.array_equal(per["k"], k_torch.cpu().numpy()) and np.array_equal(per["k"], R.cut_pair(p2))
    assert per["k"][0] == S
    r = _check_exact(per, acc, None, y, "f1", k_in=k_torch)
    assert np.array_equal(per["p_k"], p2[np.arange(B), per["k"] - 1, 0])
    assert np.array_equal(per["margin"], p2[np.arange(B), per["k"] - 1, 0] - p2[np.arange(B), per["k"] - 1, 1])
    _check_curves(acc, p2[:, :, 0], r, S, B)
    per0, acc0 = map(_np, _report(p2, None, "f1"))
    assert np.array_equal(per0["k"], per["k"]) and np.array_equal(acc0["hist"], acc["hist"])


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_reference_fixtures(path):
    from utils.report import CutReport
    d = np.load(path)
    y, p, tau = d["labels"].astype(np.float32), d["output"], float(d["tau"])
    B, S = y.shape
    for metric in METRICS:
        per, acc = map(_np, _report(p, y, metric))
        r = _check_exact(per, acc, p, y, metric)
        _check_curves(acc, p, r, S, B)
        rep = CutReport(S, metric=metric, tau=tau).update(_t(p)[:B // 2], y[:B // 2]).update(_t(p)[B // 2:].unsqueeze(2), y[B // 2:])
        reward, pred = rep.curves(tail_fix=True)
        ref64 = R.reward_curve(R.reward(y, metric), tau) / B
        dist = np.abs(ref64 - d[f"reward_{metric}"]).max()
        err = np.abs(reward - d[f"reward_{metric}"]).max()
        print(os.path.basename(path), metric, "reward: reference-restatement", dist, "device-reference", err)
        assert err <= 4 * dist
        ref64 = R.tail_fix(R.pred_curve(p, tau * 1e-3) / B)
        dist = np.abs(ref64 - d["pred"]).max()
        err = np.abs(pred - d["pred"]).max()
        print(os.path.basename(path), "prediction: reference-restatement", dist, "device-reference", err)
        assert err <= 4 * dist
        assert abs(reward.sum() - 1.0) < 1e-12 and abs(rep.curves(tail_fix=False)[1].sum() - 1.0) < 1e-12
        q, s = rep.per_query(), rep.summary()
        assert np.array_equal(q["k"], per["k"]) and np.array_equal(q["f1"], per["f1"])
        assert s["n"] == B and abs(s["f1"] - per["f1"].mean()) < 1e-12 and abs(s["regret_dcg"] - (per["best_dcg"] - per["dcg"]).mean()) < 1e-12
        assert s["best_cut_share_f1"] == np.mean(per["k"] == per["best_f1_k"]) and s["hist"] == acc["hist"].tolist()


def test_reference_bicut_fixture():
    d = np.load(BICUT)
    y, p2 = d["labels"].astype(np.float32), d["output2"]
    per, acc = map(_np, _report(p2, y, "dcg"))
    assert np.array_equal(per["k"], d["k"])
    _check_exact(per, acc, None, y, "dcg", k_in=_t(d["k"], np.int32))


def test_overflowing_reference_exponent_stays_finite():
    """p above 0.08: the reference's fp32 exp(p / 9e-4) is inf and its figure NaN; the device curve is the float64 softmax."""
    p = np.full((3, 40), 0.005, dtype=np.float32)
    p[:, 7] = 0.805
    y = np.zeros((3, 40), dtype=np.float32)
    y[:, :3] = 1
    per, acc = map(_np, _report(p, y, "f1"))
    assert np.isfinite(acc["pred_curve"]).all() and abs(acc["pred_curve"].sum() - 3.0) < 1e-12
    assert acc["pred_curve"][7] > 2.999 and per["k"].tolist() == [8, 8, 8]


def _check_truncate(model, xin, B, S):
    from rlt_hip import ops
    model = model.cuda().train()
    k, p_k = model.truncate(xin)
    assert model.training                                   # the state is restored
    model.eval()
    with torch.no_grad():
        out = model(xin)
    cut = out[-1] if isinstance(out, (list, tuple)) else out
    per, _ = ops.cut_report(cut)
    torch.cuda.synchronize()
    assert k.dtype == torch.int32 and p_k.dtype == torch.float32 and k.shape == (B,) and p_k.shape == (B,)
    assert torch.equal(k, per["k"]) and torch.equal(p_k, per["p_k"])
    ref = R.cut_pair(cut.cpu().numpy()) if cut.shape[-1] == 2 else R.cut_argmax(cut.reshape(B, S).cpu().numpy())
    assert np.array_equal(k.cpu().numpy(), ref)
    assert not any(p.grad is not None for p in model.parameters())


MODELS = ["AttnCut", "MtAttnCut", "BiCut", "Choopy", "MtChoopy", "MMOECut", "MOECut", "PLECut"]


@pytest.mark.parametrize("name", MODELS)
def test_truncate_on_every_model_class(name):
    import models
    torch.manual_seed(5)
    B, S = 6, 40
    x = torch.randn(B, S, 3, device="cuda")
    kw = {"AttnCut": dict(input_size=3), "MtAttnCut": dict(input_size=3, num_tasks=3), "BiCut": dict(input_size=3),
          "Choopy": dict(seq_len=S), "MtChoopy": dict(seq_len=S, num_tasks=3), "MMOECut": dict(seq_len=S, num_tasks=3, input_size=3),
          "MOECut": dict(seq_len=S, num_tasks=3, input_size=3), "PLECut": dict(seq_len=S, input_size=3)}[name]
    xin = x[:, :, :1].contiguous() if name in ("Choopy", "MtChoopy") else x
    _check_truncate(getattr(models, name)(**kw), xin, B, S)


def test_truncate_on_sparse_bicut():
    """BiCut on its bag-of-words input: truncate takes the ops.SparseBatch that forward takes."""
    from dataloader.bicut_data import BowTable
    from models import BiCut
    from rlt_hip import ops
    rs = np.random.RandomState(4)
    V, n_docs, B, S = 500, 90, 5, 40
    rows = [np.unique(rs.randint(0, V, size=rs.randint(0, 20))).astype(np.int32) for _ in range(n_docs)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows)
    table = BowTable.from_csr(indptr, indices, rs.randint(1, 4, size=indices.size).astype(np.float32), V)
    dense = torch.from_numpy(rs.standard_normal((B, S, 1)).astype(np.float32)).cuda()
    ids = torch.from_numpy(rs.randint(0, n_docs, size=(B, S)).astype(np.int32)).cuda()
    batch = ops.SparseBatch(dense, ids, table.to("cuda:0"), validate=True)
    torch.manual_seed(6)
    _check_truncate(BiCut(input_size=1 + V, sparse_input=True), batch, B, S)


def test_capturable_into_a_graph():
    from rlt_hip import native as N, ops
    p, y, _ = _random_set(300, 67, 3)
    pt, yt = _t(p), _t(y)
    ops.dcg_table(pt.device)
    ops.dcg_coef(300, pt.device)
    per, acc = ops.cut_report(pt, yt, N.METRIC_DCG)        # eager: warms the caches
    eager = _np({**per, **acc})
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            per, acc = ops.cut_report(pt, yt, N.METRIC_DCG)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    got = _np({**per, **acc})
    for name in eager:
        assert np.array_equal(eager[name], got[name]), name


E2E = [("attncut", (100, 200, 300)), ("choopy", None), ("mmoecut", None)]


@pytest.mark.parametrize("name,lengths", E2E, ids=[e[0] for e in E2E])
def test_run_report_end_to_end(tmp_path, name, lengths):
    """run.py trains one epoch and saves the checkpoint; a second run loads it (--epochs 0 --ft 1) and writes the report: one row
    per query id of the split, mean F1 / DCG equal to what Trainer.test computes for the same checkpoint with the same batch
    division (one batch per length bucket) to 1e-12, the same k without labels, --draw curves that sum to 1."""
    import json
    import run
    from dataloader.synth import write_synthetic_robust04
    base, save, tb = str(tmp_path / "data"), str(tmp_path / "ckpt"), str(tmp_path / "tb")
    kw = dict(lengths=lengths) if lengths else dict(seq_len=300)
    n_test = 126 if lengths else 44                          # more than 40 lists in every length bucket: each one draws
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=48, n_test=n_test, seed=11, **kw)
    common = ["--model-name", name, "--dataset-base", base, "--use-conf", "0", "--batch-size", "64", "--seed", "3", "--dropout", "0.1",
              "--save-path", save, "--criterion", "f1"]
    run.main(common + ["--epochs", "1", "--model-persist", "1", "--tensorboard-dir", tb, "--draw", "1"])
    ckpt = os.path.join(save, f"{name}.pkl")
    assert os.path.exists(ckpt)
    lines = [json.loads(l) for l in open(os.path.join(tb, "scalars.jsonl"))]
    drawn = [l for l in lines if l["tag"] in ("draw/reward", "draw/prediction")]
    for tag in ("draw/reward", "draw/prediction"):          # one batch per length bucket, each of more than 40 lists
        assert sorted(len(l["values"]) for l in drawn if l["tag"] == tag) == sorted(lengths or (300,))
    for l in drawn:
        assert abs(sum(l["values"]) - 1.0) < 1e-12
    out, out0 = str(tmp_path / "report.npz"), str(tmp_path / "report0.npz")
    argv = common + ["--epochs", "0", "--ft", "1", "--model-path", ckpt, "--tensorboard-dir", ""]
    run.main(argv + ["--report-out", out])
    gt = os.path.join(base, "robust04", "gt.pkl")           # the label-free report needs no ground truth
    os.rename(gt, gt + ".away")
    try:
        run.main(argv + ["--report-out", out0, "--report-labels", "0"])
    finally:
        os.rename(gt + ".away", gt)
    d, d0 = np.load(out), np.load(out0)
    trainer = run.Trainer(run.build_parser().parse_args(argv))
    qids = [str(q) for _L, (_x, _y, q) in sorted(trainer.data.buckets["test"].items()) for q in q]
    assert d["qid"].tolist() == qids and len(set(qids)) == n_test
    for key in ("k", "p_k", "margin", "f1", "dcg", "best_f1", "best_f1_k", "best_dcg", "best_dcg_k", "better", "length"):
        assert d[key].shape == (n_test,), key
    assert np.array_equal(d0["k"], d["k"]) and "f1" not in d0.files
    _loss, f1, dcg = trainer.test(0)
    summ = json.loads(str(d["summary"]))
    assert abs(np.mean([summ[str(L)]["f1"] for L in d["lengths"]]) - f1) < 1e-12
    assert abs(np.mean([summ[str(L)]["dcg"] for L in d["lengths"]]) - dcg) < 1e-12
    for L in d["lengths"]:
        assert d[f"hist_{L}"].sum() == (d["length"] == L).sum()
        assert abs(d[f"reward_curve_{L}"].sum() - 1.0) < 1e-12 and d[f"pred_curve_{L}"].shape == (L,)


def test_run_report_sparse_bicut(tmp_path):
    """--report-out with --bicut-stats: the sparse loader's length buckets go through the same report, PAIR rule."""
    import json
    import pickle
    import run
    from dataloader.synth import write_synthetic_robust04
    base = str(tmp_path)
    write_synthetic_robust04(base, "robust04", "bm25", n_train=12, n_test=9, lengths=(40, 100), seed=2)
    raws = [pickle.load(open(tmp_path / "robust04" / f"bm25_{s}.pkl", "rb")) for s in ("train", "test")]
    rs = np.random.RandomState(3)
    V = 300
    stats = {}
    for raw in raws:
        for docs in raw.values():
            for doc in docs:
                terms = np.unique(rs.randint(0, V, size=12))
                counts = rs.randint(1, 4, size=terms.size)
                stats[doc] = [int(counts.sum()), int(terms.size), [(int(t), int(c)) for t, c in zip(terms, counts)]]
    pickle.dump(stats, open(tmp_path / "bicut_stats.pkl", "wb"))
    out = str(tmp_path / "report.npz")
    run.main(["--model-name", "bicut", "--dataset-name", "bm25", "--dataset-base", base, "--use-conf", "0", "--batch-size", "4",
              "--seed", "1", "--epochs", "1", "--save-path", str(tmp_path / "ckpt"), "--tensorboard-dir", "",
              "--bicut-stats", str(tmp_path / "bicut_stats.pkl"), "--bicut-vocab", str(V), "--report-out", out])
    d = np.load(out)
    assert d["k"].shape == (9,) and sorted(d["lengths"].tolist()) == [40, 100]
    assert np.all((d["k"] >= 1) & (d["k"] <= d["length"]))
    summ = json.loads(str(d["summary"]))
    assert sum(s["n"] for s in summ.values()) == 9
    assert abs(np.mean(d["f1"][d["length"] == 40]) - summ["40"]["f1"]) < 1e-12
