"""Truncation baselines on the MI355X (rlt_truncation_curves through utils/baselines.py and run.py --baselines) against the
reference notebooks' own results (tests/golden/baselines_*.npz, tools/make_baseline_golden.py) and an independent numpy
restatement (tests/baseline_restate.py).

Best-k rules: the per-list best F1 k is np.argmax of the reference values exactly (F1 comes from integer counts in cal_F1's
operation order: ties are bit-identical on both sides); a best DCG k may be any k whose reference value is within 1e-12 of
the list's maximum (the device adds the DCG prefix in another order)."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_restate as R  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "baselines_*.npz")))
TOL = 1e-12


def _dev():
    return torch.device("cuda")


def _per_list(y, penalty=-1.0):
    from rlt_hip import ops
    t = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32)).to(_dev())
    curves, sums, best = ops.truncation_curves(t, penalty, per_list=True)
    torch.cuda.synchronize()
    return curves.cpu().numpy(), sums.cpu().numpy(), [b.cpu().numpy() for b in best]


def _check_best(ref_f1, ref_dcg, best, what):
    bf, bfk, bd, bdk = best
    n = ref_f1.shape[0]
    assert np.abs(bf - ref_f1.max(1)).max() < TOL, what
    assert np.abs(bd - ref_dcg.max(1)).max() < TOL, what
    assert np.array_equal(bfk, ref_f1.argmax(1)), (what, np.flatnonzero(bfk != ref_f1.argmax(1))[:5])
    at = ref_dcg[np.arange(n), bdk]
    assert np.all(at >= ref_dcg.max(1) - TOL), what
    assert np.all((bdk >= 0) & (bdk <= ref_f1.shape[1] - 1)), what


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_against_the_notebook_fixtures(path):
    from utils import baselines as bl
    d = np.load(path)
    y_tr, y_te = d["train_labels"], d["test_labels"]
    # per-list bests and the raw curves against the notebook's per-k values
    for split, y in (("train", y_tr), ("test", y_te)):
        curves, sums, best = _per_list(y)
        f1, dcg = d[f"{split}_per_k_f1"], d[f"{split}_per_k_dcg"]
        _check_best(f1, dcg, best, f"{os.path.basename(path)} {split}")
        n = y.shape[0]
        assert np.abs(curves[0] / n - d[f"{split}_curve_f1"]).max() < TOL
        assert np.abs(curves[1] / n - d[f"{split}_curve_dcg"]).max() < TOL
        assert sums[2] == n
    tc = bl.TruncationCurves(y_te.shape[1]).update(y_te)
    assert tc.n_lists == y_te.shape[0]
    f1, dcg = tc.best_cut()
    assert abs(f1 - d["best_f1"]) < TOL and abs(dcg - d["best_dcg"]) < TOL
    for i, k in enumerate(d["fixed_k"]):
        f1, dcg = bl.fixed_k(y_te, int(k))
        assert abs(f1 - d["fixed_f1"][i]) < TOL and abs(dcg - d["fixed_dcg"][i]) < TOL
        assert tc.fixed_k([int(k), int(k)]) == (f1, dcg)
    assert np.abs(tc.f1_curve().cpu().numpy() - d["test_curve_f1"]).max() < TOL
    assert np.abs(tc.dcg_curve().cpu().numpy() - d["test_curve_dcg"]).max() < TOL
    # greedy k: equal to the notebook's, or a near-tie of its curve
    g_f1, g_dcg, kf, kd = bl.greedy_k(y_tr, y_te)
    for k, ref_k, curve in ((kf, int(d["greedy_k_f1"]), d["train_curve_f1"]), (kd, int(d["greedy_k_dcg"]), d["train_curve_dcg"])):
        assert k == ref_k or abs(curve[k] - curve[ref_k]) < TOL, (k, ref_k)
    if kf == int(d["greedy_k_f1"]):
        assert abs(g_f1 - d["greedy_f1"]) < TOL
    if kd == int(d["greedy_k_dcg"]):
        assert abs(g_dcg - d["greedy_dcg"]) < TOL
    if y_tr.shape[0] == 1:                 # the edge set's one-list train split: an exact F1 tie, the first maximum exactly
        assert kf == int(d["greedy_k_f1"]) == 1
    # countp over train + test
    both = bl.TruncationCurves(y_te.shape[1]).update(y_tr).update(y_te)
    n = min(y_te.shape[1], len(d["countp"]))
    assert np.abs(both.irrelevant_share().cpu().numpy()[:n] - d["countp"][:n]).max() < TOL


@pytest.mark.parametrize("S", [1, 40, 63, 64, 65, 300, 1024])
def test_random_sets_against_the_restatement(S):
    rs = np.random.RandomState(S)
    for B in (1, 3, 65, 4097):
        for penalty in (-1.0, 0.0, -0.5):
            dens = rs.choice([0.02, 0.1, 0.5])
            y = (rs.uniform(size=(B, S)) < dens).astype(np.float32)
            y[rs.uniform(size=B) < 0.05] = 0                       # some lists without a relevant document
            curves, sums, best = _per_list(y, penalty)
            ref_sums, ref_best_sums, _ = R.curves(y, penalty)
            f1, dcg = R.per_k(y, penalty)
            what = f"S={S} B={B} penalty={penalty}"
            assert np.abs(curves - ref_sums).max() / B < TOL, what          # the mean curves
            assert np.abs(sums[:2] - ref_best_sums).max() / B < TOL, what
            assert sums[2] == B
            _check_best(f1, dcg, best, what)


def test_one_large_set():
    from rlt_hip import ops
    B, S = 262144, 300
    g = torch.Generator(device="cpu").manual_seed(5)
    prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32) / 45.0) + 0.02
    y = (torch.rand(B, S, generator=g) < prob).float()
    curves, sums, best = ops.truncation_curves(y.to(_dev()), -1.0, per_list=True)
    curves, sums = curves.cpu().numpy(), sums.cpu().numpy()
    bf, bfk, bd, bdk = [b.cpu().numpy() for b in best]
    ref_sums, ref_best_sums, ref_best = R.curves(y.numpy(), -1.0)
    rel = np.abs(curves - ref_sums).max() / np.abs(ref_sums).max()
    assert rel < TOL, rel
    assert np.abs(sums[:2] - ref_best_sums).max() / np.abs(ref_best_sums).max() < TOL
    assert np.abs(bf - ref_best[0]).max() < TOL and np.abs(bd - ref_best[2]).max() < TOL
    assert np.array_equal(bfk, ref_best[1])
    # a DCG k that differs from numpy's argmax must be a near-tie: recompute those lists
    diff = np.flatnonzero(bdk != ref_best[3])
    if len(diff):
        _, dcg = R.per_k(y.numpy()[diff])
        assert np.all(dcg[np.arange(len(diff)), bdk[diff]] >= dcg.max(1) - TOL)


def test_streaming_and_determinism():
    from utils.baselines import TruncationCurves
    rs = np.random.RandomState(3)
    a = (rs.uniform(size=(1000, 300)) < 0.1).astype(np.float32)
    b = (rs.uniform(size=(777, 300)) < 0.1).astype(np.float32)
    s1 = TruncationCurves(300).update(a).update(b)
    s2 = TruncationCurves(300).update(np.concatenate([a, b]))
    assert s1.n_lists == s2.n_lists == 1777
    c1, c2 = s1.curves.cpu().numpy(), s2.curves.cpu().numpy()
    assert np.all(np.abs(c1 - c2) <= TOL * np.maximum(np.abs(c2), 1e-300))
    assert np.all(np.abs(s1.sums.cpu().numpy() - s2.sums.cpu().numpy()) <= TOL * np.abs(s2.sums.cpu().numpy()))
    # the same call twice: bitwise equal
    r1, r2 = _per_list(a), _per_list(a)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    assert all(np.array_equal(x, z) for x, z in zip(r1[2], r2[2]))
    assert TruncationCurves(300).update(np.zeros((0, 300), np.float32)).n_lists == 0


def _expected(y_tr, y_te, ks):
    f1, dcg = R.per_k(y_te)
    tr_f1, tr_dcg = R.per_k(y_tr)
    kf, kd = int(np.argmax(tr_f1.mean(0))), int(np.argmax(tr_dcg.mean(0)))
    return {"Oracle": (f1.max(1).mean(), dcg.max(1).mean()),
            "fixed": {k: (f1[:, k].mean(), dcg[:, k].mean()) for k in ks},
            "greedy": (kf, kd, f1[:, kf].mean(), dcg[:, kd].mean()), "curves": (tr_f1.mean(0), tr_dcg.mean(0))}


def _check_history(rec, y_tr, y_te, ks):
    from utils import baselines as bl
    e = _expected(y_tr, y_te, ks)
    assert rec["n_test"] == y_te.shape[0] and rec["n_train"] == y_tr.shape[0]
    assert abs(rec["Oracle"]["f1"] - e["Oracle"][0]) < TOL and abs(rec["Oracle"]["dcg"] - e["Oracle"][1]) < TOL
    assert (rec["Oracle"]["f1"], rec["Oracle"]["dcg"]) == bl.best_cut(y_te)
    for k in ks:
        got = rec["fixed_k"][str(k)]
        assert abs(got["f1"] - e["fixed"][k][0]) < TOL and abs(got["dcg"] - e["fixed"][k][1]) < TOL
    g = rec["greedy_k"]
    assert (g["f1"], g["dcg"], g["k_f1"], g["k_dcg"]) == bl.greedy_k(y_tr, y_te)
    kf, kd, f1, dcg = e["greedy"]
    cf, cd = e["curves"]
    assert g["k_f1"] == kf or abs(cf[g["k_f1"]] - cf[kf]) < TOL
    assert g["k_dcg"] == kd or abs(cd[g["k_dcg"]] - cd[kd]) < TOL
    if (g["k_f1"], g["k_dcg"]) == (kf, kd):
        assert abs(g["f1"] - f1) < TOL and abs(g["dcg"] - dcg) < TOL


@pytest.mark.parametrize("lengths", [None, (100, 200, 300)], ids=["robust04", "buckets"])
def test_run_py_epochs_0_baselines(tmp_path, lengths):
    import run as hip_run
    from dataloader import RankData, write_synthetic_robust04
    write_synthetic_robust04(str(tmp_path), "robust04", "drmm_tks", n_train=60, n_test=30, seed=9, lengths=lengths)
    hist = tmp_path / "hist.json"
    tb = tmp_path / "tb"
    hip_run.main(["--model-name", "attncut", "--dataset-base", str(tmp_path), "--epochs", "0", "--use-conf", "0",
                  "--baselines", "1", "--history-json", str(hist), "--tensorboard-dir", str(tb), "--seed", "1"])
    out = json.loads(hist.read_text())
    assert out["history"] == [] and out["best_f1"] is None
    rd = RankData("robust04", "drmm_tks", True, str(tmp_path))
    ks = (5, 10, 30)
    assert sorted(out["baselines"]) == sorted(str(L) for L in rd.test_lengths)
    for L in rd.test_lengths:
        _check_history(out["baselines"][str(L)], rd.buckets["train"][L][1].numpy(), rd.buckets["test"][L][1].numpy(), ks)
    tags = [json.loads(line)["tag"] for line in open(tb / "scalars.jsonl")]
    assert "baseline/Oracle_F1" in tags and "baseline/Greedy_k_DCG" in tags and "baseline/Fixed_k30_F1" in tags
