"""Pin tests/loss_restate.py (the float64 numpy restatement the GPU dispatch tests compare against) to the reference's own
numbers: the golden vectors the reference produced (tests/golden/losses_edge_s300.npz, task_metrics_s300.npz) and the CPU
oracle at list lengths the goldens do not cover.  Tolerances are the ones those goldens carry in test_oracle_golden.py.
CPU only."""
import numpy as np
import pytest
import torch

import golden_util as gu
import loss_restate as lr
from oracle import losses as ol, metrics as om
from oracle.cases import SINGLE_CRITERIA, make_criterion


def _kind_of(cname):
    """criterion name -> (metric, kind, tau) as the reference's classes set them"""
    parts = cname.split("_")
    if parts[0] == "div":
        return parts[2], lr.KL if parts[1] == "kl" else lr.JS, 0.85 if parts[3] == "aug1" else 1.0
    if parts[0] == "choopy":
        return parts[1], lr.EXPECT, 1.0
    return parts[1], lr.CE, 0.95


@pytest.fixture(scope="module")
def gold():
    return gu.load("losses_edge_s300")


def test_reward_matrix_against_reference(gold):
    for metric, tol in (("f1", 2e-7), ("dcg", 2e-5)):
        assert np.abs(lr.reward(gold["y"], metric) - gold["reward/" + metric]).max() <= tol
    for pen in (-0.5, -2.0, 0.25):
        got = lr.reward(gold["y"][[0, 1, 4, 7]], "dcg", pen)
        assert np.abs(got - gold[f"reward_dcg_pen/{pen:g}"]).max() < 4e-5


@pytest.mark.parametrize("cname", SINGLE_CRITERIA)
def test_loss_and_gradient_against_reference(gold, cname):
    metric, kind, tau = _kind_of(cname)
    p = torch.softmax(torch.from_numpy(gold["logits"]), dim=1).numpy()
    _, loss, dp, _, _ = lr.reward_loss(p, gold["y"], metric, kind, tau)
    ref = float(gold["loss/" + cname])
    assert abs(loss - ref) <= 2e-6 * max(1.0, abs(ref)), (loss, ref)
    want = gold["dp/" + cname]
    assert np.abs(dp - want).max() <= 2e-5 * np.abs(want).max()


def test_cut_metrics_against_reference(gold):
    y, k = gold["y"], gold["k_s"]
    p = torch.softmax(torch.from_numpy(gold["logits"]), dim=1).numpy()
    np.testing.assert_array_equal(lr.cut_positions(p), om.cut_positions(p))
    assert abs(lr.f1_at(y, k).mean() - float(gold["metric_f1"])) < 1e-6
    assert abs(lr.dcg_at(y, k).mean() - float(gold["metric_dcg"])) < 1e-12
    for pen in (-0.5, -2.0, 0.25):
        assert abs(lr.dcg_at(y, k, pen).mean() - float(gold[f"metric_dcg_pen/{pen:g}"])) < 1e-9
    kat_x, kat_k = np.array([[1, 0, 1], [0, 0, 1], [1, 0, 0]], dtype=np.float32), np.array([1, 2, 1])
    assert abs(lr.f1_at(kat_x, kat_k).mean() - float(gold["kat_f1"])) < 1e-15
    assert abs(lr.dcg_at(kat_x, kat_k).mean() - float(gold["kat_dcg"])) < 1e-15


def test_task_metrics_against_reference():
    tg = gu.load("task_metrics_s300")
    assert abs(lr.task_dcg(tg["y"], tg["pred"]).mean() - float(tg["taskr"])) < 1e-9
    for key, want in (("pred", "taskc"), ("pred_ties", "taskc_ties")):
        auc = lr.task_auc(tg["y"], tg[key])
        assert abs(auc[auc >= 0].mean() - float(tg[want])) < 1e-12
    # a list with one class is skipped (-1), whatever the predictions
    y = np.stack([np.zeros(7), np.ones(7), np.array([0, 1, 0, 0, 1, 0, 0.])]).astype(np.float32)
    auc = lr.task_auc(y, np.tile(np.linspace(0, 1, 7, dtype=np.float32), (3, 1)))
    assert auc[0] == -1.0 and auc[1] == -1.0 and auc[2] == (1 + 3) / 10


@pytest.mark.parametrize("tag,nt", [("t3", 3), ("t21", 2.1), ("t22", 2.2)])
@pytest.mark.parametrize("metric", ["f1", "dcg"])
def test_multitask_terms_against_reference(gold, tag, nt, metric):
    """MtCutLoss = JS cut loss + 0.4 * rerank hinge + 0.6 * BCE, and its gradients with respect to the rerank scores and the
    class logits (d/dlogit = d/dc * c (1 - c))."""
    y = gold["y"]
    p = torch.softmax(torch.from_numpy(gold["logits"]), dim=1).numpy()
    c = torch.sigmoid(torch.from_numpy(gold["cls_logit"])).numpy()
    terms = lr.mt_terms(gold["rerank"] if nt != 2.1 else None, c if nt != 2.2 else None, y, 5e-4)
    _, cut, _, _, _ = lr.reward_loss(p, y, metric, lr.JS, 0.85)
    key = f"mtcut_{tag}_{metric}"
    assert abs(cut + 0.4 * terms[0] + 0.6 * terms[1] - float(gold["loss/" + key])) <= 2e-6
    d_rerank, d_class = lr.mt_terms_bwd(c if nt != 2.2 else None, y, terms, 0.4, 0.6)
    if nt != 2.1:
        assert terms[0] > 0
        assert np.abs(d_rerank - gold["drerank/" + key]).max() <= 1e-7
    if nt != 2.2:
        c64 = c.astype(np.float64)
        assert np.abs(d_class * c64 * (1 - c64) - gold["dcls_logit/" + key]).max() <= 1e-7


def test_multitask_edges():
    y = np.array([[1, 0, 0, 1.]], dtype=np.float32)
    s = np.array([[0.3, 0.1, 0.2, 0.9]], dtype=np.float32)
    assert np.array_equal(lr.mt_terms(s, None, np.ones_like(y), 5e-4), np.zeros(4))          # no y == 0 entry
    assert np.array_equal(lr.mt_terms(s, None, y, -10.0), np.zeros(4))                        # hinge inactive
    t = lr.mt_terms(s, None, y, 0.5)
    assert abs(t[0] - (0.15 - 0.6 + 0.5)) < 1e-7 and t[2] == -0.5 and t[3] == 0.5
    # the -100 clamp of nn.BCELoss and torch's backward at c = 0 / 1 exactly
    c = np.array([[0.0, 1.0, 0.5, 1.0]], dtype=np.float32)
    want = torch.nn.functional.binary_cross_entropy(torch.from_numpy(c).double(), torch.from_numpy(y).double())
    assert abs(lr.mt_terms(None, c, y, 0.0)[1] - float(want)) < 1e-12 and float(want) > 50
    cg = torch.from_numpy(c).double().requires_grad_(True)
    torch.nn.functional.binary_cross_entropy(cg, torch.from_numpy(y).double()).backward()
    _, d_class = lr.mt_terms_bwd(c, y, np.zeros(4), 0.0, 1.0)
    np.testing.assert_allclose(d_class, cg.grad.numpy(), rtol=1e-12)


def _lists(S, seed, B=7):
    g = np.random.default_rng(seed)
    y = (g.random((B, S)) < 0.2).astype(np.float32)
    y[0] = 0
    y[1] = 1
    y[2] = 0
    y[2, 0] = 1
    y[3] = 0
    y[3, -1] = 1
    z = 3.0 * g.standard_normal((B, S))
    p = np.exp(z - z.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    p[4] = np.float32(1.0 / S)
    return y, p


@pytest.mark.parametrize("S", [1, 3, 65, 129, 321, 513])
def test_against_the_oracle_at_other_lengths(S):
    y, p = _lists(S, 1000 + S)
    for cname in SINGLE_CRITERIA:
        metric, kind, tau = _kind_of(cname)
        yy = y
        if metric == "dcg" and lr.reward(y, metric).max() / tau > 80:
            yy = np.delete(y, 1, axis=0)             # exp(r / tau) of the all-relevant list leaves fp32 in the reference
        pp = p[:len(yy)]
        assert lr.reward(yy, metric).max() / tau <= 80
        pt = torch.from_numpy(pp).unsqueeze(2).requires_grad_(True)
        lo = make_criterion(ol, cname)(pt, torch.from_numpy(yy))
        lo.backward()
        _, loss, dp, r, _ = lr.reward_loss(pp, yy, metric, kind, tau)
        assert np.abs(r - ol.reward_matrix(torch.from_numpy(yy), metric).numpy()).max() <= (2e-7 if metric == "f1" else 2e-5 * max(1.0, np.abs(r).max()))
        assert abs(loss - lo.item()) <= 2e-6 * max(1.0, abs(lo.item())), (cname, loss, lo.item())
        want = pt.grad.squeeze(2).numpy()
        assert np.abs(dp - want).max() <= 2e-5 * np.abs(want).max(), cname
    k = lr.cut_positions(p)
    np.testing.assert_array_equal(k, om.cut_positions(p))
    assert k[4] == 1
    for kk in (k, np.ones(len(y), dtype=np.int64), np.full(len(y), S)):
        assert np.abs(lr.f1_at(y, kk) - om.f1_per_list(y, kk)).max() < 1e-12
        for pen in (-1.0, 0.25):
            assert np.abs(lr.dcg_at(y, kk, pen) - om.dcg_per_list(y, kk, pen)).max() < 1e-12
    pred = np.round(p / p.max() * 3) / 3                # four levels: heavy ties
    for pr in (p, pred.astype(np.float32)):
        assert abs(lr.task_dcg(y, pr).mean() - om.taskr_metric(y, pr)) < 1e-9
        auc = lr.task_auc(y, pr)
        assert auc[0] == -1.0 and auc[1] == -1.0
        if S > 1:
            assert abs(auc[auc >= 0].mean() - om.taskc_metric(y, pr)) < 1e-12
