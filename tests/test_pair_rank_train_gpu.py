"""The pairwise ranking losses on the training path: utils.losses.PairwiseRankLoss and MtCutLoss(rerank_loss=...) on the outputs of
MtAttnCut (tasks 3 and 2.2) and MMOECut at B = 5, S = 40, and run.py --rerank-loss end to end.

The multi-task loss must be cut + w_r * pair + w_c * BCE with the pair term from the float64 restatement
(tests/pair_rank_restate.py) on the model's own rerank output; the gradient arriving at the rerank head must be w_r times the
restated dscore.  Bounds: those of tests/test_pair_rank_gpu.py (K_ASSERT) on the pair term, plus what the composition adds and
no more - the cut term is the library's own fp32 number (taken as it is), the BCE an fp32 mean of B S terms compared with float64
at 1e-6 relative (the bound tests/test_hip_parity.py gives that kernel), and one fp32 rounding for each of the two products and
two additions on the tape; the gradient passes one more fp32 multiplication (by the incoming w_r)."""
import json

import numpy as np
import pytest
import torch

import pair_rank_restate as PR

pytestmark = pytest.mark.gpu

B, S = 5, 40
W_R, W_C = 0.3, 0.45


@pytest.fixture(scope="module")
def lib():
    from rlt_hip import native
    native.load()
    return native


def batch(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, generator=g)
    y = (torch.rand(B, S, generator=g) < 0.3).float()
    y[0] = 0.0                                  # a list without pairs
    return x.cuda(), y.cuda()


def build(model_name, num_tasks):
    import models
    torch.manual_seed(7)
    if model_name == "mtattncut":
        return models.MtAttnCut(num_tasks=num_tasks, dropout=0.0).cuda().train()
    return models.MMOECut(seq_len=S, num_tasks=num_tasks, dropout=0.0).cuda().train()


def heads(model, out):
    return dict(zip(model.head_names(), out))


@pytest.mark.parametrize("metric", ["f1", "ndcg"])
@pytest.mark.parametrize("kind", ["ranknet", "lambdarank"])
@pytest.mark.parametrize("model_name,num_tasks,sigma", [("mtattncut", 3, 1.0), ("mtattncut", 2.2, 2.0), ("mmoecut", 3, 40.0)])
def test_multitask_loss_is_cut_plus_pair_plus_bce(lib, model_name, num_tasks, sigma, kind, metric):
    from utils import losses
    model = build(model_name, num_tasks)
    x, y = batch(11)
    crit = losses.MtCutLoss(metric=metric, rerank_weight=W_R, classi_weight=W_C, num_tasks=num_tasks, rerank_loss=kind,
                            rerank_sigma=sigma)
    out = model(x)
    h = heads(model, out)
    h["rerank"].retain_grad()
    loss = crit(out, y)
    loss.backward()
    torch.cuda.synchronize()
    score = h["rerank"].detach().reshape(B, S).cpu().numpy()
    labels = y.cpu().numpy()
    ref = PR.restate(score, labels, kind, sigma=sigma, n_grades=2, normalize=True, gscale=W_R)
    cut = float(losses.DivLoss(metric=metric, div_type="js", augmented=True)(h["decison_layer"].detach(), y))
    want, slack = cut + W_R * ref["loss"], W_R * float(PR.loss_bound(ref["loss"], PR.K_ASSERT))
    if "classi" in h:
        c = h["classi"].detach().reshape(B, S).double().cpu()
        bce = float(torch.nn.functional.binary_cross_entropy(c, y.double().cpu()))
        want += W_C * bce
        slack += 1e-6 * W_C * abs(bce)
    slack += 4 * 2.0 ** -24 * (abs(cut) + abs(want))
    assert abs(float(loss) - want) <= slack, (float(loss), want, slack)
    got = h["rerank"].grad.reshape(B, S).double().cpu().numpy()
    bound = PR.grad_bound(ref["dscore"], ref["A"], PR.K_ASSERT) + PR.fp32_rounding(ref["dscore"])
    assert (np.abs(got - ref["dscore"]) <= bound).all()
    assert not got[0].any() and np.abs(got[1:]).max() > 0       # the pairless list: exactly zero
    # the stand-alone criterion on the same scores: the same loss bits as the raw pass, the unweighted gradient
    leaf = h["rerank"].detach().clone().requires_grad_(True)
    alone = losses.PairwiseRankLoss(kind=kind, sigma=sigma)(leaf, y)
    alone.backward()
    one = PR.restate(score, labels, kind, sigma=sigma)
    assert abs(float(alone) - one["loss"]) <= PR.loss_bound(one["loss"], PR.K_ASSERT)
    assert (np.abs(leaf.grad.reshape(B, S).double().cpu().numpy() - one["dscore"]) <= PR.grad_bound(one["dscore"], one["A"], PR.K_ASSERT)).all()


@pytest.mark.parametrize("metric", ["f1", "ndcg"])
@pytest.mark.parametrize("num_tasks", [3, 2.1, 2.2])
def test_hinge_is_the_path_it_was(lib, num_tasks, metric):
    from utils import losses
    model = build("mtattncut", num_tasks)
    x, y = batch(12)
    with torch.no_grad():
        out = model(x)
    results = []
    for kw in ({}, {"rerank_loss": "hinge"}, {"rerank_loss": "hinge", "rerank_sigma": 9.0}):
        torch.manual_seed(0)
        crit = losses.MtCutLoss(metric=metric, rerank_weight=W_R, classi_weight=W_C, num_tasks=num_tasks, **kw)
        leaves = [o.detach().clone().requires_grad_(True) for o in out]
        loss = crit(tuple(leaves), y)
        loss.backward()
        results.append([loss.detach().cpu().numpy().view(np.int32)] + [t.grad.cpu().numpy().view(np.int32) for t in leaves])
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))


def test_run_with_rerank_loss_end_to_end(lib, tmp_path):
    import run
    from dataloader.synth import write_synthetic_robust04
    from rlt_hip import ops
    base = str(tmp_path / "data")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=48, n_test=44, seed=11, seq_len=300)
    common = ["--model-name", "mtattncut", "--dataset-base", base, "--use-conf", "0", "--batch-size", "64", "--seed", "3", "--dropout", "0.1",
              "--save-path", str(tmp_path / "ckpt"), "--criterion", "f1", "--tensorboard-dir", "", "--synthetic", "0", "--epochs", "1"]
    hist = {}
    for name, extra in (("lambdarank", ["--rerank-loss", "lambdarank", "--rerank-sigma", "2"]), ("hinge", ["--rerank-loss", "hinge"]),
                        ("plain", [])):
        path = str(tmp_path / f"{name}.json")
        ops._SEED_COUNTER[0] = 0                # the dropout seeds count calls per PROCESS: every run here starts as a fresh one does
        run.main(common + extra + ["--history-json", path])
        hist[name] = json.load(open(path))
    assert hist["hinge"] == hist["plain"]
    lam = hist["lambdarank"]["history"][0]
    assert all(np.isfinite(v) for v in lam["train"]) and all(np.isfinite(v) for v in lam["test"])
    assert lam["train"][0] != hist["plain"]["history"][0]["train"][0]
    with pytest.raises(ValueError, match="no rerank head"):
        run.main(common + ["--rerank-loss", "ranknet", "--num-tasks", "2.1"])
    with pytest.raises(ValueError, match="no rerank head"):
        run.main(["--model-name", "attncut"] + common[2:] + ["--rerank-loss", "ranknet"])
