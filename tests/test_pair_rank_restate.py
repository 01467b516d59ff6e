"""tests/pair_rank_restate.py, the float64 specification of rlt_pair_rank_loss, checked on the CPU: its gradient is torch float64
autograd's at 1e-12 (RankNet: of the restated loss itself; LambdaRank: with the weights held constant), its counting rank is
the stable argsort's inverse on NaN-free input with ties and signed zeros, and it has teeth - on the input classes of the GPU test
each of three planted mistakes moves the loss or a gradient by more than 100x the GPU test's tolerance."""
import numpy as np
import pytest
import torch

import pair_rank_restate as PR

SIGMAS = {"ranknet": 1.0, "lambdarank": 2.5}


def torch_loss(score, labels, kind, sigma, gains, normalize, rank):
    """The batch loss written once more, in torch float64 with torch's own softplus, as a function of a leaf tensor."""
    s = torch.tensor(np.asarray(score, np.float32).astype(np.float64), requires_grad=True)
    B, S = s.shape
    sig = float(np.float32(sigma))
    total = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        g = PR.grades(labels[b], len(gains))
        pair = torch.tensor(g[:, None] > g[None, :])
        n = int(pair.sum())
        if n == 0:
            continue
        x = sig * (s[b][:, None] - s[b][None, :])
        l = torch.nn.functional.softplus(-x, beta=1.0, threshold=1000.0)     # (the default threshold of 20 makes it linear beyond)
        if kind == "lambdarank":
            G = np.array([float(np.float32(v)) for v in gains])[g]
            D = PR.discount(rank[b])
            w = np.abs(G[:, None] - G[None, :]) * np.abs(D[:, None] - D[None, :])
            ideal = PR.ideal_value(g, gains)
            if normalize and ideal > 0:
                w = w / ideal
            total = total + (torch.tensor(w).detach() * l)[pair].sum()
        else:
            total = total + l[pair].sum() / n
    return s, total / B


@pytest.mark.parametrize("name", sorted(PR.CLASSES))
@pytest.mark.parametrize("kind", ["ranknet", "lambdarank"])
def test_gradient_is_autograd(kind, name):
    sigma = SIGMAS[kind]
    for S, B in ((1, 2), (2, 3), (7, 3), (40, 5), (65, 2)):
        score, labels = PR.inputs(name, B, S, sigma=sigma, seed=S)
        kw = PR.class_args(name)
        gains = kw.get("gains") or PR.default_gains(kw["n_grades"])
        for normalize in (True, False):
            ref = PR.restate(score, labels, kind, sigma=sigma, normalize=normalize, **kw)
            s, loss = torch_loss(score, labels, kind, sigma, gains, normalize, ref["rank"])
            assert abs(float(loss) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
            if loss.requires_grad:
                loss.backward()
                grad = s.grad.numpy()
            else:
                grad = np.zeros_like(ref["dscore"])
            assert np.abs(grad - ref["dscore"]).max() <= 1e-12 * max(1.0, np.abs(ref["dscore"]).max())
            if name in PR.PAIRLESS or S == 1:
                assert ref["loss"] == 0.0 and not ref["dscore"].any() and not ref["n_pairs"].any()


def test_gscale_scales_the_gradient_only():
    score, labels = PR.inputs("graded", 3, 40, seed=1)
    a = PR.restate(score, labels, "lambdarank", sigma=0.7, gains=list(PR.CUSTOM_GAINS))
    b = PR.restate(score, labels, "lambdarank", sigma=0.7, gains=list(PR.CUSTOM_GAINS), gscale=-3.5)
    assert a["loss"] == b["loss"] and np.array_equal(a["loss_per_list"], b["loss_per_list"])
    assert np.allclose(b["dscore"], -3.5 * a["dscore"], rtol=1e-13, atol=0) and np.allclose(b["A"], 3.5 * a["A"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("S", [1, 2, 3, 17, 64, 65, 300])
def test_counting_rank_is_the_stable_argsort_inverse(S):
    rng = np.random.default_rng(S)
    for name in ("randn", "ties", "saturated"):
        s, _ = PR.inputs(name, 4, S, seed=3)
        if S >= 3:
            s[0, :3] = (0.0, -0.0, 0.0)
            s[1, -2:] = (-0.0, 0.0)
        s[2] = rng.permutation(s[2])
        want = np.stack([np.argsort(np.argsort(-row, kind="stable"), kind="stable") for row in s]).astype(np.int32)
        got = PR.counting_rank(s)
        assert np.array_equal(got, want)
        assert all(sorted(row) == list(range(S)) for row in got)


def test_grades_follow_the_reward_spec_rule():
    y = np.array([0.0, 0.49, 0.5, 1.5, 2.5, -3.0, 7.4, 9.0, np.nan, -0.0], np.float32)
    assert PR.grades(y, 8).tolist() == [0, 0, 0, 2, 2, 0, 7, 7, 0, 0]          # round half to even, clamp, NaN -> 0
    assert PR.grades(y, 2).tolist() == [0, 0, 0, 1, 1, 0, 1, 1, 0, 0]
    g = PR.grades(np.array([3, 3, 4, 0, 7], np.float32), 8)
    # descending gain: 7 (31.5), 3 (3.0) twice, 4 (2.5)
    want = 31.5 * PR._PREFIX[1] + 3.0 * (PR._PREFIX[3] - PR._PREFIX[1]) + 2.5 * (PR._PREFIX[4] - PR._PREFIX[3])
    assert PR.ideal_value(g, PR.CUSTOM_GAINS) == want


@pytest.mark.parametrize("mistake", PR.MISTAKES)
@pytest.mark.parametrize("name", [n for n in sorted(PR.CLASSES) if n not in PR.PAIRLESS])
def test_restatement_has_teeth(name, mistake):
    """On at least one (S, B, kind) id of every input class with pairs, the planted mistake moves the restated loss or a restated
    gradient by more than 100x the bound the GPU test asserts (K = PR.K_ASSERT)."""
    K = 100.0 * PR.K_ASSERT
    moved = 0
    for S in (3, 64, 65, 300):
        for kind in ("ranknet", "lambdarank"):
            sigma = SIGMAS[kind]
            score, labels = PR.inputs(name, 3, S, sigma=sigma, seed=0)
            kw = PR.class_args(name)
            ref = PR.restate(score, labels, kind, sigma=sigma, **kw)
            bad = PR.restate(score, labels, kind, sigma=sigma, mistake=mistake, **kw)
            dl = np.abs(bad["loss_per_list"] - ref["loss_per_list"]) > PR.loss_bound(ref["loss_per_list"], K)
            dg = np.abs(bad["dscore"] - ref["dscore"]) > PR.grad_bound(ref["dscore"], ref["A"], K)
            moved += bool(dl.any() or dg.any())
    assert moved >= 1, (name, mistake)
