"""Pin tests/mmoe_bicut_restate.py (the float64 numpy restatement tests/test_mmoe_bicut_gpu.py compares the kernels with) to
independent sources: the CPU oracle's BiCutLoss and the reference's golden for it, and torch float64 autograd for the gates,
the mixture and the two-class head.  float64 against float64: 1e-12 (of max(1, largest reference value)).  The golden holds
what the reference computed in float32, so it carries the tolerances tests/test_oracle_golden.py gives it.  CPU only."""
import numpy as np
import pytest
import torch

import golden_util as gu
import mmoe_bicut_restate as R
from oracle import losses as ol

TOL = 1e-12


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------- BiCutLoss
def oracle_bicut(out, labels, metric, alpha, r):
    o = torch.from_numpy(out).double().requires_grad_(True)
    loss = ol.BiCutLoss(alpha=alpha, r=r, metric=metric)(o, torch.from_numpy(labels))
    loss.backward()
    return loss.item(), o.grad.numpy()


@pytest.mark.parametrize("B,S,only", [(9, 1, None), (9, 2, None), (9, 64, None), (18, 129, None), (37, 300, None),
                                      (4, 129, 64), (4, 129, "none"), (4, 129, "ties"), (3, 65, "end")], ids=str)
def test_bicut_loss_against_the_oracle(B, S, only):
    """the placed edges of bicut_edge_lists (last class-0 position at 0 / 63 / 64 / 127 / 128 / S - 1, none, ties; labels all
    0, all 1, a single 1): mask end as placed, value and gradient as the oracle's in float64.  The oracle keeps the reward
    pairs in a float32 tensor like the reference; reward_dtype = float32 rounds the restatement's in the same place."""
    out, labels, idx = R.bicut_edge_lists(B, S, only=only)
    np.testing.assert_array_equal(R.bicut_last_truncate(out), idx)
    np.testing.assert_array_equal(ol.bicut_last_truncate(torch.from_numpy(out)).numpy(), idx)
    for metric in ("nci", "f1"):
        for alpha, r in ((0.65, 0.1), (0.65, 0.0971134020)):
            per, loss, dout, mask, abs_terms = R.bicut_loss(out, labels, metric == "nci", alpha, r, reward_dtype=np.float32)
            want_loss, want_dout = oracle_bicut(out, labels, metric, alpha, r)
            assert abs(loss - want_loss) <= TOL * max(1.0, abs(want_loss)), (metric, loss, want_loss)
            assert close(dout, want_dout), metric
            assert ((mask == 0) == (np.arange(S)[None, :] > idx[:, None])).all()
            assert (dout[mask == 0] == 0).all() and (abs_terms >= np.abs(per) * (1 - 1e-15)).all()
            # float64 rewards are the float32 ones up to a float32 rounding
            _, loss64, dout64, _, _ = R.bicut_loss(out, labels, metric == "nci", alpha, r)
            assert abs(loss64 - loss) <= 1e-7 * float(abs_terms.sum()) / B
            assert (np.abs(dout64 - dout) <= 6e-8 * np.abs(dout64)).all()


def test_bicut_loss_ties_and_empty_rows():
    """by hand: a tie is class 0; a row without a class-0 position is not masked; S = 1"""
    out = np.array([[[0.5, 0.5], [0.2, 0.8], [0.5, 0.5], [0.1, 0.9]],
                    [[0.3, 0.7], [0.2, 0.8], [0.4, 0.6], [0.1, 0.9]],
                    [[0.9, 0.1], [0.2, 0.8], [0.4, 0.6], [0.1, 0.9]]], dtype=np.float32)
    np.testing.assert_array_equal(R.bicut_last_truncate(out), [2, 4, 0])
    labels = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
    per, loss, dout, mask, _ = R.bicut_loss(out, labels, False, 0.65, 0.1)
    o = out.astype(np.float64)
    want = [o[0, 0, 1] * 0.65 / 0.9 + o[0, 1, 0] * 0.35 / 0.1 + o[0, 2, 1] * 0.65 / 0.9,
            o[1, 0, 0] * 0.35 / 0.1 + (o[1, 1, 1] + o[1, 2, 1] + o[1, 3, 1]) * 0.65 / 0.9,
            o[2, 0, 1] * 0.65 / 0.9]
    assert close(per, want) and abs(loss - sum(want) / 3) < TOL
    np.testing.assert_array_equal(mask, [[1, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 0]])
    per, _, dout, _, _ = R.bicut_loss(out[:, :1], labels[:, :1], True, 0.65, 0.1)
    assert close(per, [o[0, 0, 1] / 0.65, -o[1, 0, 1], o[2, 0, 1] / 0.65])
    assert close(dout[:, 0, 1], [1 / 0.65 / 3, -1.0 / 3, 1 / 0.65 / 3]) and (dout[:, 0, 0] == 0).all()


def test_bicut_loss_against_the_reference_golden():
    gold = gu.load("bicutloss_edge_s50")
    out = torch.softmax(torch.from_numpy(gold["logits"]), dim=2).numpy()
    for metric in ("nci", "f1"):
        _, loss, dout, _, _ = R.bicut_loss(out, gold["y"], metric == "nci", 0.65, 0.0971134020, reward_dtype=np.float32)
        ref = float(gold["loss/" + metric])
        assert abs(loss - ref) <= 2e-6 * max(1.0, abs(ref)), (metric, loss, ref)
        np.testing.assert_allclose(dout, gold["dout/" + metric], rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------- gates and mixture
@pytest.mark.parametrize("B,S,C,nt,ne,E", [(3, 5, 7, 1, 4, 12), (4, 2, 65, 3, 1, 4), (5, 3, 6, 2, 3, 8)], ids=str)
def test_gates_and_mixture_against_autograd(B, S, C, nt, ne, E):
    """the formula tools/gpu_probe.py's embed_mmoe section uses: softmax(h.reshape(B, -1) @ w) and the gate-weighted expert sum,
    torch float64 autograd; the restatement takes and returns the position-major layouts of the header"""
    gen = torch.Generator().manual_seed(B * 1009 + S * 101 + C)
    h = torch.randn(B, S, C, generator=gen, dtype=torch.float64).requires_grad_(True)
    w = [(torch.randn(S * C, ne, generator=gen, dtype=torch.float64) / (S * C) ** 0.5).requires_grad_(True) for _ in range(nt)]
    ex = [torch.randn(B, S, E, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(ne)]
    dm = torch.randn(nt, B, S, E, generator=gen, dtype=torch.float64)
    g = [torch.softmax(h.reshape(B, -1) @ wt, 1) for wt in w]
    est = torch.stack(ex)
    mixed = torch.stack([(gt.t()[:, :, None, None] * est).sum(0) for gt in g])
    gs = torch.stack(g)
    gs.retain_grad()
    mixed_from = torch.stack([(gs[t].t()[:, :, None, None] * est).sum(0) for t in range(nt)])
    mixed_from.backward(dm)
    dgates_want = gs.grad.numpy().copy()
    dex_want = [e.grad.numpy().copy() for e in ex]

    pm = lambda a: R.to_position_major(a.detach().numpy())                                # noqa: E731
    h_pm, w_np, ex_pm = pm(h), [wt.detach().numpy() for wt in w], np.stack([pm(e) for e in ex])
    dm_pm = np.stack([pm(dm[t]) for t in range(nt)])
    gates = R.gates(h_pm, w_np, S, B)
    assert close(gates, gs.detach().numpy()) and close(gates.sum(-1), np.ones((nt, B)))
    assert close(R.mix_fwd(ex_pm, gates, B), np.stack([pm(mixed[t]) for t in range(nt)]))
    dx, dg = R.mix_bwd(ex_pm, gates, dm_pm, B)
    assert close(dg, dgates_want)
    for e in range(ne):
        assert close(R.from_position_major(dx[e], B, S), dex_want[e])
    dl, dh, dw = R.gate_bwd(h_pm, w_np, gates, dg, S, B)
    assert close(dl, R.gate_dlogit(gates, dg))
    if ne == 1:
        assert (dl == 0).all() and (dh == 0).all() and (dw == 0).all()
    assert close(R.from_position_major(dh, B, S), h.grad.numpy())
    for t in range(nt):
        assert close(dw[t], w[t].grad.numpy())


# ---------------------------------------------------------------------------------------------- two-class head
@pytest.mark.parametrize("B,S,p", [(1, 1, 0.0), (3, 5, 0.3), (6, 9, 0.5)], ids=str)
def test_pair_softmax_against_autograd(B, S, p):
    gen = torch.Generator().manual_seed(B * 31 + S)
    z = torch.randn(S * B, 2, generator=gen, dtype=torch.float64).requires_grad_(True)
    keep = (torch.rand(S * B, 2, generator=gen) >= p).double() / (1.0 - p)
    dout = torch.randn(B, S, 2, generator=gen, dtype=torch.float64)
    out = torch.softmax(z * keep, 1).reshape(S, B, 2).permute(1, 0, 2)
    out.backward(dout)
    got = R.pair_softmax(z.detach().numpy(), keep.numpy(), S, B)
    assert got.shape == (B, S, 2) and close(got, out.detach().numpy())
    dz = R.pair_softmax_bwd(got, dout.numpy(), keep.numpy(), S, B)
    assert close(dz, z.grad.numpy())
    if p > 0:
        assert (keep.numpy() == 0).any() and (dz[keep.numpy() == 0] == 0).all()


# ---------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("B,S,F", [(1, 1, 1), (3, 5, 3), (4, 7, 2)], ids=str)
def test_layout_maps_and_embedding(B, S, F):
    x = np.arange(B * S * F, dtype=np.float32).reshape(B, S, F)
    pm = R.to_position_major(x)
    for b in range(B):
        for s in range(S):
            assert (pm[s * B + b] == x[b, s]).all()
    assert np.array_equal(R.from_position_major(pm, B, S), x)
    assert np.array_equal(pm, torch.from_numpy(x).permute(1, 0, 2).reshape(S * B, F).numpy())
    score = np.arange(B * S, dtype=np.float32).reshape(B, S) + 0.5
    pe = -np.arange(S * F, dtype=np.float32).reshape(S, F) - 1
    want = torch.cat((torch.from_numpy(score)[:, :, None], torch.from_numpy(pe).expand(B, S, F)), 2)      # models/Choopy.py:19-20
    assert np.array_equal(R.choopy_embed(score, pe), R.to_position_major(want.numpy()))
