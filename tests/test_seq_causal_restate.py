"""tests/seq_causal_restate.py pinned on the host: to float64 torch.nn.MultiheadAttention(batch_first=True) called with the boolean
upper-triangular attn_mask, forward and autograd gradients, at 1e-12; and the yardsticks of the device tests
(tests/test_seq_causal_gpu.py): on the `ramp_v` input, for every shape used there, every way of getting the diagonal wrong moves the
float64 reference by more than 100 x the device tolerances - in every 32-position block the mistake touches."""
import numpy as np
import pytest
import torch

import seq_attention_restate as R
import seq_causal_restate as C


def to_pm(x):
    B, S, E = x.shape
    return x.transpose(0, 1).reshape(S * B, E)


def from_pm(x, S, B):
    return x.reshape(S, B, -1).transpose(0, 1)


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("B,S,E,H", [(3, 7, 32, 2), (2, 17, 64, 4), (2, 5, 64, 1), (1, 1, 16, 1)])
def test_restatement_is_multihead_attention_with_the_causal_mask(B, S, E, H):
    torch.manual_seed(B * 100 + S)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True).double()
    x = torch.randn(B, S, E, dtype=torch.float64, requires_grad=True)
    g = torch.randn(B, S, E, dtype=torch.float64)
    banned = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)           # True = not allowed to attend
    y, weights = mha(x, x, x, attn_mask=banned, need_weights=True, average_attn_weights=False)
    y.backward(g)
    w_in, b_in = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    w_out, b_out = mha.out_proj.weight.detach(), mha.out_proj.bias.detach()
    qkv = to_pm(x.detach() @ w_in.t() + b_in).numpy()
    HD = E // H
    out, lse, p = C.forward(qkv, S, B, H, HD)
    assert rel(from_pm(torch.from_numpy(out), S, B) @ w_out.t() + b_out, y.detach()) < 1e-12
    assert rel(torch.from_numpy(p), weights.detach()) < 1e-12
    assert not p[..., np.triu_indices(S, 1)[0], np.triu_indices(S, 1)[1]].any()                # exactly 0 above the diagonal
    q, k, _ = R.heads(qkv, S, B, H, HD)
    scores = (torch.from_numpy(q @ k.transpose(0, 1, 3, 2)) / HD ** 0.5).masked_fill(banned, -float("inf"))
    assert rel(torch.from_numpy(lse), torch.logsumexp(scores, -1)) < 1e-12
    dqkv = torch.from_numpy(C.backward(qkv, to_pm(g @ w_out).numpy(), S, B, H, HD))
    assert rel(dqkv.t() @ to_pm(x.detach()), mha.in_proj_weight.grad) < 1e-12
    assert rel(dqkv.sum(0), mha.in_proj_bias.grad) < 1e-12
    assert rel(from_pm(dqkv @ w_in, S, B), x.grad) < 1e-12


def test_the_full_mask_is_the_unmasked_restatement_and_dropout_is_autograd():
    S, B, H, HD = 9, 2, 2, 16
    qkv, dout = C.inputs("randn", S, B, H, HD)
    full = np.ones((S, S), dtype=bool)
    for a, b in zip(C.forward(qkv, S, B, H, HD, allow=full), R.forward(qkv, S, B, H, HD)):
        assert np.array_equal(a, b)
    assert np.array_equal(C.backward(qkv, dout, S, B, H, HD, allow=full), R.backward(qkv, dout, S, B, H, HD))
    mask = C.keep_mask(7, S, B, H, 0.3)
    x = torch.from_numpy(R.heads(qkv, S, B, H, HD)).requires_grad_(True)
    s = (x[0] @ x[1].transpose(-1, -2) / HD ** 0.5).masked_fill(~torch.from_numpy(C.causal(S)), -float("inf"))
    o = (torch.softmax(s, -1) * torch.from_numpy(mask)) @ x[2]
    o.backward(torch.from_numpy(R.heads(dout, S, B, H, HD)[0]))
    assert R.rel(C.forward(qkv, S, B, H, HD, mask)[0], R.rows(o.detach().numpy()[None])) < 1e-13
    assert R.rel(C.backward(qkv, dout, S, B, H, HD, mask), R.rows(x.grad.numpy())) < 1e-12


def test_row_zero_and_the_prefix_property_of_the_restatement():
    S, B, H, HD = 40, 2, 2, 16
    qkv, dout = C.inputs("ramp_v", S, B, H, HD)
    out, lse, _ = C.forward(qkv, S, B, H, HD)
    assert np.array_equal(out[:B], qkv[:B, 2 * H * HD:].astype(np.float64))                     # position 0: V at position 0
    j = 17
    q2 = qkv.copy()
    q2[j * B:] = 8 * np.random.default_rng(1).standard_normal(q2[j * B:].shape)
    out2, lse2, _ = C.forward(q2, S, B, H, HD)
    assert np.array_equal(out2[:j * B], out[:j * B]) and np.array_equal(lse2[..., :j], lse[..., :j])
    assert not np.array_equal(out2[j * B:], out[j * B:])


def test_yardsticks_every_wrong_diagonal_moves_the_reference():
    """ramp_v, every shape of the device tests with S >= 2: the diagonal dropped (`strict`), one key too many (`one_more`), the mask at
    32- and 64-key granularity, no mask, the transposed mask - each moves `out` by more than 100 x FWD_TOL of max |out| in every
    32-position query block whose rows it changes at all, and dqkv by more than 100 x GRAD_TOL of max |dqkv|"""
    worst = {}
    for S, B, H, HD in R.SHAPES:
        if S < 2:
            continue
        qkv, dout = C.inputs("ramp_v", S, B, H, HD)
        ref = C.forward(qkv, S, B, H, HD)[0]
        gref = C.backward(qkv, dout, S, B, H, HD)
        base = C.causal(S)
        for name, allow in C.variants(S).items():
            changed = (allow != base).any(-1)
            blocks = np.array([changed[t:t + 32].any() for t in range(0, S, 32)])
            if not blocks.any():
                continue
            mv = C.block_moves(C.forward(qkv, S, B, H, HD, allow=allow)[0], ref, S, B, np.abs(ref).max())
            gv = R.rel(C.backward(qkv, dout, S, B, H, HD, allow=allow), gref)
            assert mv[blocks].min() > 100 * R.FWD_TOL, (name, (S, B, H, HD), mv)
            assert gv > 100 * R.GRAD_TOL, (name, (S, B, H, HD), gv)
            o, g = worst.get(name, (np.inf, np.inf))
            worst[name] = (min(o, float(mv[blocks].min())), min(g, gv))
    assert set(worst) == set(C.variants(2))
    print({k: "out %.3g dqkv %.3g" % v for k, v in worst.items()})
