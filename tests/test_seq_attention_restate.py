"""tests/seq_attention_restate.py pinned on the host: to float64 torch.nn.MultiheadAttention(batch_first=True), to a float64
nn.TransformerEncoderLayer(batch_first=True, dropout=0) forward and autograd gradients, and the yardsticks of the device tests
(tests/test_seq_attention_gpu.py): for every input class and shape used there, each way of getting a tile tail wrong moves the
float64 reference by more than 100 x the forward tolerance."""
import numpy as np
import pytest
import torch

import dropout_restate as D
import seq_attention_restate as R


def to_pm(x):
    """(B, S, C) -> position-major (S*B, C)"""
    B, S, C = x.shape
    return x.transpose(0, 1).reshape(S * B, C)


def from_pm(x, S, B):
    return x.reshape(S, B, -1).transpose(0, 1)


class RestatedAttention(torch.autograd.Function):
    """the numpy restatement as a float64 tape node: position-major qkv -> position-major concatenated heads"""

    @staticmethod
    def forward(ctx, qkv, S, B, H):
        HD = qkv.shape[1] // (3 * H)
        ctx.dims = (S, B, H, HD)
        ctx.save_for_backward(qkv)
        return torch.from_numpy(R.forward(qkv.detach().numpy(), S, B, H, HD)[0])

    @staticmethod
    def backward(ctx, dout):
        qkv, = ctx.saved_tensors
        return torch.from_numpy(R.backward(qkv.detach().numpy(), dout.numpy(), *ctx.dims)), None, None, None


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("B,S,E,H", [(3, 7, 32, 2), (2, 17, 64, 4), (2, 5, 64, 1)])
def test_restatement_is_multihead_attention_batch_first(B, S, E, H):
    torch.manual_seed(B * 100 + S)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True).double()
    x = torch.randn(B, S, E, dtype=torch.float64, requires_grad=True)
    g = torch.randn(B, S, E, dtype=torch.float64)
    y, weights = mha(x, x, x, need_weights=True, average_attn_weights=False)
    y.backward(g)
    w_in, b_in = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    w_out, b_out = mha.out_proj.weight.detach(), mha.out_proj.bias.detach()
    qkv = to_pm(x.detach() @ w_in.t() + b_in).numpy()
    out, lse, p = R.forward(qkv, S, B, H, E // H)
    assert rel(from_pm(torch.from_numpy(out), S, B) @ w_out.t() + b_out, y.detach()) < 1e-12
    assert rel(torch.from_numpy(p), weights.detach()) < 1e-12
    q, k, _ = R.heads(qkv, S, B, H, E // H)
    scores = torch.from_numpy(q @ k.transpose(0, 1, 3, 2)) / (E // H) ** 0.5
    assert rel(torch.from_numpy(lse), torch.logsumexp(scores, -1)) < 1e-12
    dqkv = torch.from_numpy(R.backward(qkv, to_pm(g @ w_out).numpy(), S, B, H, E // H))
    assert rel(dqkv.t() @ to_pm(x.detach()), mha.in_proj_weight.grad) < 1e-12
    assert rel(dqkv.sum(0), mha.in_proj_bias.grad) < 1e-12
    assert rel(from_pm(dqkv @ w_in, S, B), x.grad) < 1e-12


@pytest.mark.parametrize("B,S,E,H", [(3, 7, 32, 2), (2, 17, 64, 4)])
def test_restated_encoder_layer_is_transformer_encoder_layer_batch_first(B, S, E, H):
    """forward and all 13 gradients (x and the 12 parameters) at 1e-12"""
    torch.manual_seed(S)
    F = torch.nn.functional
    layer = torch.nn.TransformerEncoderLayer(E, H, dim_feedforward=48, dropout=0.0, batch_first=True).double()
    x = torch.randn(B, S, E, dtype=torch.float64, requires_grad=True)
    g = torch.randn(B, S, E, dtype=torch.float64)
    layer(x).backward(g)
    want = [x.grad] + [p.grad for p in layer.parameters()]
    mine = [t.detach().clone().requires_grad_(True) for t in [x] + list(layer.parameters())]
    xm, w_in, b_in, w_o, b_o, w1, b1, w2, b2, n1w, n1b, n2w, n2b = mine
    names = [n for n, _ in layer.named_parameters()]
    assert names == ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                     "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                     "norm2.bias"]
    h = to_pm(xm)
    att = RestatedAttention.apply(h @ w_in.t() + b_in, S, B, H)
    h1 = F.layer_norm(h + att @ w_o.t() + b_o, (E,), n1w, n1b, 1e-5)
    y = F.layer_norm(h1 + torch.relu(h1 @ w1.t() + b1) @ w2.t() + b2, (E,), n2w, n2b, 1e-5)
    assert rel(from_pm(y.detach(), S, B), layer(x).detach()) < 1e-12
    y.backward(to_pm(g))
    for name, a, b in zip(["x"] + names, mine, want):
        assert rel(a.grad, b) < 1e-12, name


def test_keep_mask_follows_the_pair_stream():
    seed, S, B, H, p = 0x1234ABCD, 9, 3, 2, 0.3
    m = R.keep_mask(seed, S, B, H, p)
    thr = D.drop_threshold(p)
    for b, h, i, j in [(0, 0, 0, 0), (2, 1, 8, 3), (1, 0, 4, 8)]:
        keep = bool(D.keep(int(D.pair_seed(seed, b * H + h)), i, j, thr))
        assert m[b, h, i, j] == (float(D.keep_scale(p)) if keep else 0.0)
    assert 0.55 < (m > 0).mean() < 0.85


def test_dropout_restatement_is_autograd_of_the_masked_product():
    S, B, H, HD = 6, 2, 2, 16
    qkv, dout = R.inputs("randn", S, B, H, HD)
    qkv = qkv[:S * B]
    mask = R.keep_mask(7, S, B, H, 0.3)
    x = torch.from_numpy(R.heads(qkv, S, B, H, HD)).requires_grad_(True)
    p = torch.softmax(x[0] @ x[1].transpose(-1, -2) / HD ** 0.5, -1) * torch.from_numpy(mask)
    o = p @ x[2]
    o.backward(torch.from_numpy(R.heads(dout, S, B, H, HD)[0]))
    assert R.rel(R.forward(qkv, S, B, H, HD, mask)[0], R.rows(o.detach().numpy()[None])) < 1e-13
    assert R.rel(R.backward(qkv, dout, S, B, H, HD, mask), R.rows(x.grad.numpy())) < 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
def test_yardsticks_every_tail_mistake_moves_the_reference(kind):
    """for every shape of the device tests: dropping the last key, admitting the (planted) key behind the buffer, reading the
    neighbouring list's row - each more than 100 x the forward tolerance; the zero-row form of `past_S` is printed"""
    worst = {}
    for S, B, H, HD in R.SHAPES:
        qkv, _ = R.inputs(kind, S, B, H, HD)
        y = R.yardsticks(qkv, S, B, H, HD)
        for name in ("drop_last", "past_S", "neighbour"):
            if name in y:
                assert y[name] > 100 * R.FWD_TOL, (kind, (S, B, H, HD), name, y[name])
        for name, v in y.items():
            worst[name] = min(worst.get(name, np.inf), v)
        if kind == "last_key" and S > 1:
            p = R.forward(qkv[:S * B], S, B, H, HD)[2][..., S - 1]
            assert 0.3 <= p.min() and p.max() <= 0.9, ((S, B, H, HD), p.min(), p.max())
        if kind == "neighbour" and B > 1:        # the planted row is dominant for the list that must not read it
            assert y["neighbour"] > 0.3
    print(kind, {k: f"{v:.3g}" for k, v in worst.items()})
