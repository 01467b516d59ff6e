"""Within-list attention on the device (csrc/attention_seq.hip) through the raw C ABI against the float64 restatement
(tests/seq_attention_restate.py, pinned on the host by tests/test_seq_attention_restate.py), and the Python layers above it.

  shapes      seq_attention_restate.SHAPES: every tile-tail fill of both head dims, B in {1, 3, 5}, a head group narrower than a
              workgroup's 64 columns, more than one workgroup per list
  inputs      randn / last_key / neighbour (seq_attention_restate.inputs); qkv is handed over with one planted position behind its
              S * B rows and NaN behind that, every other buffer between NaN guards that must be intact afterwards
  tolerances  relative max-norm 1e-5 for out, 3e-5 for dQ, dK, dV (tests/test_attention_dispatch_gpu.py), for all three precision
              codes; lse within seq_attention_restate.lse_bound per row"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import seq_attention_restate as R

pytestmark = pytest.mark.gpu
GUARD = 4096          # floats of NaN on either side of a buffer


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


class Guarded:
    """a float32 device buffer between two NaN guards"""

    def __init__(self, n, fill=float("nan")):
        self.full = torch.full((n + 2 * GUARD,), float("nan"), device=dev())
        self.t = self.full[GUARD:GUARD + n]
        self.t.fill_(fill)

    @classmethod
    def of(cls, array):
        g = cls(array.size)
        g.t.copy_(torch.from_numpy(np.array(array, dtype=np.float32)).reshape(-1))
        return g

    def intact(self):
        return bool(torch.isnan(self.full[:GUARD]).all()) and bool(torch.isnan(self.full[GUARD + self.t.numel():]).all())


def run(N, qkv, dout, S, B, H, HD, p=0.0, seed=0, prec=None, twice=False):
    """forward and backward through the C ABI -> out (S*B, E), lse (B, H, S), dqkv (S*B, 3E) as float64 numpy.  qkv may carry rows
    behind the call's S * B (the planted position)."""
    from rlt_hip.native import ptr
    E = H * HD
    prec = N.PRECISION_DEFAULT if prec is None else prec
    gq, gd = Guarded.of(qkv), Guarded.of(dout)
    res = []
    for _ in range(2 if twice else 1):
        go, gl, gg = Guarded(S * B * E), Guarded(B * H * S), Guarded(S * B * 3 * E)
        st = N.stream()
        N.call("rlt_seq_attention_fwd", ptr(gq.t), S, B, H, HD, p, seed, ptr(go.t), ptr(gl.t), prec, st)
        assert N.query("rlt_seq_attention_bwd_workspace", S, B, H, HD, p, prec) == 0
        N.call("rlt_seq_attention_bwd", ptr(gq.t), ptr(go.t), ptr(gd.t), ptr(gl.t), S, B, H, HD, p, seed, ptr(gg.t), None, 0, prec, st)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (gq, gd, go, gl, gg)), "a guard was written"
        res.append((go.t.clone(), gl.t.clone(), gg.t.clone()))
    if twice:
        assert all(torch.equal(a, b) for a, b in zip(*res)), "two calls differ"
    o, l, g = res[0]
    return o.view(S * B, E).double().cpu().numpy(), l.view(B, H, S).double().cpu().numpy(), g.view(S * B, 3 * E).double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(kind, shape, p=0.0, seed=0):
    """inputs and float64 reference of one id, computed once: qkv (with the planted tail), dout, out, lse, dqkv, score_max"""
    S, B, H, HD = shape
    qkv, dout = R.inputs(kind, S, B, H, HD)
    mask = R.keep_mask(seed, S, B, H, p) if p > 0 else None
    out, lse, _ = R.forward(qkv[:S * B], S, B, H, HD, mask)
    dqkv = R.backward(qkv[:S * B], dout, S, B, H, HD, mask)
    q, k, _ = R.heads(qkv[:S * B], S, B, H, HD)
    score_max = np.abs(q @ k.transpose(0, 1, 3, 2)).max(-1) / math.sqrt(HD)
    for a in (qkv, dout, out, lse, dqkv, score_max):
        a.setflags(write=False)
    return qkv, dout, out, lse, dqkv, score_max


def check(got, ref, shape, what):
    S, B, H, HD = shape
    E = H * HD
    out, lse, dqkv = got
    _, _, o_ref, l_ref, g_ref, score_max = ref
    if S == 1:
        # one key: P = 1 and dS = P (dP - delta) is the difference of two equal numbers, so dQ = dK = 0 exactly and a relative error has
        # no denominator.  The error is then measured against the size of the cancelling terms, |dP| |k| / sqrt(HD) and |dP| |q| / sqrt(HD)
        # (dP = dout . v per row): the same 3e-5, of what the sum is made of
        q, k, v = R.heads(ref[0][:B], S, B, H, HD)
        dp = np.abs((R.heads(ref[1], S, B, H, HD)[0] * v).sum(-1, keepdims=True)) / math.sqrt(HD)
        fq, fk = float((dp * np.abs(k)).max()), float((dp * np.abs(q)).max())
        assert np.abs(g_ref[:, :2 * E]).max() < 1e-12 * min(fq, fk)
        zero = {"dq": float(np.abs(dqkv[:, :E]).max() / fq), "dk": float(np.abs(dqkv[:, E:2 * E]).max() / fk)}
    else:
        zero = {}
    errs = {"out": R.rel(out, o_ref), "dq": R.rel(dqkv[:, :E], g_ref[:, :E]), "dk": R.rel(dqkv[:, E:2 * E], g_ref[:, E:2 * E]),
            "dv": R.rel(dqkv[:, 2 * E:], g_ref[:, 2 * E:]), "lse": float((np.abs(lse - l_ref) / R.lse_bound(l_ref, score_max)).max())}
    errs.update(zero)
    print(what, shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert not np.isnan(out).any() and not np.isnan(dqkv).any() and not np.isnan(lse).any()
    assert errs["out"] < R.FWD_TOL and errs["lse"] <= 1.0, errs
    assert errs["dq"] < R.GRAD_TOL and errs["dk"] < R.GRAD_TOL and errs["dv"] < R.GRAD_TOL, errs
    return errs


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "S%d-B%d-H%d-HD%d" % s)
def test_abi_against_the_restatement(N, shape, kind):
    ref = case(kind, shape)
    got = run(N, ref[0], ref[1], *shape, prec=N.PRECISION_FP32)
    check(got, ref, shape, kind)


@pytest.mark.parametrize("shape", [(65, 3, 4, 64), (33, 5, 3, 16)], ids=lambda s: "S%d-B%d-H%d-HD%d" % s)
def test_the_three_precision_codes_run_the_same_kernel(N, shape):
    R_ = case("randn", shape)
    got = [run(N, R_[0], R_[1], *shape, prec=c) for c in (N.PRECISION_FP32, N.PRECISION_BF16X3, N.PRECISION_BF16X6, N.PRECISION_DEFAULT)]
    for g, code in zip(got, ("fp32", "bf16x3", "bf16x6", "default")):
        check(g, R_, shape, code)
        assert all(np.array_equal(a, b) for a, b in zip(g, got[0])), code


@pytest.mark.parametrize("shape,p", [((129, 5, 4, 64), 0.0), ((65, 5, 8, 16), 0.0), ((65, 5, 4, 64), 0.3), ((33, 5, 3, 16), 0.3)],
                         ids=lambda s: str(s).replace(" ", ""))
def test_a_list_does_not_see_the_other_lists(N, shape, p):
    """every row of the lists != 2 in qkv and dout is NaN: list 2's rows of out, lse and dqkv are bit-identical to the clean run
    (on a batch-axis kernel they would be NaN)"""
    S, B, H, HD = shape
    qkv, dout = R.inputs("randn", *shape)
    clean = run(N, qkv, dout, *shape, p=p, seed=11)
    qn, dn = qkv.copy().reshape(S + 1, B, -1), dout.copy().reshape(S, B, -1)
    others = [b for b in range(B) if b != 2]
    qn[:, others] = np.nan
    dn[:, others] = np.nan
    dirty = run(N, qn.reshape(qkv.shape), dn.reshape(dout.shape), *shape, p=p, seed=11)
    for a, b in zip(clean, dirty):
        if a.shape[0] == B:                                   # lse (B, H, S)
            assert np.array_equal(a[2], b[2]) and not np.isnan(b[2]).any()
        else:
            a, b = a.reshape(S, B, -1)[:, 2], b.reshape(S, B, -1)[:, 2]
            assert np.array_equal(a, b) and not np.isnan(b).any()


@pytest.mark.parametrize("shape", [(2, 3, 4, 64), (17, 3, 4, 64), (65, 3, 1, 64), (2, 5, 3, 16), (17, 3, 8, 16), (65, 1, 8, 16)],
                         ids=lambda s: "S%d-B%d-H%d-HD%d" % s)
def test_dropout_against_the_restated_mask(N, shape):
    p, seed = 0.3, 0x5EED1234
    S, B, H, HD = shape
    ref = case("randn", shape, p, seed)
    got = run(N, ref[0], ref[1], *shape, p=p, seed=seed, twice=True)
    check(got, ref, shape, "dropout")
    plain = case("randn", shape)
    assert np.array_equal(got[1], run(N, ref[0], ref[1], *shape)[1])          # lse is of the undropped scores
    assert R.rel(got[0], plain[2]) > 0.05                                       # and the mask did something
    # one flipped mask entry in the restatement is seen at more than 10 x the tolerance
    mask = R.keep_mask(seed, S, B, H, p)
    b, h, i, j = B - 1, H - 1, S - 1, S // 2
    mask[b, h, i, j] = 0.0 if mask[b, h, i, j] else float(R.D.keep_scale(p))
    flipped = R.forward(ref[0][:S * B], S, B, H, HD, mask)[0]
    assert R.rel(got[0], flipped) > 10 * R.FWD_TOL
    assert R.rel(got[2], R.backward(ref[0][:S * B], ref[1], S, B, H, HD, mask)) > 10 * R.GRAD_TOL


def test_determinism_and_untouched_surroundings(N):
    """two calls give the same bits (run(twice=True)); the guards around dqkv, out and lse are intact (asserted in run) and every
    element inside them is written"""
    for shape in [(300, 3, 4, 64), (129, 3, 3, 16)]:
        ref = case("last_key", shape)
        got = run(N, ref[0], ref[1], *shape, twice=True)
        assert not any(np.isnan(g).any() for g in got)


def test_offsets_beyond_2_to_31_elements(N):
    """S*B*3E = 2.2e9 floats: the last lists' rows lie past a 32-bit element offset (and a 32-bit byte offset many times over)"""
    from rlt_hip.native import ptr
    S, B, H, HD = 2, 1_400_000, 4, 64
    E = H * HD
    if torch.cuda.mem_get_info()[0] < 40 * 2 ** 30:
        pytest.skip("needs 40 GB of free device memory")
    g = torch.Generator(device=dev()).manual_seed(5)
    qkv = torch.randn(S * B, 3 * E, device=dev(), generator=g)
    dout = torch.randn(S * B, E, device=dev(), generator=g)
    out, lse, dqkv = torch.empty(S * B, E, device=dev()), torch.empty(B, H, S, device=dev()), torch.full((S * B, 3 * E), float("nan"), device=dev())
    N.call("rlt_seq_attention_fwd", ptr(qkv), S, B, H, HD, 0.0, 0, ptr(out), ptr(lse), N.PRECISION_DEFAULT, N.stream())
    N.call("rlt_seq_attention_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, 0, ptr(dqkv), None, 0, N.PRECISION_DEFAULT, N.stream())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dqkv).any())
    lists = [0, 1, B // 2, B - 2, B - 1]
    sub = lambda t: t.view(S, B, -1)[:, lists].reshape(S * len(lists), -1).cpu().numpy()
    o_ref, l_ref, _ = R.forward(sub(qkv), S, len(lists), H, HD)
    g_ref = R.backward(sub(qkv), sub(dout), S, len(lists), H, HD)
    assert R.rel(sub(out), o_ref) < R.FWD_TOL and R.rel(sub(dqkv), g_ref) < R.GRAD_TOL
    assert np.abs(lse[lists].cpu().numpy() - l_ref).max() < 1e-5


# ------------------------------------------------------------------------------------------------ the Python layers
def test_ops_seq_attention_is_the_abi_call(N):
    from rlt_hip import ops
    shape = S, B, H, HD = (65, 3, 4, 64)
    ref = case("randn", shape)
    want = run(N, ref[0], ref[1], *shape)
    qkv = torch.from_numpy(ref[0][:S * B].copy()).to(dev()).requires_grad_(True)
    out = ops.seq_attention(qkv, S, B, H)
    out.backward(torch.from_numpy(ref[1].copy()).to(dev()))
    assert np.array_equal(out.detach().double().cpu().numpy(), want[0]) and np.array_equal(qkv.grad.double().cpu().numpy(), want[2])
    with pytest.raises(ValueError):
        ops.encoder_layer(qkv, None, S, B, H, axis="batch")


def mfma_tol(N, tol):
    return tol * (6.0 if N.get_precision() == "bf16x3" else 1.0)          # the op-level bound of the encoder tests (tools/gpu_probe.py)


def trel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("B,S,E,H", [(5, 40, 256, 4), (3, 33, 128, 8)])
def test_encoder_layer_position_axis_is_the_batch_first_layer(N, B, S, E, H):
    """forward at 2e-5 and all 13 gradients at 1e-4 (relative max-norm: the bounds of the full-size encoder checks) against the
    float64 torch layer with batch_first=True"""
    from models._common import ParamTree
    from rlt_hip import ops
    torch.manual_seed(S)
    ref = torch.nn.TransformerEncoderLayer(E, H, dim_feedforward=2048, dropout=0.0, batch_first=True).double()
    x = torch.randn(B, S, E, dtype=torch.float64, requires_grad=True)
    g = torch.randn(B, S, E, dtype=torch.float64)
    y_ref = ref(x)
    y_ref.backward(g)
    layer = ParamTree(ref).float().to(dev())
    xp = x.detach().transpose(0, 1).reshape(S * B, E).float().to(dev()).requires_grad_(True)
    y = ops.encoder_layer(xp, layer, S, B, H, axis="position")
    assert type(y.grad_fn).__name__ == "EncoderLayerSeqFnBackward"
    y.backward(g.transpose(0, 1).reshape(S * B, E).float().to(dev()))
    bm = lambda t: t.view(S, B, E).transpose(0, 1)
    assert trel(bm(y), y_ref) < mfma_tol(N, 2e-5)
    assert trel(bm(xp.grad), x.grad) < mfma_tol(N, 1e-4)
    for (name, a), (_, b) in zip(layer.named_parameters(), ref.named_parameters()):
        assert trel(a.grad, b.grad) < mfma_tol(N, 1e-4), name


def stock(name, hip, S):
    """float64 stock-torch restatement of AttnCut / Choopy with within-list attention, on the model's state_dict"""
    nn = torch.nn

    class Stock(nn.Module):
        def __init__(self):
            super().__init__()
            if name == "AttnCut":
                self.encoding_layer = nn.LSTM(3, 128, 2, batch_first=True, bidirectional=True)
                d, h, layers = 256, 4, 1
            else:
                self.position_encoding = nn.Parameter(torch.zeros(S, 127))
                d, h, layers = 128, 8, 3
            self.attention_layer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d, h, dropout=0.0, batch_first=True), layers,
                                                         enable_nested_tensor=False)
            self.decison_layer = nn.Sequential(nn.Linear(d, 1), nn.Softmax(dim=1))

        def forward(self, x):
            if name == "AttnCut":
                h = self.encoding_layer(x)[0]
            else:
                h = torch.cat((x, self.position_encoding.expand(x.shape[0], S, 127)), dim=2)
            return self.decison_layer(self.attention_layer(h))

    m = Stock()
    m.load_state_dict(hip.state_dict())
    return m.double().eval()


@pytest.mark.parametrize("name", ["AttnCut", "Choopy"])
def test_models_on_the_position_axis(N, name):
    import models as hm
    B, S = 5, 40
    torch.manual_seed(7)
    kw = {} if name == "AttnCut" else {"seq_len": S}
    pos = getattr(hm, name)(attention_axis="position", **kw).to(dev()).eval()
    lst = getattr(hm, name)(attention_axis="list", **kw)
    assert [(k, tuple(v.shape)) for k, v in pos.state_dict().items()] == [(k, tuple(v.shape)) for k, v in lst.state_dict().items()]
    lst.load_state_dict(pos.state_dict())                        # a checkpoint of one axis loads on the other, both ways
    pos.load_state_dict(lst.state_dict())
    lst = lst.to(dev()).eval()
    with pytest.raises(ValueError):
        getattr(hm, name)(attention_axis="batch", **kw)
    x = torch.randn(B, S, 3 if name == "AttnCut" else 1)
    with torch.no_grad():
        want = stock(name, pos, S)(x.double())
        got = pos(x.to(dev()))
        assert float((got.double().cpu() - want).abs().max()) < 1e-5
        # list 0 perturbed: on the position axis the other lists' outputs keep their bits, on the list axis they move
        x2 = x.clone()
        x2[0] += 0.5
        got2, l1, l2 = pos(x2.to(dev())), lst(x.to(dev())), lst(x2.to(dev()))
        assert torch.equal(got2[1:], got[1:]) and not torch.equal(got2[0], got[0])
        assert not torch.equal(l1[1:], l2[1:])


def test_run_py_records_the_axis(N, tmp_path):
    import run
    from dataloader.synth import write_synthetic_robust04
    base, hist, state = str(tmp_path / "data"), str(tmp_path / "h.json"), str(tmp_path / "state.pt")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=16, n_test=8, seed=3, seq_len=40)
    run.main(["--model-name", "attncut", "--dataset-base", base, "--use-conf", "0", "--batch-size", "8", "--seed", "1", "--epochs", "1",
              "--attention-axis", "position", "--history-json", hist, "--save-state", state, "--tensorboard-dir", "",
              "--report-out", str(tmp_path / "r.npz"), "--save-path", str(tmp_path / "best")])
    h = json.load(open(hist))
    assert h["attention_axis"] == "position" and len(h["history"]) == 1 and math.isfinite(h["history"][0]["train"][0])
    assert torch.load(state, map_location="cpu")["attention_axis"] == "position"
    assert str(np.load(str(tmp_path / "r.npz"))["attention_axis"]) == "position"
    assert run.build_parser().parse_args([]).attention_axis == "list"
