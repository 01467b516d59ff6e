"""Causal within-list attention on the device (csrc/attention_seq.hip: rlt_seq_attention_fwd_ex / _bwd_ex with RLT_SEQ_MASK_CAUSAL)
through the raw C ABI against the float64 restatement (tests/seq_causal_restate.py, pinned on the host by
tests/test_seq_causal_restate.py), and the Python layers above it.

  shapes      seq_attention_restate.SHAPES: the diagonal on every edge of the 32-key sub-tile, the 64-row staged tile and the
              128-row / 32-row pass (S = 1, 2, 31 .. 33, 63 .. 65, 127 .. 129, 300), both head dims
  inputs      randn / ramp_v (seq_causal_restate.inputs); every buffer lies between NaN guards that must be intact afterwards
  tolerances  the project's: relative max-norm 1e-5 for out, 3e-5 for each of dQ, dK, dV against its own maximum, lse within
              seq_attention_restate.lse_bound per row over the admitted keys"""
import functools
import json
import math

import numpy as np
import pytest
import torch

import seq_attention_restate as R
import seq_causal_restate as C

pytestmark = pytest.mark.gpu
GUARD = 4096          # floats of NaN on either side of a buffer
NONE, CAUSAL = 0, 1
ids = lambda s: "S%d-B%d-H%d-HD%d" % s


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


def run(N, qkv, dout, S, B, H, HD, mask=CAUSAL, p=0.0, seed=0, prec=None, twice=False, old=False):
    """forward and backward through the C ABI -> out (S*B, E), lse (B, H, S), dqkv (S*B, 3E) as float32 numpy (bits kept).
    old: the entry points without _ex (no mask argument)."""
    from rlt_hip.native import ptr
    E = H * HD
    prec = N.PRECISION_DEFAULT if prec is None else prec
    gq, gd = Guarded.of(qkv), Guarded.of(dout)
    res = []
    for _ in range(2 if twice else 1):
        go, gl, gg = Guarded(S * B * E), Guarded(B * H * S), Guarded(S * B * 3 * E)
        st = N.stream()
        if old:
            N.call("rlt_seq_attention_fwd", ptr(gq.t), S, B, H, HD, p, seed, ptr(go.t), ptr(gl.t), prec, st)
            N.call("rlt_seq_attention_bwd", ptr(gq.t), ptr(go.t), ptr(gd.t), ptr(gl.t), S, B, H, HD, p, seed, ptr(gg.t), None, 0, prec, st)
        else:
            N.call("rlt_seq_attention_fwd_ex", ptr(gq.t), S, B, H, HD, p, seed, mask, ptr(go.t), ptr(gl.t), prec, st)
            N.call("rlt_seq_attention_bwd_ex", ptr(gq.t), ptr(go.t), ptr(gd.t), ptr(gl.t), S, B, H, HD, p, seed, mask, ptr(gg.t), None, 0,
                   prec, st)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (gq, gd, go, gl, gg)), "a guard was written"
        res.append((go.t.clone(), gl.t.clone(), gg.t.clone()))
    if twice:
        assert all(torch.equal(a, b) for a, b in zip(*res)), "two calls differ"
    o, l, g = res[0]
    return o.view(S * B, E).cpu().numpy(), l.view(B, H, S).cpu().numpy(), g.view(S * B, 3 * E).cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(kind, shape, p=0.0, seed=0):
    """inputs and float64 causal reference of one id, computed once: qkv, dout, out, lse, dqkv, score_max (admitted keys)"""
    S, B, H, HD = shape
    qkv, dout = C.inputs(kind, S, B, H, HD)
    mask = C.keep_mask(seed, S, B, H, p) if p > 0 else None
    out, lse, _ = C.forward(qkv, S, B, H, HD, mask)
    dqkv = C.backward(qkv, dout, S, B, H, HD, mask)
    q, k, _ = R.heads(qkv, S, B, H, HD)
    score_max = np.where(C.causal(S), np.abs(q @ k.transpose(0, 1, 3, 2)), 0.0).max(-1) / math.sqrt(HD)
    for a in (qkv, dout, out, lse, dqkv, score_max):
        a.setflags(write=False)
    return qkv, dout, out, lse, dqkv, score_max


def check(got, ref, shape, what):
    S, B, H, HD = shape
    E = H * HD
    out, lse, dqkv = (np.asarray(a, dtype=np.float64) for a in got)
    qkv, dout, o_ref, l_ref, g_ref, score_max = ref
    errs = {"out": R.rel(out, o_ref), "dq": R.rel(dqkv[:, :E], g_ref[:, :E]), "dk": R.rel(dqkv[:, E:2 * E], g_ref[:, E:2 * E]),
            "dv": R.rel(dqkv[:, 2 * E:], g_ref[:, 2 * E:]), "lse": float((np.abs(lse - l_ref) / R.lse_bound(l_ref, score_max)).max())}
    if S == 1:
        # one key: P = 1 and dS = P (dP - delta) is the difference of two equal numbers, dQ = dK = 0 exactly: measured against the
        # size of the cancelling terms, as in tests/test_seq_attention_gpu.py
        q, k, v = R.heads(qkv, S, B, H, HD)
        dp = np.abs((R.heads(dout, S, B, H, HD)[0] * v).sum(-1, keepdims=True)) / math.sqrt(HD)
        errs["dq"] = float(np.abs(dqkv[:, :E]).max() / (dp * np.abs(k)).max())
        errs["dk"] = float(np.abs(dqkv[:, E:2 * E]).max() / (dp * np.abs(q)).max())
    print(what, shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert not np.isnan(out).any() and not np.isnan(dqkv).any() and not np.isnan(lse).any()
    assert errs["out"] < R.FWD_TOL and errs["lse"] <= 1.0, errs
    assert errs["dq"] < R.GRAD_TOL and errs["dk"] < R.GRAD_TOL and errs["dv"] < R.GRAD_TOL, errs
    return errs


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_abi_against_the_causal_restatement(N, shape, kind):
    ref = case(kind, shape)
    got = run(N, ref[0], ref[1], *shape, prec=N.PRECISION_FP32)
    check(got, ref, shape, kind)


# ------------------------------------------------------------------------------------------------ 2. row 0
@pytest.mark.parametrize("shape", [(129, 5, 4, 64), (65, 3, 8, 16), (1, 3, 3, 16)], ids=ids)
def test_row_zero_is_v_at_position_zero(N, shape):
    S, B, H, HD = shape
    E = H * HD
    qkv, dout = C.inputs("ramp_v", *shape)
    out, lse, _ = run(N, qkv, dout, *shape)
    assert np.array_equal(out[:B].view(np.uint32), qkv[:B, 2 * E:].view(np.uint32))            # every list and head, bit for bit


# ------------------------------------------------------------------------------------------------ 3. the prefix property
@pytest.mark.parametrize("shape", [(129, 3, 4, 64), (65, 3, 8, 16)], ids=ids)
def test_prefix_property_bit_for_bit(N, shape):
    """rows of positions >= j replaced by 8 x randn: out and lse of the positions < j keep their bits, the others move; with dout zero
    from position j on, dqkv is exactly 0.0 in every row >= j and the rows < j keep their bits.  Under RLT_SEQ_MASK_NONE the same
    perturbation moves the rows < j (the test sees something)."""
    S, B, H, HD = shape
    qkv, dout = C.inputs("randn", *shape)
    rng = np.random.default_rng(9)
    for j in (1, 31, 32, 33, 64, 65, S - 1):
        if j >= S:
            continue
        d0 = dout.copy()
        d0[j * B:] = 0.0
        q2 = qkv.copy()
        q2[j * B:] = (8 * rng.standard_normal(q2[j * B:].shape)).astype(np.float32)
        clean, dirty = run(N, qkv, d0, *shape), run(N, q2, d0, *shape)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert np.array_equal(bits(clean[0][:j * B]), bits(dirty[0][:j * B])), j
        assert np.array_equal(bits(clean[1][..., :j]), bits(dirty[1][..., :j])), j
        assert not np.array_equal(clean[0][j * B:], dirty[0][j * B:]) and not np.array_equal(clean[1][..., j:], dirty[1][..., j:])
        for g in (clean[2], dirty[2]):
            assert not np.isnan(g).any() and not g[j * B:].any(), j                              # exactly 0.0 from position j on
        assert np.array_equal(bits(clean[2][:j * B]), bits(dirty[2][:j * B])), j
        assert clean[2][:j * B].any()
        c0, d0_ = run(N, qkv, d0, *shape, mask=NONE), run(N, q2, d0, *shape, mask=NONE)
        assert not np.array_equal(c0[0][:j * B], d0_[0][:j * B]) and not np.array_equal(c0[2][:j * B], d0_[2][:j * B]), j


# ------------------------------------------------------------------------------------------------ 4. the old entry points
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("shape", [(65, 3, 4, 64), (33, 5, 3, 16)], ids=ids)
def test_mask_none_is_the_call_without_ex(N, shape, p):
    qkv, dout = R.inputs("randn", *shape)
    S, B = shape[:2]
    old = run(N, qkv[:S * B], dout, *shape, p=p, seed=77, old=True)
    new = run(N, qkv[:S * B], dout, *shape, mask=NONE, p=p, seed=77)
    for a, b in zip(old, new):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ref = R.forward(qkv[:S * B], *shape, R.keep_mask(77, S, B, shape[2], p) if p else None)[0]
    assert R.rel(new[0], ref) < R.FWD_TOL                                                       # and it is the unmasked attention


# ------------------------------------------------------------------------------------------------ 5. dropout
@pytest.mark.parametrize("shape", [(2, 3, 4, 64), (65, 3, 1, 64), (17, 3, 8, 16), (65, 1, 8, 16)], ids=ids)
def test_dropout_against_the_restated_mask(N, shape):
    p, seed = 0.3, 0x5EED1234
    S, B, H, HD = shape
    ref = case("randn", shape, p, seed)
    got = run(N, ref[0], ref[1], *shape, p=p, seed=seed, twice=True)
    check(got, ref, shape, "dropout")
    plain = case("randn", shape)
    assert np.array_equal(got[1], run(N, ref[0], ref[1], *shape)[1])          # lse is of the undropped admitted scores
    assert R.rel(got[0], plain[2]) > 0.05                                       # and the mask did something
    # one flipped keep entry below the diagonal is seen at more than 10 x the tolerance
    mask = C.keep_mask(seed, S, B, H, p)
    b, h, i, j = B - 1, H - 1, S - 1, S // 2
    mask[b, h, i, j] = 0.0 if mask[b, h, i, j] else float(R.D.keep_scale(p))
    assert R.rel(got[0], C.forward(ref[0], S, B, H, HD, mask)[0]) > 10 * R.FWD_TOL
    assert R.rel(got[2], C.backward(ref[0], ref[1], S, B, H, HD, mask)) > 10 * R.GRAD_TOL


# ------------------------------------------------------------------------------------------------ 6. precision, determinism
@pytest.mark.parametrize("shape", [(65, 3, 4, 64), (33, 5, 3, 16)], ids=ids)
def test_the_three_precision_codes_run_the_same_kernel(N, shape):
    ref = case("ramp_v", shape)
    got = [run(N, ref[0], ref[1], *shape, prec=c) for c in (N.PRECISION_FP32, N.PRECISION_BF16X3, N.PRECISION_BF16X6, N.PRECISION_DEFAULT)]
    for g, code in zip(got, ("fp32", "bf16x3", "bf16x6", "default")):
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(g, got[0])), code
    check(got[0], ref, shape, "codes")


def test_determinism_and_untouched_surroundings(N):
    """two calls give the same bits (run(twice=True)); the guards around every buffer are intact (asserted in run) and every element
    inside them is written"""
    for shape in [(300, 3, 4, 64), (129, 3, 3, 16)]:
        ref = case("randn", shape)
        got = run(N, ref[0], ref[1], *shape, twice=True)
        assert not any(np.isnan(g).any() for g in got)
        got = run(N, ref[0], ref[1], *shape, p=0.3, seed=5, twice=True)
        assert not any(np.isnan(g).any() for g in got)


# ------------------------------------------------------------------------------------------------ 7. the Python layers
def test_ops_seq_attention_causal_is_the_abi_call(N):
    from rlt_hip import ops
    shape = S, B, H, HD = (65, 3, 4, 64)
    ref = case("randn", shape)
    want = run(N, ref[0], ref[1], *shape)
    qkv = torch.from_numpy(ref[0].copy()).to(dev()).requires_grad_(True)
    out = ops.seq_attention(qkv, S, B, H, causal=True)
    out.backward(torch.from_numpy(ref[1].copy()).to(dev()))
    assert np.array_equal(out.detach().cpu().numpy(), want[0]) and np.array_equal(qkv.grad.cpu().numpy(), want[2])
    plain = ops.seq_attention(qkv.detach(), S, B, H)
    assert not torch.equal(plain, out.detach())
    with pytest.raises(ValueError):
        ops.encoder_layer(qkv, None, S, B, H, axis="list", causal=True)


def mfma_tol(N, tol):
    return tol * (6.0 if N.get_precision() == "bf16x3" else 1.0)          # the op-level bound of the encoder tests


def trel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def banned(S):
    return torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)


@pytest.mark.parametrize("B,S,E,H", [(5, 40, 256, 4), (3, 33, 128, 8)])
def test_encoder_layer_causal_is_the_batch_first_layer_with_src_mask(N, B, S, E, H):
    """forward at 2e-5 and all 13 gradients at 1e-4 (the bounds of test_encoder_layer_position_axis_is_the_batch_first_layer) against
    the float64 torch layer called with the upper-triangular src_mask"""
    from models._common import ParamTree
    from rlt_hip import ops
    torch.manual_seed(S)
    ref = torch.nn.TransformerEncoderLayer(E, H, dim_feedforward=2048, dropout=0.0, batch_first=True).double()
    x = torch.randn(B, S, E, dtype=torch.float64, requires_grad=True)
    g = torch.randn(B, S, E, dtype=torch.float64)
    y_ref = ref(x, src_mask=banned(S))
    y_ref.backward(g)
    layer = ParamTree(ref).float().to(dev())
    xp = x.detach().transpose(0, 1).reshape(S * B, E).float().to(dev()).requires_grad_(True)
    y = ops.encoder_layer(xp, layer, S, B, H, axis="position", causal=True)
    assert type(y.grad_fn).__name__ == "EncoderLayerSeqCausalFnBackward"
    y.backward(g.transpose(0, 1).reshape(S * B, E).float().to(dev()))
    bm = lambda t: t.view(S, B, E).transpose(0, 1)
    assert trel(bm(y), y_ref) < mfma_tol(N, 2e-5)
    assert trel(bm(xp.grad), x.grad) < mfma_tol(N, 1e-4)
    for (name, a), (_, b) in zip(layer.named_parameters(), ref.named_parameters()):
        assert trel(a.grad, b.grad) < mfma_tol(N, 1e-4), name
    assert trel(bm(y), ref(x).detach()) > 1e-2                               # and the mask is not a detail


# ------------------------------------------------------------------------------------------------ 8. models
def stock(name, hip, S):
    """float64 stock-torch restatement of AttnCut / Choopy with causal within-list attention, on the model's state_dict"""
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

        def encode(self, x):
            if name == "AttnCut":
                h = self.encoding_layer(x)[0]
            else:
                h = torch.cat((x, self.position_encoding.expand(x.shape[0], S, 127)), dim=2)
            return self.attention_layer(h, mask=banned(S))

        def forward(self, x):
            return self.decison_layer(self.encode(x))

    m = Stock()
    m.load_state_dict(hip.state_dict())
    return m.double().eval()


@pytest.mark.parametrize("name", ["AttnCut", "Choopy"])
def test_models_under_the_causal_mask(N, name):
    import models as hm
    B, S = 5, 40
    torch.manual_seed(7)
    kw = {} if name == "AttnCut" else {"seq_len": S}
    cau = getattr(hm, name)(attention_axis="position", attention_mask="causal", **kw).to(dev()).eval()
    full = getattr(hm, name)(attention_axis="position", **kw)
    assert cau.attention_mask == "causal" and full.attention_mask == "none"
    assert [(k, tuple(v.shape)) for k, v in cau.state_dict().items()] == [(k, tuple(v.shape)) for k, v in full.state_dict().items()]
    full.load_state_dict(cau.state_dict())                       # weights load across the masks, both ways
    cau.load_state_dict(full.state_dict())
    full = full.to(dev()).eval()
    x = torch.randn(B, S, 3 if name == "AttnCut" else 1)
    with torch.no_grad():
        want = stock(name, cau, S)(x.double())
        got = cau(x.to(dev()))
        assert float((got.double().cpu() - want).abs().max()) < 1e-5
        assert not torch.equal(full(x.to(dev())), got)


def test_mask_argument_errors(N):
    import models as hm
    from models import _common as MC
    for name in ("AttnCut", "Choopy", "MtAttnCut", "MtChoopy", "MMOECut", "MOECut", "PLECut", "ProbeBase"):
        cls = getattr(hm, name)
        with pytest.raises(ValueError):
            cls(attention_axis="list", attention_mask="causal")
        with pytest.raises(ValueError):
            cls(attention_mask="causal")                                      # the default axis is 'list'
        with pytest.raises(ValueError):
            cls(attention_axis="position", attention_mask="prefix")
        with pytest.raises(ValueError):
            cls(attention_axis="batch", attention_mask="none")
        assert cls(attention_axis="position", attention_mask="causal").attention_mask == "causal"
        assert cls().attention_mask == "none"
    with pytest.raises(ValueError):
        MC.encoder(torch.zeros(4, 8), None, 1, 2, 2, axis="list", causal=True)


def test_choopy_encoder_output_is_prefix_only(N):
    """the encoder output on the model's own input keeps its bits at the positions < 20 when the scores from position 20 on are
    perturbed (three causal layers; everything else of a layer is per row) - without the mask it moves"""
    import models as hm
    from models import _common as MC
    from rlt_hip import ops
    B, S, J = 5, 40, 20
    torch.manual_seed(11)
    m = hm.Choopy(seq_len=S, attention_axis="position", attention_mask="causal").to(dev()).eval()
    x = torch.randn(B, S, 1, device=dev())
    x2 = x.clone()
    x2[:, J:] += torch.randn(B, S - J, 1, device=dev())

    def enc(inp, causal):
        with torch.no_grad():
            return MC.encoder(ops.choopy_embed(inp, m.position_encoding), m.attention_layer, m.n_head, S, B, 0.0, "position", causal)
    a, b = enc(x, True).view(S, B, -1), enc(x2, True).view(S, B, -1)
    assert torch.equal(a[:J], b[:J]) and not torch.equal(a[J:], b[J:])
    a, b = enc(x, False).view(S, B, -1), enc(x2, False).view(S, B, -1)
    assert not torch.equal(a[:J], b[:J])


# ------------------------------------------------------------------------------------------------ 9. run.py
def test_run_py_records_the_mask(N, tmp_path):
    import run
    from dataloader.synth import write_synthetic_robust04
    base, hist, state = str(tmp_path / "data"), str(tmp_path / "h.json"), str(tmp_path / "state.pt")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=16, n_test=8, seed=3, seq_len=40)
    common = ["--model-name", "choopy", "--dataset-base", base, "--use-conf", "0", "--batch-size", "8", "--seed", "1", "--epochs", "1",
              "--tensorboard-dir", ""]
    run.main(common + ["--attention-axis", "position", "--attention-mask", "causal", "--history-json", hist, "--save-state", state,
                       "--model-persist", "1", "--report-out", str(tmp_path / "r.npz"), "--save-path", str(tmp_path / "best")])
    h = json.load(open(hist))
    assert h["attention_axis"] == "position" and h["attention_mask"] == "causal"
    assert len(h["history"]) == 1 and math.isfinite(h["history"][0]["train"][0])
    st = torch.load(state, map_location="cpu")
    assert st["attention_axis"] == "position" and st["attention_mask"] == "causal"
    rep = np.load(str(tmp_path / "r.npz"))
    assert str(rep["attention_axis"]) == "position" and str(rep["attention_mask"]) == "causal"
    meta = json.load(open(str(tmp_path / "best" / "choopy.pkl.meta.json")))
    assert meta == {"attention_axis": "position", "attention_mask": "causal"}
    args = run.build_parser().parse_args([])
    assert args.attention_mask == "none" and args.attention_axis == "list"
    with pytest.raises(SystemExit) as e:                                      # an argument error, before any data is read
        run.main(["--model-name", "choopy", "--dataset-base", str(tmp_path / "nowhere"), "--attention-axis", "list",
                  "--attention-mask", "causal"])
    assert e.value.code == 2
