"""torch.autograd.Function wrappers around the C ABI (include/rlt_hip.h).

PyTorch here is plumbing: it owns device buffers, the stream and the autograd tape.  Every
arithmetic step of the hot path - forward AND backward - is a call into librlt_hip.so.
Activations are "position-major": a (S*B, E) matrix whose row index is s*B + b.
"""
import contextvars
import math

import torch
from torch.autograd import Function

from . import native as N
from .native import call, ptr, query, stream, workspace


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


class KernelTimer:
    """Optional HIP-event timing of named launches on the current stream (bench.py's live roofline
    measurement).  Disabled unless `KernelTimer.active` is set to an instance."""
    active = None

    def __init__(self):
        self.events = {}

    def reset(self):
        self.events = {}

    def timed(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        self.events.setdefault(name, []).append((a, b))

    def summary(self):
        """name -> (launches, mean milliseconds); call after torch.cuda.synchronize()."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.events.items()}


_SEED_COUNTER = [0]
_SEED_STREAM = [0]
KERNEL_LEVEL_ENCODER = [False]      # tests: run the encoder layer launch by launch from the host (EncoderLayerKernelsFn)


def set_seed_stream(stream_id):
    """Data-parallel runs: every rank has the same torch seed (identical initial weights) but must draw its own
    dropout masks - the rank is mixed into the seed as a stream id."""
    _SEED_STREAM[0] = int(stream_id)


def next_seed():
    """A fresh 32-bit dropout seed: a function of torch's seed, the stream id (rank) and a call counter, so that
    torch.manual_seed(...) makes a training run reproducible."""
    _SEED_COUNTER[0] += 1
    x = (torch.initial_seed() * 0x9E3779B97F4A7C15 + _SEED_COUNTER[0] * 0xD1B54A32D192ED03
         + _SEED_STREAM[0] * 0xA24BAED4963EE407) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 29
    return int((x * 0xBF58476D1CE4E5B9 >> 32) & 0xFFFFFFFF)


# the scope is a context variable: per thread (autograd runs backward nodes on its own threads) and per asyncio task, like the
# thread-local scope of the library's own entry points (include/rlt_hip.h)
_CALL_PRECISION = contextvars.ContextVar("rlt_call_precision", default=N.PRECISION_DEFAULT)


class precision:
    """`with ops.precision('fp32'):` - every library call issued inside (the forward of the modules called there) runs in
    that mode, whatever the process default (native.set_precision) is; each tape node remembers the mode of its forward and
    gives it to its backward (the stash layout depends on it).  Re-entrant: nested scopes restore the outer one; scopes of
    different threads do not see each other."""

    def __init__(self, mode):
        self.code = N.PRECISION_DEFAULT if mode is None else N.precision_code(mode)
        self._tokens = []

    def __enter__(self):
        self._tokens.append(_CALL_PRECISION.set(self.code))
        return self

    def __exit__(self, *exc):
        _CALL_PRECISION.reset(self._tokens.pop())
        return False


def current_precision():
    """The RLT_PRECISION_* code a forward issued now runs in: the enclosing `precision(...)` scope's, else the process
    default read once, so that forward and backward of a tape node agree even if the default is changed in between."""
    c = _CALL_PRECISION.get()
    return c if c >= 0 else int(N.load().rlt_get_precision())


def _launch(name, fn):
    t = KernelTimer.active
    if t is None:
        fn()
    else:
        t.timed(name, fn)


# ------------------------------------------------------------------------------ raw helpers
def gemm(ta, tb, M, Nn, K, A, lda, B, ldb, C, ldc, bias=None, bias2=None, flags=0, a_off=0, b_off=0, c_off=0,
         relu_mask=None, ldmask=0, colsum_a=None, mask_scale=1.0, drop_p=0.0, seed=0, prec=None):
    """C[M,N] (+)= op(A) op(B) (+bias); *_off are element offsets into the tensors.
    relu_mask: C = mask > 0 ? C*mask_scale : 0 (fused ReLU/dropout backward); colsum_a (M): row sums of
    op(A) (ta=1 only); drop_p/seed: dropout on the output."""
    ws_bytes = query("rlt_gemm_workspace", ta, tb, M, Nn, K)
    ws = workspace(ws_bytes, C.device) if ws_bytes else None
    esz = 4
    call("rlt_gemm_ex", ta, tb, M, Nn, K,
         N.c_void_p(A.data_ptr() + a_off * esz), lda, N.c_void_p(B.data_ptr() + b_off * esz), ldb,
         N.c_void_p(C.data_ptr() + c_off * esz), ldc, ptr(bias), ptr(bias2), flags,
         ptr(relu_mask), ldmask, mask_scale, ptr(colsum_a), drop_p, seed, ptr(ws), ws_bytes,
         current_precision() if prec is None else prec, stream())


def gemm_bits(ta, tb, M, Nn, K, A, lda, B, ldb, C, ldc, bias=None, flags=0, bits_out=None, bits_in=None, mask_scale=1.0,
              drop_p=0.0, seed=0, prec=None):
    """rlt_gemm_bits: ReLU (+ dropout) forward that also emits a 1-bit mask of the surviving elements (bits_out,
    int32 (ceil(M/32), N): `alloc_relu_bits(M, N, device)`), or the masked backward product that consumes it (bits_in,
    mask_scale = 1/(1-p))."""
    call("rlt_gemm_bits", ta, tb, M, Nn, K, ptr(A), lda, ptr(B), ldb, ptr(C), ldc, ptr(bias), flags, drop_p, seed,
         ptr(bits_out), ptr(bits_in), mask_scale, current_precision() if prec is None else prec, stream())


def alloc_relu_bits(M, Nn, device):
    """Buffer for the 1-bit mask of rlt_gemm_bits: packed along rows, bit (row & 31) of word [(row >> 5), col]."""
    return torch.zeros(((M + 31) // 32, Nn), dtype=torch.int32, device=device)


def unpack_relu_bits(bits, M):
    """(ceil(M/32), N) int32 -> (M, N) bool (tests)."""
    sh = torch.arange(32, dtype=torch.int32, device=bits.device).view(1, 32, 1)
    return (((bits.unsqueeze(1) >> sh) & 1).reshape(-1, bits.shape[1])[:M]).bool()


def colsum(X, ldx, T, Nn, out, accumulate=0, x_off=0):
    ws_bytes = query("rlt_colsum_workspace", T, Nn)
    ws = workspace(ws_bytes, X.device)
    call("rlt_colsum", N.c_void_p(X.data_ptr() + 4 * x_off), ldx, T, Nn, ptr(out), accumulate, ptr(ws), ws_bytes, stream())


# ------------------------------------------------------------------------------ Linear
class LinearFn(Function):
    """y = x W^T + b (optional fused ReLU).  x (T,K), W (N,K), b (N)."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        T, K = x.shape
        Nn = w.shape[0]
        y = _empty((T, Nn), x)
        ctx.prec = current_precision()
        gemm(0, 1, T, Nn, K, x, K, w, K, y, Nn, bias=b, flags=N.GEMM_RELU if relu else 0, prec=ctx.prec)
        ctx.relu = relu
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        T, K = x.shape
        Nn = w.shape[0]
        dy = N.f32c(dy)
        if ctx.relu:
            dy = dy.clone()
            call("rlt_relu_bwd", ptr(dy), ptr(y), dy.numel(), stream())
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _empty((T, K), x)
            gemm(0, 0, T, K, Nn, dy, Nn, w, K, dx, K, prec=ctx.prec)
        if ctx.needs_input_grad[1]:
            dw = _empty((Nn, K), x)
            db = _empty((Nn,), x) if ctx.needs_input_grad[2] else None
            gemm(1, 0, Nn, K, T, dy, Nn, x, K, dw, K, colsum_a=db, prec=ctx.prec)      # db rides on the dW product
        elif ctx.needs_input_grad[2]:
            db = _empty((Nn,), x)
            colsum(dy, Nn, T, Nn, db)
        return dx, dw, db, None


def linear(x, w, b, relu=False):
    return LinearFn.apply(x, w, b, relu)


class FFNFn(Function):
    """y = relu(x W1^T + b1) W2^T + b2 (the encoder layer's feed-forward block) as one tape node:
    backward fuses the ReLU mask into the dH product and the bias gradients into the dW products."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, drop_p=0.0, seed=0):
        T, E = x.shape
        Fh = w1.shape[0]
        h = _empty((T, Fh), x)          # relu output, already dropped when drop_p > 0
        ctx.prec = pr = current_precision()
        gemm(0, 1, T, Fh, E, x, E, w1, E, h, Fh, bias=b1, flags=N.GEMM_RELU, drop_p=drop_p, seed=seed, prec=pr)
        y = _empty((T, w2.shape[0]), x)
        gemm(0, 1, T, w2.shape[0], Fh, h, Fh, w2, Fh, y, w2.shape[0], bias=b2, prec=pr)
        ctx.save_for_backward(x, w1, w2, h)
        ctx.drop_p = drop_p
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, h = ctx.saved_tensors
        T, E = x.shape
        Fh, Eo = w1.shape[0], w2.shape[0]
        dy = N.f32c(dy)
        pr = ctx.prec
        dw2, db2 = _empty((Eo, Fh), x), _empty((Eo,), x)
        gemm(1, 0, Eo, Fh, T, dy, Eo, h, Fh, dw2, Fh, colsum_a=db2, prec=pr)
        dh = _empty((T, Fh), x)
        # dH = (dY W2) * (H > 0) [/ (1-p)]: a dropped element has H == 0, so one mask covers ReLU and dropout
        gemm(0, 0, T, Fh, Eo, dy, Eo, w2, Fh, dh, Fh, relu_mask=h, ldmask=Fh, mask_scale=1.0 / (1.0 - ctx.drop_p), prec=pr)
        dw1, db1 = _empty((Fh, E), x), _empty((Fh,), x)
        gemm(1, 0, Fh, E, T, dh, Fh, x, E, dw1, E, colsum_a=db1, prec=pr)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty((T, E), x)
            gemm(0, 0, T, E, Fh, dh, Fh, w1, E, dx, E, prec=pr)
        return dx, dw1, db1, dw2, db2, None, None


def ffn(x, w1, b1, w2, b2, drop_p=0.0):
    return FFNFn.apply(x, w1, b1, w2, b2, drop_p, next_seed() if drop_p > 0 else 0)


# ------------------------------------------------------------------------------ residual + LayerNorm
class AddLayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps, drop_p=0.0, seed=0):
        T, E = x.shape
        y = _empty((T, E), x)
        stats = _empty((T, 2), x)
        call("rlt_add_layernorm_fwd", ptr(x), ptr(r), ptr(gamma), ptr(beta), T, E, eps, drop_p, seed,
             ptr(y), ptr(stats), stream())
        ctx.save_for_backward(x, r, gamma, stats)
        ctx.drop = (drop_p, seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, r, gamma, stats = ctx.saved_tensors
        T, E = x.shape
        dy = N.f32c(dy)
        drop_p, seed = ctx.drop
        dz = _empty((T, E), x)
        dr = _empty((T, E), x) if drop_p > 0 else None
        dgamma, dbeta = _empty((E,), x), _empty((E,), x)
        ws_bytes = query("rlt_add_layernorm_bwd_workspace", T, E)
        ws = workspace(ws_bytes, x.device)
        call("rlt_add_layernorm_bwd", ptr(x), ptr(r), ptr(gamma), ptr(stats), ptr(dy), T, E, drop_p, seed,
             ptr(dz), ptr(dr), ptr(dgamma), ptr(dbeta), 0, ptr(ws), ws_bytes, stream())
        return dz, (dz if dr is None else dr), dgamma, dbeta, None, None, None


def add_layernorm(x, r, gamma, beta, eps=1e-5, drop_p=0.0):
    """LayerNorm(x + dropout(r)) * gamma + beta."""
    return AddLayerNormFn.apply(x, r, gamma, beta, eps, drop_p, next_seed() if drop_p > 0 else 0)


# ------------------------------------------------------------------------------ list-axis attention
def _list_attention_fwd(qkv, S, B, H, HD, drop_p, seed, pr):
    """-> (out (S*B, E), lse (S,H,B), the images the backward reads or None)."""
    out = _empty((S * B, qkv.shape[1] // 3), qkv)
    lse = _empty((S, H, B), qkv)
    img_bytes = query("rlt_list_attention_fwd_workspace", S, B, H, HD, drop_p, pr)
    images = workspace(img_bytes, qkv.device) if img_bytes else None     # pre-split tile records / images of this call
    _launch("attn_fwd", lambda: call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, drop_p, seed,
                                     ptr(out), ptr(lse), ptr(images), img_bytes, pr, stream()))
    # kept for the backward only where it reads them (split-bf16 records); the images of the pipelined bf16x6 forward kernels
    # are scratch of the call above - several GB per layer at the benchmark sizes
    if images is not None and not N.load().rlt_list_attention_images_retained(S, B, H, HD, pr):
        images = None
    return out, lse, images


def _list_attention_bwd(qkv, out, dout, lse, images, S, B, H, HD, drop_p, seed, pr):
    dqkv = torch.empty_like(qkv)
    ws_bytes = query("rlt_list_attention_bwd_workspace", S, B, H, HD, drop_p, pr)
    ws = workspace(ws_bytes, qkv.device)
    call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, drop_p, ptr(images), ptr(ws), ws_bytes, pr, stream())
    _launch("attn_bwd_dkv", lambda: call("rlt_list_attention_bwd_dkv", ptr(qkv), ptr(dout), ptr(lse), ptr(images), ptr(ws), ws_bytes,
                                         S, B, H, HD, drop_p, seed, ptr(dqkv), pr, stream()))
    _launch("attn_bwd_dq", lambda: call("rlt_list_attention_bwd_dq", ptr(qkv), ptr(dout), ptr(lse), ptr(images), ptr(ws), ws_bytes,
                                        S, B, H, HD, drop_p, seed, ptr(dqkv), pr, stream()))
    return dqkv


class ListAttentionFn(Function):
    """qkv (S*B, 3E) -> concatenated heads (S*B, E); attention over the B lists at each position."""

    @staticmethod
    def forward(ctx, qkv, S, B, H, drop_p=0.0, seed=0):
        HD = qkv.shape[1] // 3 // H
        ctx.prec = pr = current_precision()
        out, lse, ctx.images = _list_attention_fwd(qkv, S, B, H, HD, drop_p, seed, pr)
        ctx.dims = (S, B, H, HD)
        ctx.drop = (drop_p, seed)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        S, B, H, HD = ctx.dims
        drop_p, seed = ctx.drop
        dqkv = _list_attention_bwd(qkv, out, N.f32c(dout), lse, ctx.images, S, B, H, HD, drop_p, seed, ctx.prec)
        ctx.images = None
        return dqkv, None, None, None, None, None


def list_attention(qkv, S, B, H, drop_p=0.0):
    return ListAttentionFn.apply(qkv, S, B, H, drop_p, next_seed() if drop_p > 0 else 0)


# ------------------------------------------------------------------------------ within-list ("position-axis") attention
def _seq_attention_fwd(qkv, S, B, H, HD, drop_p, seed, pr, causal=False):
    out = _empty((S * B, H * HD), qkv)
    lse = _empty((B, H, S), qkv)
    if causal:
        _launch("seq_attn_fwd", lambda: call("rlt_seq_attention_fwd_ex", ptr(qkv), S, B, H, HD, drop_p, seed, N.SEQ_MASK_CAUSAL,
                                             ptr(out), ptr(lse), pr, stream()))
    else:
        _launch("seq_attn_fwd", lambda: call("rlt_seq_attention_fwd", ptr(qkv), S, B, H, HD, drop_p, seed, ptr(out), ptr(lse), pr, stream()))
    return out, lse


def _seq_attention_bwd(qkv, out, dout, lse, S, B, H, HD, drop_p, seed, pr, causal=False):
    dqkv = torch.empty_like(qkv)
    ws_bytes = query("rlt_seq_attention_bwd_workspace", S, B, H, HD, drop_p, pr)
    ws = workspace(ws_bytes, qkv.device) if ws_bytes else None
    if causal:
        _launch("seq_attn_bwd", lambda: call("rlt_seq_attention_bwd_ex", ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, drop_p, seed,
                                             N.SEQ_MASK_CAUSAL, ptr(dqkv), ptr(ws), ws_bytes, pr, stream()))
    else:
        _launch("seq_attn_bwd", lambda: call("rlt_seq_attention_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, drop_p, seed,
                                             ptr(dqkv), ptr(ws), ws_bytes, pr, stream()))
    return dqkv


class SeqAttentionFn(Function):
    """qkv (S*B, 3E) -> concatenated heads (S*B, E); every list attends over its own S positions (rlt_seq_attention_*: one
    launch forward, one launch backward).  causal: position i attends to the positions <= i only (RLT_SEQ_MASK_CAUSAL)."""

    @staticmethod
    def forward(ctx, qkv, S, B, H, drop_p=0.0, seed=0, causal=False):
        E = qkv.shape[1] // 3
        if qkv.shape != (S * B, 3 * E) or E % H:
            raise RuntimeError(f"seq_attention: qkv {tuple(qkv.shape)} does not match S*B = {S * B} rows of 3 * H * HD columns")
        HD = E // H
        ctx.prec = pr = current_precision()
        ctx.causal = bool(causal)
        out, lse = _seq_attention_fwd(qkv, S, B, H, HD, drop_p, seed, pr, ctx.causal)
        ctx.dims = (S, B, H, HD)
        ctx.drop = (drop_p, seed)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        S, B, H, HD = ctx.dims
        drop_p, seed = ctx.drop
        dqkv = _seq_attention_bwd(qkv, out, N.f32c(dout), lse, S, B, H, HD, drop_p, seed, ctx.prec, ctx.causal)
        return dqkv, None, None, None, None, None, None


def seq_attention(qkv, S, B, H, drop_p=0.0, causal=False):
    N.require_cuda(qkv)
    return SeqAttentionFn.apply(N.f32c(qkv), S, B, H, drop_p, next_seed() if drop_p > 0 else 0, causal)


def _check_active(active, B, like, what):
    if active is None:
        return
    if active.dtype != torch.int32 or active.shape != (B,) or not active.is_contiguous() or active.device != like.device:
        raise ValueError(f"{what}: active must be a contiguous int32 tensor of shape ({B},) on {like.device}")


def seq_attention_append(qkv_chunk, cache, t0, C, Smax, B, H, active=None, want_lse=False):
    """Streaming (inference only, no tape): the causal within-list attention of the C new ranks t0 .. t0+C-1 over a K/V cache
    (rlt_seq_attention_append).  qkv_chunk (C*B, 3E) position-major, cache (Smax*B, 2E) fp32 - written in place at rows
    t0 .. t0+C-1, read below t0 -, active (B,) int32 or None.  -> out (C*B, E), or (out, lse (B,H,C)) with want_lse.  The rows of a
    retired list (active[b] == 0) are not written: out is zero there when `active` is given, lse is not initialised."""
    N.require_cuda(qkv_chunk)
    E = qkv_chunk.shape[1] // 3
    if qkv_chunk.dtype != torch.float32 or not qkv_chunk.is_contiguous() or qkv_chunk.shape != (C * B, 3 * E) or E % H:
        raise ValueError(f"seq_attention_append: qkv_chunk {tuple(qkv_chunk.shape)} is not C*B = {C * B} contiguous fp32 rows of 3 * H * HD columns")
    if cache.dtype != torch.float32 or not cache.is_contiguous() or cache.shape != (Smax * B, 2 * E) or cache.device != qkv_chunk.device:
        raise ValueError(f"seq_attention_append: the cache must be a contiguous fp32 ({Smax * B}, {2 * E}) tensor on {qkv_chunk.device}, got {tuple(cache.shape)}")
    if t0 < 0 or C < 1 or t0 + C > Smax:
        raise ValueError(f"seq_attention_append: ranks {t0} .. {t0 + C - 1} do not lie inside a list of {Smax}")
    _check_active(active, B, qkv_chunk, "seq_attention_append")
    out = _empty((C * B, E), qkv_chunk) if active is None else torch.zeros((C * B, E), dtype=torch.float32, device=qkv_chunk.device)
    lse = _empty((B, H, C), qkv_chunk) if want_lse else None
    _launch("seq_attn_append", lambda: call("rlt_seq_attention_append", ptr(qkv_chunk), ptr(cache), t0, C, Smax, B, H, E // H, ptr(active),
                                            ptr(out), ptr(lse), current_precision(), stream()))
    return (out, lse) if want_lse else out


def encoder_layer_append(x_chunk, layer, cache, t0, Smax, B, H, active=None, eps=1e-5):
    """Streaming (inference only): the eval-mode encoder layer of EncoderLayerKernelsFn._forward on the C*B rows of a chunk of
    ranks t0 .. t0+C-1, with rlt_seq_attention_append over the layer's K/V `cache` (Smax*B, 2E) in the attention slot: in_proj,
    attention, out_proj, residual + LayerNorm, the FFN pair, residual + LayerNorm.  Nothing is stashed (no 1-bit ReLU mask, no
    tape).  The GEMMs and LayerNorms run over ALL C*B rows; only the attention skips the lists `active` retires.  -> (C*B, E)."""
    T, E = x_chunk.shape
    if T % B:
        raise ValueError(f"encoder_layer_append: {T} rows are not a whole number of ranks of {B} lists")
    C = T // B
    att_p = layer.self_attn
    w1, w2 = layer.linear1.weight, layer.linear2.weight
    Fh = w1.shape[0]
    with torch.no_grad():
        x = N.f32c(x_chunk)
        qkv = _empty((T, 3 * E), x)
        gemm(0, 1, T, 3 * E, E, x, E, att_p.in_proj_weight, E, qkv, 3 * E, bias=att_p.in_proj_bias)
        att = seq_attention_append(qkv, cache, t0, C, Smax, B, H, active)
        proj = _empty((T, E), x)
        gemm(0, 1, T, E, E, att, E, att_p.out_proj.weight, E, proj, E, bias=att_p.out_proj.bias)
        h1, st = _empty((T, E), x), _empty((T, 2), x)
        call("rlt_add_layernorm_fwd", ptr(x), ptr(proj), ptr(layer.norm1.weight), ptr(layer.norm1.bias), T, E, eps, 0.0, 0, ptr(h1), ptr(st), stream())
        hid = _empty((T, Fh), x)
        gemm(0, 1, T, Fh, E, h1, E, w1, E, hid, Fh, bias=layer.linear1.bias, flags=N.GEMM_RELU)
        ff = _empty((T, E), x)
        gemm(0, 1, T, E, Fh, hid, Fh, w2, Fh, ff, E, bias=layer.linear2.bias)
        y = _empty((T, E), x)
        call("rlt_add_layernorm_fwd", ptr(h1), ptr(ff), ptr(layer.norm2.weight), ptr(layer.norm2.bias), T, E, eps, 0.0, 0, ptr(y), ptr(st), stream())
    return y


# ------------------------------------------------------------------------------ whole encoder layer
class EncoderLayerFn(Function):
    """One post-norm nn.TransformerEncoderLayer (list-axis attention, ReLU FFN) as ONE tape node on the path-level
    entry points rlt_encoder_layer_fwd / _bwd: the launch sequence (in_proj, attention, out_proj, residual+LayerNorm,
    the FFN pair with its 1-bit ReLU mask, residual+LayerNorm), the stash layout and the in-place accumulation of the
    two fan-out gradients live in the library (csrc/path.hip); here: buffers and the tape."""

    @staticmethod
    def forward(ctx, x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, S, B, H, eps, drop_p, seeds):
        T, E = x.shape
        FF = w1.shape[0]
        if T != S * B or in_w.shape != (3 * E, E) or w2.shape != (E, FF):
            raise RuntimeError(f"encoder layer: x {tuple(x.shape)} does not match S*B = {S * B} / the layer's weights")
        weights = (in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b)
        pr = current_precision()
        stash_bytes = query("rlt_workspace_bytes", N.OP_ENCODER_STASH, S, B, E, H, FF, 0, pr)
        ws_bytes = query("rlt_workspace_bytes", N.OP_ENCODER_FWD_WS, S, B, E, H, FF, 1 if drop_p > 0 else 0, pr)
        stash = N.byte_buffer(stash_bytes, x.device)
        ws = N.byte_buffer(ws_bytes, x.device)
        y = _empty((T, E), x)
        sarr = (N.c_uint32 * 4)(*seeds)
        wp = N.encoder_ptrs(weights)
        _launch("encoder_fwd", lambda: call("rlt_encoder_layer_fwd", ptr(x), N.ctypes.byref(wp), S, B, E, H, FF, eps, drop_p, sarr,
                                            ptr(y), ptr(stash), stash_bytes, ptr(ws), ws_bytes, pr, stream()))
        ctx.cfg = (S, B, E, H, FF, eps, drop_p, tuple(seeds), stash_bytes, pr)
        ctx.stash = stash
        ctx.save_for_backward(x, *weights)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, *weights = ctx.saved_tensors
        S, B, E, H, FF, eps, drop_p, seeds, stash_bytes, pr = ctx.cfg
        if ctx.stash is None:
            raise RuntimeError("EncoderLayerFn.backward frees its stash and can run only once")
        dy = N.f32c(dy)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(w) for w in weights]
        ws_bytes = query("rlt_workspace_bytes", N.OP_ENCODER_BWD_WS, S, B, E, H, FF, 1 if drop_p > 0 else 0, pr)
        ws = N.byte_buffer(ws_bytes, x.device)
        sarr = (N.c_uint32 * 4)(*seeds)
        wp, gp = N.encoder_ptrs(weights), N.encoder_ptrs(grads)
        _launch("encoder_bwd", lambda: call("rlt_encoder_layer_bwd", ptr(x), N.ctypes.byref(wp), S, B, E, H, FF, eps, drop_p, sarr,
                                            ptr(dy), ptr(ctx.stash), stash_bytes, ptr(dx), N.ctypes.byref(gp),
                                            ptr(ws), ws_bytes, pr, stream()))
        ctx.stash = None
        return (dx, *grads, None, None, None, None, None, None)


class EncoderLayerKernelsFn(Function):
    """The encoder layer composed from the KERNEL-level entry points, launch by launch, on the host: the same launches
    in the same order as rlt_encoder_layer_fwd / _bwd (csrc/path.hip) make inside the library.  Not the product path -
    it exists so that bench.py can bracket the three attention launches of a REAL training step with HIP events
    (`KernelTimer.active`), and as a cross-check of the path-level composition in the tests.

    Same kernels as LinearFn / ListAttentionFn / AddLayerNormFn / FFNFn chained by hand; what the single node buys is
    the two fan-out points of the layer (x feeds in_proj and the first residual; LN1's output feeds the FFN and the
    second residual): the dX products of in_proj and linear1 accumulate straight into the residual gradient
    (RLT_GEMM_ACCUMULATE) instead of autograd materialising both and adding them in a separate pass (two 1.26 GB
    adds per layer at B=4096)."""

    @staticmethod
    def forward(ctx, *args):
        ctx.prec = current_precision()
        ctx.axis, ctx.causal = "list", False
        with precision(ctx.prec):          # every gemm() below reads the scope
            return EncoderLayerKernelsFn._forward(ctx, *args)

    @staticmethod
    def backward(ctx, dy):
        with precision(ctx.prec):
            return EncoderLayerKernelsFn._backward(ctx, dy)

    @staticmethod
    def _forward(ctx, x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, S, B, H, eps, drop_p, seeds):
        T, E = x.shape
        HD = E // H
        Fh = w1.shape[0]
        pr = ctx.prec
        s_attn, s_ln1, s_ffn, s_ln2 = seeds
        qkv = _empty((T, 3 * E), x)
        gemm(0, 1, T, 3 * E, E, x, E, in_w, E, qkv, 3 * E, bias=in_b)
        images = None
        if ctx.axis == "position":
            att, lse = _seq_attention_fwd(qkv, S, B, H, HD, drop_p, s_attn, pr, ctx.causal)
        else:
            att, lse, images = _list_attention_fwd(qkv, S, B, H, HD, drop_p, s_attn, pr)
        proj = _empty((T, E), x)
        gemm(0, 1, T, E, E, att, E, out_w, E, proj, E, bias=out_b)
        h1 = _empty((T, E), x)
        st1 = _empty((T, 2), x)
        call("rlt_add_layernorm_fwd", ptr(x), ptr(proj), ptr(n1_w), ptr(n1_b), T, E, eps, drop_p, s_ln1, ptr(h1), ptr(st1), stream())
        hid = _empty((T, Fh), x)
        relu_bits = None
        if Fh % 32 == 0:
            # 1-bit mask (passed the ReLU and kept by the dropout) for the backward dH product, which then reads
            # T*Fh/8 bytes instead of the 4*T*Fh of `hid`
            relu_bits = alloc_relu_bits(T, Fh, x.device)
            gemm_bits(0, 1, T, Fh, E, h1, E, w1, E, hid, Fh, bias=b1, flags=N.GEMM_RELU, bits_out=relu_bits,
                      drop_p=drop_p, seed=s_ffn)
        else:
            gemm(0, 1, T, Fh, E, h1, E, w1, E, hid, Fh, bias=b1, flags=N.GEMM_RELU, drop_p=drop_p, seed=s_ffn)
        ff = _empty((T, E), x)
        gemm(0, 1, T, E, Fh, hid, Fh, w2, Fh, ff, E, bias=b2)
        y = _empty((T, E), x)
        st2 = _empty((T, 2), x)
        call("rlt_add_layernorm_fwd", ptr(h1), ptr(ff), ptr(n2_w), ptr(n2_b), T, E, eps, drop_p, s_ln2, ptr(y), ptr(st2), stream())
        ctx.cfg = (S, B, H, HD, eps, drop_p, seeds)
        ctx.images = images
        ctx.relu_bits = relu_bits
        ctx.save_for_backward(x, in_w, out_w, n1_w, w1, w2, n2_w, qkv, att, lse, proj, st1, h1, hid, ff, st2)
        return y

    @staticmethod
    def _backward(ctx, dy):
        x, in_w, out_w, n1_w, w1, w2, n2_w, qkv, att, lse, proj, st1, h1, hid, ff, st2 = ctx.saved_tensors
        S, B, H, HD, eps, drop_p, (s_attn, s_ln1, s_ffn, s_ln2) = ctx.cfg
        pr = ctx.prec
        T, E = x.shape
        Fh = w1.shape[0]
        dy = N.f32c(dy)

        def ln_bwd(xx, rr, gamma, stats, dyy, seed):
            dz = _empty((T, E), x)
            dr = _empty((T, E), x) if drop_p > 0 else None
            dg, db = _empty((E,), x), _empty((E,), x)
            ws_bytes = query("rlt_add_layernorm_bwd_workspace", T, E)
            ws = workspace(ws_bytes, x.device)
            call("rlt_add_layernorm_bwd", ptr(xx), ptr(rr), ptr(gamma), ptr(stats), ptr(dyy), T, E, drop_p, seed,
                 ptr(dz), ptr(dr), ptr(dg), ptr(db), 0, ptr(ws), ws_bytes, stream())
            return dz, (dz if dr is None else dr), dg, db

        # LN2: dz2 = gradient of h1 through the residual, dr2 = gradient of the FFN branch output
        dz2, dr2, dn2_w, dn2_b = ln_bwd(h1, ff, n2_w, st2, dy, s_ln2)
        dw2, db2 = _empty((E, Fh), x), _empty((E,), x)
        gemm(1, 0, E, Fh, T, dr2, E, hid, Fh, dw2, Fh, colsum_a=db2)
        dhid = _empty((T, Fh), x)
        if ctx.relu_bits is not None:
            gemm_bits(0, 0, T, Fh, E, dr2, E, w2, Fh, dhid, Fh, bits_in=ctx.relu_bits, mask_scale=1.0 / (1.0 - drop_p))
            ctx.relu_bits = None
        else:
            gemm(0, 0, T, Fh, E, dr2, E, w2, Fh, dhid, Fh, relu_mask=hid, ldmask=Fh, mask_scale=1.0 / (1.0 - drop_p))
        dw1, db1 = _empty((Fh, E), x), _empty((Fh,), x)
        gemm(1, 0, Fh, E, T, dhid, Fh, h1, E, dw1, E, colsum_a=db1)
        gemm(0, 0, T, E, Fh, dhid, Fh, w1, E, dz2, E, flags=N.GEMM_ACCUMULATE)       # dh1 = dz2 + dhid W1, in place
        del dhid
        # LN1
        dz1, dr1, dn1_w, dn1_b = ln_bwd(x, proj, n1_w, st1, dz2, s_ln1)
        dw_o, db_o = _empty((E, E), x), _empty((E,), x)
        gemm(1, 0, E, E, T, dr1, E, att, E, dw_o, E, colsum_a=db_o)
        datt = _empty((T, E), x)
        gemm(0, 0, T, E, E, dr1, E, out_w, E, datt, E)
        # attention
        if ctx.axis == "position":
            dqkv = _seq_attention_bwd(qkv, att, datt, lse, S, B, H, HD, drop_p, s_attn, pr, ctx.causal)
        else:
            dqkv = _list_attention_bwd(qkv, att, datt, lse, ctx.images, S, B, H, HD, drop_p, s_attn, pr)
            ctx.images = None
        # in_proj
        dw_in, db_in = _empty((3 * E, E), x), _empty((3 * E,), x)
        gemm(1, 0, 3 * E, E, T, dqkv, 3 * E, x, E, dw_in, E, colsum_a=db_in)
        gemm(0, 0, T, E, 3 * E, dqkv, 3 * E, in_w, E, dz1, E, flags=N.GEMM_ACCUMULATE)    # dx = dz1 + dqkv W_in, in place
        return (dz1, dw_in, db_in, dw_o, db_o, dn1_w, dn1_b, dw1, db1, dw2, db2, dn2_w, dn2_b,
                None, None, None, None, None, None)


class EncoderLayerSeqFn(Function):
    """The encoder layer with WITHIN-LIST attention (every list attends over its own positions; nn.TransformerEncoderLayer with
    batch_first=True): the host composition of EncoderLayerKernelsFn - in_proj, attention, out_proj, the two residual +
    LayerNorm calls, the FFN pair with its 1-bit mask, the two RLT_GEMM_ACCUMULATE fan-out gradients - with
    rlt_seq_attention_fwd / _bwd in the attention slot.  This IS the product path of axis='position'."""

    @staticmethod
    def forward(ctx, *args):
        ctx.prec = current_precision()
        ctx.axis, ctx.causal = "position", False
        with precision(ctx.prec):
            return EncoderLayerKernelsFn._forward(ctx, *args)

    @staticmethod
    def backward(ctx, dy):
        with precision(ctx.prec):
            return EncoderLayerKernelsFn._backward(ctx, dy)


class EncoderLayerSeqCausalFn(EncoderLayerSeqFn):
    """EncoderLayerSeqFn under the causal mask: position i attends to the positions <= i of its list (rlt_seq_attention_fwd_ex /
    _bwd_ex with RLT_SEQ_MASK_CAUSAL); everything else of the layer is per row, so row i of the layer's output depends on the
    rows <= i of its input only."""

    @staticmethod
    def forward(ctx, *args):
        ctx.prec = current_precision()
        ctx.axis, ctx.causal = "position", True
        with precision(ctx.prec):
            return EncoderLayerKernelsFn._forward(ctx, *args)


ATTENTION_AXES = ("list", "position")
ATTENTION_MASKS = ("none", "causal")


def check_attention_axis(axis):
    if axis not in ATTENTION_AXES:
        raise ValueError(f"attention axis must be one of {ATTENTION_AXES}, got {axis!r}")
    return axis


def check_attention_mask(mask, axis):
    """'none' or 'causal'; the causal mask exists on the position axis only (on the list axis the keys are other lists, which
    have no order).  -> True for 'causal'."""
    if mask not in ATTENTION_MASKS:
        raise ValueError(f"attention mask must be one of {ATTENTION_MASKS}, got {mask!r}")
    if mask == "causal" and check_attention_axis(axis) != "position":
        raise ValueError("attention mask 'causal' needs attention axis 'position' (the list axis attends across lists, not positions)")
    return mask == "causal"


def encoder_layer(x, layer, S, B, H, drop_p=0.0, eps=1e-5, axis="list", causal=False):
    """`layer`: a ParamTree mirror of nn.TransformerEncoderLayer.  axis='list': the lists of the mini-batch attend to each other at
    every position (what the reference computes); axis='position': every list attends over its own positions - with causal=True
    position i over the positions <= i only (nn.TransformerEncoderLayer called with the upper-triangular src_mask)."""
    check_attention_axis(axis)
    if causal and axis != "position":
        raise ValueError("causal=True needs axis='position' (the list axis attends across lists, not positions)")
    att = layer.self_attn
    seeds = tuple(next_seed() for _ in range(4)) if drop_p > 0 else (0, 0, 0, 0)
    if axis == "position":
        fn = EncoderLayerSeqCausalFn if causal else EncoderLayerSeqFn
    else:
        fn = EncoderLayerKernelsFn if (KernelTimer.active is not None or KERNEL_LEVEL_ENCODER[0]) else EncoderLayerFn
    return fn.apply(x, att.in_proj_weight, att.in_proj_bias, att.out_proj.weight, att.out_proj.bias,
                                layer.norm1.weight, layer.norm1.bias, layer.linear1.weight, layer.linear1.bias,
                                layer.linear2.weight, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias,
                                S, B, H, eps, drop_p, seeds)


def encoder_ffn_hidden(y):
    """Tests only: the FFN hidden activation (T, FF) inside the stash of the encoder-layer tape node `y` (or the node
    that produced the tensor `y`); offsets: enc_stash() in csrc/path.hip; valid until that node's backward has run."""
    node = y.grad_fn if torch.is_tensor(y) else y
    if type(node).__name__ != "EncoderLayerFnBackward" or node.stash is None:
        raise RuntimeError("not the output of a live encoder-layer tape node")
    S, B, E, H, FF = node.cfg[:5]
    T, rup = S * B, lambda n: (n + 255) // 256 * 256
    off = rup(T * 3 * E * 4) + rup(T * E * 4) + rup(S * H * B * 4) + rup(T * E * 4) + rup(T * 2 * 4) + rup(T * E * 4)
    return node.stash[off:off + T * FF * 4].view(torch.float32).view(T, FF)


# ------------------------------------------------------------------------------ 2-layer BiLSTM (H = 128)
class BiLSTMFn(Function):
    """nn.LSTM(input, hidden, num_layers=2, batch_first=True, bidirectional=True) on position-major input x (S*B, I) ->
    (S*B, 2*hidden), ONE tape node on the path-level entry points: hidden 128 (what the reference hard-codes outside
    MMOECut's `encoding_size` argument) on the persistent recurrence kernels (rlt_bilstm_fwd / _bwd, csrc/path.hip),
    any other hidden size on the general step-by-step form (rlt_bilstm_generic_fwd / _bwd, csrc/lstm_generic.hip)."""

    @staticmethod
    def forward(ctx, x, S, B, *w):          # w: 16 tensors, per layer w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r
        T, I = x.shape
        if len(w) != 16:
            raise RuntimeError("BiLSTMFn takes the 16 parameters of a 2-layer bidirectional LSTM")
        Hd = w[1].shape[1]
        if w[0].shape != (4 * Hd, I) or w[4].shape != (4 * Hd, I) or w[8].shape != (4 * Hd, 2 * Hd) or w[1].shape != (4 * Hd, Hd) or T != S * B:
            raise RuntimeError(f"BiLSTM input has {I} features x {T} rows; the layers were built for "
                               f"{w[0].shape[1]} features, hidden {Hd} and S*B = {S * B} rows")
        fast = Hd == 128
        pr = current_precision()
        if fast:
            stash_bytes = query("rlt_workspace_bytes", N.OP_BILSTM_STASH, S, B, I, 0, 0, 0, pr)
            ws_bytes = query("rlt_workspace_bytes", N.OP_BILSTM_WS, S, B, I, 0, 0, 0, pr)
        else:
            stash_bytes = query("rlt_bilstm_generic_bytes", 1, S, B, I, Hd)
            ws_bytes = query("rlt_bilstm_generic_bytes", 0, S, B, I, Hd)
        stash = N.byte_buffer(stash_bytes, x.device)
        ws = N.byte_buffer(ws_bytes, x.device)
        h = _empty((T, 2 * Hd), x)
        wp = N.lstm_ptrs([w[0:8], w[8:16]])
        if fast:
            _launch("bilstm_fwd", lambda: call("rlt_bilstm_fwd", ptr(x), I, wp, S, B, ptr(h), ptr(stash), stash_bytes,
                                               ptr(ws), ws_bytes, pr, stream()))
        else:
            call("rlt_bilstm_generic_fwd", ptr(x), I, Hd, wp, S, B, ptr(h), ptr(stash), stash_bytes, ptr(ws), ws_bytes, pr, stream())
        ctx.cfg = (S, B, I, Hd, stash_bytes, ws_bytes, pr)
        ctx.stash = stash
        ctx.save_for_backward(x, h, *w)
        return h

    @staticmethod
    def backward(ctx, dh):
        if ctx.stash is None:
            raise RuntimeError("BiLSTMFn.backward overwrites its stash in place and can run only once")
        x, h, *w = ctx.saved_tensors
        S, B, I, Hd, stash_bytes, ws_bytes, pr = ctx.cfg
        dh = N.f32c(dh)
        grads = [torch.empty_like(t) for t in w]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ws = N.byte_buffer(ws_bytes, x.device)
        wp, gp = N.lstm_ptrs([w[0:8], w[8:16]]), N.lstm_ptrs([grads[0:8], grads[8:16]])
        if Hd == 128:
            _launch("bilstm_bwd", lambda: call("rlt_bilstm_bwd", ptr(x), I, wp, ptr(h), ptr(dh), S, B, ptr(ctx.stash), stash_bytes,
                                               ptr(dx), gp, ptr(ws), ws_bytes, pr, stream()))
        else:
            call("rlt_bilstm_generic_bwd", ptr(x), I, Hd, wp, ptr(h), ptr(dh), S, B, ptr(ctx.stash), stash_bytes,
                 ptr(dx), gp, ptr(ws), ws_bytes, pr, stream())
        ctx.stash = None
        return (dx, None, None, *grads)


def bilstm(x, params, S, B):
    """`params`: a ParamTree mirror of the reference's nn.LSTM (state_dict names weight_ih_l0 ... bias_hh_l1_reverse)."""
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    w = [getattr(params, f"{n}_l{layer}{suffix}") for layer in (0, 1) for suffix in ("", "_reverse") for n in names]
    return BiLSTMFn.apply(x, S, B, *w)


# ------------------------------------------------------------------------------ the same stack on a sparse layer-0 input
class SparseBatch:
    """BiCut's input without the zeros: `dense` (B,S,Dn) float32 (retrieval score, then the scalar statistics), `ids` (B,S)
    int32 (the row of each ranked document in `table`) and `table`, an object with `n_docs`, `V`, the CSR arrays `indptr` /
    `indices` / `values` (int64 / int32 / float32) and the static term index `col_ptr` / `col_rows` / `col_vals` / `chunk_col` /
    `chunk_ptr` / `multi_cols`, `n_chunks`, `n_multi` on the device of `ids` - dataloader.bicut_data.BowTable.to(device) is one.
    Densified it would be the reference's (B, S, Dn + V) input.  `validate`: test the ids against the table (the one host
    synchronisation; leave it out for ids built from the table's own map)."""

    def __init__(self, dense, ids, table, validate=False):
        if dense.dim() != 3 or dense.dtype != torch.float32 or ids.dim() != 2 or ids.dtype != torch.int32 \
                or tuple(dense.shape[:2]) != tuple(ids.shape):
            raise ValueError("SparseBatch: dense must be (B, S, Dn) float32 and ids (B, S) int32 over the same lists")
        if not 1 <= dense.shape[2] <= 16:
            raise ValueError(f"SparseBatch: {dense.shape[2]} dense columns; the kernels take 1..16")
        self.dense, self.ids, self.table, self.validate = dense, ids, table, validate

    @property
    def shape(self):
        return (self.ids.shape[0], self.ids.shape[1], self.dense.shape[2] + int(self.table.V))

    def __getitem__(self, lists):
        if not isinstance(lists, slice):
            raise TypeError("SparseBatch: index with a slice of lists")
        return SparseBatch(self.dense[lists], self.ids[lists], self.table, self.validate)

    def to_dense(self):
        """The reference's (B, S, Dn + V) input (tests and small tables only)."""
        B, S, Dn = self.dense.shape
        t = self.table
        x = torch.zeros((B * S, Dn + int(t.V)), dtype=torch.float32, device=self.ids.device)
        x[:, :Dn] = self.dense.reshape(B * S, Dn)
        ids = self.ids.reshape(-1).long()
        n = (t.indptr[ids + 1] - t.indptr[ids])
        rows = torch.repeat_interleave(torch.arange(B * S, device=ids.device), n)
        pos = torch.arange(int(n.sum()), device=ids.device) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
        j = torch.repeat_interleave(t.indptr[ids], n) + pos
        x[rows, Dn + t.indices[j].long()] = t.values[j]
        return x.view(B, S, -1)

    def struct(self, perm=None):
        """rlt_sparse_batch over contiguous arrays; returns (struct, the tensors it points into)."""
        t = self.table
        dense = self.dense if self.dense.is_contiguous() else self.dense.contiguous()
        ids = self.ids if self.ids.is_contiguous() else self.ids.contiguous()
        N.require_cuda(dense, ids, t.indptr, t.indices, t.values, t.col_ptr, t.col_rows, t.col_vals, t.chunk_col, t.chunk_ptr, t.multi_cols)
        if t.indptr.dtype != torch.int64 or t.indices.dtype != torch.int32 or t.values.dtype != torch.float32 \
                or t.indptr.numel() != int(t.n_docs) + 1 or t.col_ptr.dtype != torch.int64 or t.col_ptr.numel() != int(t.V) + 1 \
                or t.chunk_ptr.numel() != int(t.V) + 1 or t.chunk_col.numel() != int(t.n_chunks):
            raise ValueError("SparseBatch: the table's arrays must be indptr (n_docs+1) int64, indices int32, values float32 and "
                             "the term index of dataloader.bicut_data.term_index")
        if self.validate:
            lo, hi = torch.aminmax(ids)
            if int(lo) < 0 or int(hi) >= int(t.n_docs):
                raise ValueError(f"SparseBatch: document row outside [0, {int(t.n_docs)}): min {int(lo)}, max {int(hi)}")
        keep = (dense, ids, perm)
        sb = N.SparseBatchPtrs()
        for name, a in (("dense", dense), ("ids", ids), ("perm", perm)):
            setattr(sb, name, None if a is None else a.data_ptr())
        for name in N.SPARSE_POINTERS[3:]:
            setattr(sb, name, getattr(t, name).data_ptr())
        sb.Dn, sb.n_docs, sb.V, sb.n_chunks, sb.n_multi = dense.shape[2], int(t.n_docs), int(t.V), int(t.n_chunks), int(t.n_multi)
        return sb, keep


class BiLSTMSparseFn(Function):
    """BiLSTMFn with layer 0 fed by a SparseBatch (rlt_bilstm_sparse_fwd / _bwd, csrc/path.hip + csrc/sparse_in.hip): w[0] and
    w[4] - weight_ih_l0 and weight_ih_l0_reverse - are (512, Dn + V) tensors stored COLUMN-MAJOR (strides (1, 512)), and so are
    their gradients, of which every column is written.  No gradient for the input: it is data."""

    @staticmethod
    def forward(ctx, batch, S, B, *w):
        if len(w) != 16:
            raise RuntimeError("BiLSTMSparseFn takes the 16 parameters of a 2-layer bidirectional LSTM")
        I = batch.shape[2]
        for k in (0, 4):
            if tuple(w[k].shape) != (512, I) or w[k].stride() != (1, 512):
                raise RuntimeError(f"sparse BiLSTM: layer-0 input weight of shape {tuple(w[k].shape)} and strides {w[k].stride()}; "
                                   f"the batch needs (512, {I}) stored column-major, strides (1, 512)")
        if tuple(batch.ids.shape) != (B, S) or tuple(w[1].shape) != (512, 128) or tuple(w[8].shape) != (512, 256):
            raise RuntimeError("sparse BiLSTM: hidden size 128, two layers, ids (B, S)")
        dev = batch.ids.device
        pr = current_precision()
        t = batch.table
        # token rows ordered by (table row, token row): a fixed-size sort, no host synchronisation
        perm = torch.sort(batch.ids.t().reshape(-1), stable=True)[1].to(torch.int32)
        sb, keep = batch.struct(perm)
        stash_bytes = query("rlt_workspace_bytes", N.OP_BILSTM_STASH, S, B, 256, 0, 0, 0, pr)
        ws_bytes = query("rlt_bilstm_sparse_workspace", S, B, sb.Dn, sb.n_docs, sb.V, sb.n_chunks)
        if not stash_bytes or not ws_bytes:
            raise RuntimeError("sparse BiLSTM: shape outside what the kernels support")
        stash = N.byte_buffer(stash_bytes, dev)
        ws = N.byte_buffer(ws_bytes, dev)
        h = torch.empty((S * B, 256), dtype=torch.float32, device=dev)
        wp = N.lstm_ptrs([w[0:8], w[8:16]])
        _launch("bilstm_sparse_fwd", lambda: call("rlt_bilstm_sparse_fwd", N.ctypes.byref(sb), wp, S, B, ptr(h), ptr(stash), stash_bytes,
                                                  ptr(ws), ws_bytes, pr, stream()))
        ctx.cfg = (S, B, stash_bytes, ws_bytes, pr)
        ctx.stash, ctx.sb, ctx.keep, ctx.table = stash, sb, keep, t
        ctx.save_for_backward(h, *w)
        return h

    @staticmethod
    def backward(ctx, dh):
        if ctx.stash is None:
            raise RuntimeError("BiLSTMSparseFn.backward overwrites its stash in place and can run only once")
        h, *w = ctx.saved_tensors
        S, B, stash_bytes, ws_bytes, pr = ctx.cfg
        dh = N.f32c(dh)
        grads = [torch.empty_like(t) for t in w]            # (preserves the column-major strides of w[0] and w[4])
        ws = N.byte_buffer(ws_bytes, h.device)
        wp, gp = N.lstm_ptrs([w[0:8], w[8:16]]), N.lstm_ptrs([grads[0:8], grads[8:16]])
        _launch("bilstm_sparse_bwd", lambda: call("rlt_bilstm_sparse_bwd", N.ctypes.byref(ctx.sb), wp, ptr(h), ptr(dh), S, B,
                                                  ptr(ctx.stash), stash_bytes, gp, ptr(ws), ws_bytes, pr, stream()))
        ctx.stash = None
        return (None, None, None, *grads)


def bilstm_sparse(batch, params, S, B):
    """`params`: as for bilstm(), with weight_ih_l0 / weight_ih_l0_reverse stored column-major (models.BiCut(sparse_input=True))."""
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    w = [getattr(params, f"{n}_l{layer}{suffix}") for layer in (0, 1) for suffix in ("", "_reverse") for n in names]
    return BiLSTMSparseFn.apply(batch, S, B, *w)


# ------------------------------------------------------------------------------ layout
class ToPositionMajorFn(Function):
    """(B,S,F) -> (S*B,F)."""

    @staticmethod
    def forward(ctx, x):
        B, S, F = x.shape
        out = _empty((S * B, F), x)
        call("rlt_to_position_major", ptr(x), B, S, F, ptr(out), stream())
        ctx.dims = (B, S, F)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, S, F = ctx.dims
        dout = N.f32c(dout)
        dx = _empty((B, S, F), dout)
        call("rlt_from_position_major", ptr(dout), B, S, F, ptr(dx), stream())
        return dx


def to_position_major(x):
    return ToPositionMajorFn.apply(x)


class ChoopyEmbedFn(Function):
    """cat(score, position_encoding) in position-major layout: (B,S,1),(S,E-1) -> (S*B,E)."""

    @staticmethod
    def forward(ctx, score, pe):
        B, S = score.shape[0], score.shape[1]
        E = pe.shape[1] + 1
        out = _empty((S * B, E), score)
        call("rlt_choopy_embed", ptr(score), ptr(pe), B, S, E, ptr(out), stream())
        ctx.dims = (B, S, E)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, S, E = ctx.dims
        dout = N.f32c(dout)
        dpe = _empty((S, E - 1), dout)
        # dPE[s] = sum over the B rows of position s, columns 1..E-1
        call("rlt_segment_colsum", N.c_void_p(dout.data_ptr() + 4), E, S, B, E - 1, ptr(dpe), E - 1, 0, stream())
        dscore = None
        if ctx.needs_input_grad[0]:
            col = dout[:, 0].contiguous().view(S, B, 1)
            dscore = _empty((B, S, 1), dout)
            call("rlt_from_position_major", ptr(col), B, S, 1, ptr(dscore), stream())
        return dscore, dpe


def choopy_embed(score, pe):
    return ChoopyEmbedFn.apply(score, pe)


# ------------------------------------------------------------------------------ heads
class HeadsFn(Function):
    """n Linear(E,1) heads + {softmax over positions | sigmoid | identity}: x (S*B,E) -> (n,B,S)."""

    @staticmethod
    def forward(ctx, x, w, b, kinds, S, B):
        n, E = w.shape
        out = _empty((n, B, S), x)
        karr = (N.c_int * n)(*kinds)
        call("rlt_heads_fwd", ptr(x), ptr(w), ptr(b), karr, n, S, B, E, ptr(out), stream())
        ctx.meta = (tuple(kinds), S, B)
        ctx.save_for_backward(x, w, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, out = ctx.saved_tensors
        kinds, S, B = ctx.meta
        n, E = w.shape
        dout = N.f32c(dout)
        dx = _empty((S * B, E), x)
        dw, db = _empty((n, E), x), _empty((n,), x)
        karr = (N.c_int * n)(*kinds)
        ws_bytes = query("rlt_heads_bwd_workspace", n, S, B, E)
        ws = workspace(ws_bytes, x.device)
        call("rlt_heads_bwd", ptr(x), ptr(w), karr, n, ptr(out), ptr(dout), S, B, E, ptr(dx), 0, ptr(dw), ptr(db),
             ptr(ws), ws_bytes, stream())
        return dx, dw, db, None, None, None


def heads(x, weights, biases, kinds, S, B):
    """weights: list of (1,E) parameters, biases: list of (1,) parameters (glue: tiny cat)."""
    w = torch.cat([wi.reshape(1, -1) for wi in weights], dim=0) if len(weights) > 1 else weights[0].reshape(1, -1)
    b = torch.cat([bi.reshape(1) for bi in biases], dim=0) if len(biases) > 1 else biases[0].reshape(1)
    out = HeadsFn.apply(x, w, b, kinds, S, B)
    return [out[i].unsqueeze(2) for i in range(len(kinds))]          # each (B,S,1)


class HazardHeadFn(Function):
    """Linear(E,1) stop logits -> (p, stop), both (B,S): stop_s = sigmoid(z_s), p_s = stop_s prod_{j<s} (1 - stop_j), the last
    position taking the remaining mass (rlt_hazard_head_fwd).  The tape keeps z: the backward recomputes the rest from it."""

    @staticmethod
    def forward(ctx, x, w, b, offset, S, B):
        E = w.numel()
        p, stop, z = _empty((B, S), x), _empty((B, S), x), _empty((B, S), x)
        call("rlt_hazard_head_fwd", ptr(x), ptr(w), ptr(b), ptr(offset), S, B, E, ptr(p), ptr(stop), ptr(z), stream())
        ctx.meta = (S, B)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, w, z)
        return p, stop

    @staticmethod
    def backward(ctx, dp, dstop):
        x, w, z = ctx.saved_tensors
        S, B = ctx.meta
        E = w.numel()
        # an output nothing read has no gradient (None): the losses read p alone, and dstop = NULL is the kernel's own form of that
        dp = torch.zeros_like(z) if dp is None else N.f32c(dp)
        dstop = None if dstop is None else N.f32c(dstop)
        dx = _empty((S * B, E), x)
        dw, db = _empty((1, E), x), _empty((1,), x)
        ws_bytes = query("rlt_hazard_head_bwd_workspace", S, B, E)
        ws = workspace(ws_bytes, x.device)
        call("rlt_hazard_head_bwd", ptr(x), ptr(w), ptr(z), ptr(dp), ptr(dstop), S, B, E, ptr(dx), 0, ptr(dw), ptr(db),
             ptr(ws), ws_bytes, stream())
        return dx, dw, db, None, None, None


def hazard_prior_offset(S, device=None):
    """(S,) fp32: offset_s = -log(S-1-s) for s < S-1, 0 at the end.  With it a zero weight and bias give the uniform cut
    distribution (stop_s = 1 / (S-s)); without it they give a geometric one with mean 2."""
    off = torch.zeros(S, dtype=torch.float32)
    if S > 1:
        off[:S - 1] = -torch.log(torch.arange(S - 1, 0, -1, dtype=torch.float64)).float()
    return off if device is None else off.to(device)


def hazard_head(x_pm, weight, bias, S, B, offset=None):
    """x_pm (S*B,E) position-major, weight (1,E) or (E,), bias (1,), offset (S,) or None -> (p, stop), each (B,S) and
    differentiable.  p[b,s], stop[b,s] depend, to the bit, on rows <= s of list b only (p[b,S-1] excepted)."""
    E = x_pm.shape[1]
    if weight.numel() != E or bias.numel() != 1:
        raise ValueError(f"hazard_head: one weight row of {E} and one bias, got {tuple(weight.shape)} and {tuple(bias.shape)}")
    if offset is not None:
        if offset.numel() != S:
            raise ValueError(f"hazard_head: offset must have S = {S} elements, got {tuple(offset.shape)}")
        offset = N.f32c(offset.detach())
    return HazardHeadFn.apply(N.f32c(x_pm), N.f32c(weight.reshape(1, E)), N.f32c(bias.reshape(1)), offset, S, B)


def hazard_head_append(x_pm, weight, bias, t0, B, carry, tau=1.0, final=False, active=None, k=None, offset=None, want_p=False,
                       want_z=False):
    """Streaming (inference only, no tape): the hazard head on a chunk of positions t0 .. t0+C-1 (rlt_hazard_head_append).
    x_pm (C*B, E) position-major; carry (B,) float64, in place: zeros before the chunk at t0 = 0; offset (C,): the chunk's slice
    of the prior offset, or None; final: the chunk ends the list.  With active (B,) int32 and k (B,) int32, both in place, the
    stop decision is taken on the device: the first row with stop >= tau (cut_sweep's 'above' comparison) writes k = its 1-based
    rank and clears active; under final every list still active stops at the last row.  -> {'stop', 'p', 'z'}: (B, C) each, p and
    z None unless asked for.  The rows of a list that was retired on entry are not written: they are NaN."""
    N.require_cuda(x_pm)
    T, E = x_pm.shape
    if T % B or T == 0:
        raise ValueError(f"hazard_head_append: {T} rows are not a whole number of positions of {B} lists")
    C = T // B
    if weight.numel() != E or bias.numel() != 1:
        raise ValueError(f"hazard_head_append: one weight row of {E} and one bias, got {tuple(weight.shape)} and {tuple(bias.shape)}")
    if carry.dtype != torch.float64 or carry.shape != (B,) or not carry.is_contiguous() or carry.device != x_pm.device:
        raise ValueError(f"hazard_head_append: carry must be a contiguous float64 tensor of shape ({B},) on {x_pm.device}")
    if (active is None) != (k is None):
        raise ValueError("hazard_head_append: pass both `active` and `k`, or neither")
    _check_active(active, B, x_pm, "hazard_head_append")
    if k is not None and (k.dtype != torch.int32 or k.shape != (B,) or not k.is_contiguous() or k.device != x_pm.device):
        raise ValueError(f"hazard_head_append: k must be a contiguous int32 tensor of shape ({B},) on {x_pm.device}")
    if offset is not None:
        if offset.numel() != C:
            raise ValueError(f"hazard_head_append: offset must have C = {C} elements (the chunk's slice), got {tuple(offset.shape)}")
        offset = N.f32c(offset.detach())
    if t0 < 0:
        raise ValueError(f"hazard_head_append: t0 = {t0} is negative")
    x = N.f32c(x_pm.detach())
    w, b = N.f32c(weight.detach().reshape(1, E)), N.f32c(bias.detach().reshape(1))
    new = (lambda: _empty((B, C), x)) if active is None else (lambda: torch.full((B, C), float("nan"), dtype=torch.float32, device=x.device))
    stop, p, z = new(), (new() if want_p else None), (new() if want_z else None)
    _launch("hazard_append", lambda: call("rlt_hazard_head_append", ptr(x), ptr(w), ptr(b), ptr(offset), t0, C, B, E, 1 if final else 0,
                                          ptr(carry), float(tau), ptr(active), ptr(k), ptr(stop), ptr(p), ptr(z), stream()))
    return {"stop": stop, "p": p, "z": z}


def _check_slots(t, n, dtype, like, what, name):
    if t.dtype != dtype or t.shape != (n,) or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"{what}: {name} must be a contiguous {str(dtype).split('.')[-1]} tensor of shape ({n},) on {like.device}")


def stream_compact_plan(active, origin=None, carry=None, k=None, k_full=None):
    """Streaming (inference only): the slot map that takes the retired lists out of a running stream (rlt_stream_compact_plan).
    active (B,) int32: a slot is live iff non-zero; origin (B,) int32: each slot's original list number, None = the identity; carry
    (B,) float64 or None; k (B,) int32 together with k_full (B_full,) int32, written in place - k_full[origin[b]] = k[b] for every
    retired slot -, or neither.  -> {'slot_src': (B,) int32, the live slots ascending then -1, 'origin': (B,) int32, their original
    numbers then -1, 'carry': (B,) float64 gathered through slot_src (None without carry; not initialised behind the live slots),
    'n_live': (1,) int32 ON THE DEVICE: the call does not synchronise}."""
    N.require_cuda(active)
    if active.dim() != 1 or active.shape[0] < 1:
        raise ValueError(f"stream_compact_plan: active must be a contiguous int32 tensor of shape (B,) with B >= 1, got {tuple(active.shape)}")
    B = int(active.shape[0])
    _check_active(active, B, active, "stream_compact_plan")
    if origin is not None:
        _check_slots(origin, B, torch.int32, active, "stream_compact_plan", "origin")
    if carry is not None:
        _check_slots(carry, B, torch.float64, active, "stream_compact_plan", "carry")
    if (k is None) != (k_full is None):
        raise ValueError("stream_compact_plan: pass both `k` and `k_full`, or neither")
    B_full = B
    if k is not None:
        _check_slots(k, B, torch.int32, active, "stream_compact_plan", "k")
        if k_full.dim() != 1 or k_full.shape[0] < B:
            raise ValueError(f"stream_compact_plan: k_full must be a contiguous int32 tensor of shape (B_full,) with B_full >= B = {B}, got {tuple(k_full.shape)}")
        B_full = int(k_full.shape[0])
        _check_slots(k_full, B_full, torch.int32, active, "stream_compact_plan", "k_full")
        if k_full.data_ptr() == k.data_ptr():
            raise ValueError("stream_compact_plan: k_full must not be k itself (the call reads one while it writes the other)")
    slot_src, origin_out = torch.empty_like(active), torch.empty_like(active)
    carry_out = None if carry is None else torch.empty_like(carry)
    n_live = torch.empty(1, dtype=torch.int32, device=active.device)
    _launch("stream_compact_plan", lambda: call("rlt_stream_compact_plan", ptr(active), ptr(origin), ptr(carry), ptr(k), B, B_full, ptr(slot_src),
                                                ptr(origin_out), ptr(carry_out), ptr(k_full), ptr(n_live), stream()))
    return {"slot_src": slot_src, "origin": origin_out, "carry": carry_out, "n_live": n_live}


def kv_cache_compact(src, dst, slot_src, t0, B_src, B_dst):
    """Streaming (inference only): gather the first t0 ranks of a K/V cache of B_src slots into one of B_dst slots through the map
    of stream_compact_plan (rlt_kv_cache_compact): dst row s*B_dst + j = src row s*B_src + slot_src[j], bit for bit.  src
    (>= t0*B_src, 2E) and dst (>= t0*B_dst, 2E) fp32, contiguous, two different buffers; slot_src int32 with at least B_dst entries.
    dst is written in place; its rows from t0*B_dst on are not touched."""
    N.require_cuda(src)
    if min(t0, B_dst) < 0 or B_src < 1 or B_dst > B_src:
        raise ValueError(f"kv_cache_compact: t0 = {t0}, B_src = {B_src}, B_dst = {B_dst} is not a compaction of t0 >= 0 ranks to 0 <= B_dst <= B_src slots")
    for t, rows, name in ((src, t0 * B_src, "src"), (dst, t0 * B_dst, "dst")):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[0] < rows or t.device != src.device:
            raise ValueError(f"kv_cache_compact: {name} must be a contiguous fp32 tensor of at least {rows} rows on {src.device}, got {tuple(t.shape)}")
    if src.shape[1] != dst.shape[1]:
        raise ValueError(f"kv_cache_compact: src and dst rows differ, {src.shape[1]} and {dst.shape[1]} columns")
    if slot_src.dtype != torch.int32 or slot_src.dim() != 1 or not slot_src.is_contiguous() or slot_src.shape[0] < B_dst or slot_src.device != src.device:
        raise ValueError(f"kv_cache_compact: slot_src must be a contiguous int32 tensor of at least {B_dst} entries on {src.device}")
    _launch("kv_cache_compact", lambda: call("rlt_kv_cache_compact", ptr(src), ptr(dst), ptr(slot_src), t0, B_src, B_dst, int(src.shape[1]), stream()))


# ------------------------------------------------------------------------------ MMOE
class MMOEGateFn(Function):
    """gates (n_tasks,B,n_e) = softmax_e(flatten_s(h[b]) @ w_gate[t])."""

    @staticmethod
    def forward(ctx, h, S, B, *w_gates):
        C = h.shape[1]
        nt, ne = len(w_gates), w_gates[0].shape[1]
        gates = _empty((nt, B, ne), h)
        warr = N.pointer_array(w_gates)
        call("rlt_mmoe_gate_fwd", ptr(h), warr, nt, ne, S, B, C, ptr(gates), stream())
        ctx.dims = (S, B, C, nt, ne)
        ctx.save_for_backward(h, gates, *w_gates)
        return gates

    @staticmethod
    def backward(ctx, dgates):
        h, gates, *w_gates = ctx.saved_tensors
        S, B, C, nt, ne = ctx.dims
        dgates = N.f32c(dgates)
        dh = torch.empty_like(h)
        dws = [torch.empty_like(w) for w in w_gates]
        ws_bytes = query("rlt_mmoe_gate_bwd_workspace", nt, ne, S, B, C)
        ws = workspace(ws_bytes, h.device)
        call("rlt_mmoe_gate_bwd", ptr(h), N.pointer_array(w_gates), ptr(gates), ptr(dgates), nt, ne, S, B, C,
             ptr(dh), 0, N.pointer_array(dws), ptr(ws), ws_bytes, stream())
        return (dh, None, None, *dws)


class MMOEMixFn(Function):
    """mixed (n_tasks,S*B,E) = sum_e gates[t][b][e] * expert_e."""

    @staticmethod
    def forward(ctx, gates, S, B, *experts):
        nt, _, ne = gates.shape
        E = experts[0].shape[1]
        mixed = _empty((nt, S * B, E), gates)
        call("rlt_mmoe_mix_fwd", N.pointer_array(experts), ptr(gates), nt, ne, S, B, E, ptr(mixed), stream())
        ctx.dims = (S, B, E, nt, ne)
        ctx.save_for_backward(gates, *experts)
        return mixed

    @staticmethod
    def backward(ctx, dmixed):
        gates, *experts = ctx.saved_tensors
        S, B, E, nt, ne = ctx.dims
        dmixed = N.f32c(dmixed)
        dex = [torch.empty_like(e) for e in experts]
        dgates = torch.empty_like(gates)
        call("rlt_mmoe_mix_bwd", N.pointer_array(experts), ptr(gates), ptr(dmixed), nt, ne, S, B, E,
             N.pointer_array(dex), ptr(dgates), stream())
        return (dgates, None, None, *dex)


# ------------------------------------------------------------------------------ losses
_COEF_CACHE = {}


def dcg_coef(S, device):
    """log2(j+2) table exactly as the reference builds it (utils/metrics.py:7), fp32 on device."""
    key = (S, str(device))
    if key not in _COEF_CACHE:
        _COEF_CACHE[key] = torch.tensor([math.log(j + 2, 2) for j in range(S)], dtype=torch.float32, device=device)
    return _COEF_CACHE[key]


_DCG_TABLE_CACHE = {}


def dcg_table(device):
    """The float64 DCG coefficient table of rlt_loss_metrics (1 / log2(j + 2) and its prefix sums), filled once per device by
    rlt_dcg_table_init on the current stream: caller memory, the library keeps no state of its own."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()      # 'cuda' and 'cuda:0' are one device
    if key not in _DCG_TABLE_CACHE:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the DCG table must exist before a hipGraph capture starts: call ops.dcg_table(device) once, eagerly")
        nbytes = query("rlt_dcg_table_bytes")
        with torch.cuda.device(key):
            t = torch.empty((nbytes // 8,), dtype=torch.float64, device=torch.device("cuda", key))
            call("rlt_dcg_table_init", ptr(t), nbytes, stream())
            # filled once, read from whatever stream a later loss call runs on: nothing orders those streams behind this one
            torch.cuda.current_stream().synchronize()
        _DCG_TABLE_CACHE[key] = t
    return _DCG_TABLE_CACHE[key]


def _fused_metric_buffers(B, dev):
    return (torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev),
            torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((2,), dtype=torch.float64, device=dev))


class RewardLossFn(Function):
    """Fused reward matrix + {Choopy | AttnCut | KL | JS} loss; returns a 0-d tensor.  `penalty`: the DCG gain numerator of
    a non-relevant document (Metric_for_Loss.dcg's argument, utils/metrics.py:94).  With `with_metrics` the same kernel
    pass also yields the cut metrics of run.py:141-145 and the call returns (loss, k (B) int32, sums (2) float64 =
    [sum F1@k, sum DCG@k])."""

    @staticmethod
    def forward(ctx, p, labels, metric, kind, tau, penalty=-1.0, with_metrics=False, metric_penalty=-1.0):
        B, S = labels.shape
        coef = dcg_coef(S, p.device) if metric == N.METRIC_DCG else None
        per_list = _empty((B,), p)
        loss = _empty((1,), p)
        dp = _empty((B, S), p)
        ctx.save_for_backward(dp)
        ctx.pshape = p.shape
        if not with_metrics:
            call("rlt_reward_loss_ex", ptr(p), ptr(labels), ptr(coef), B, S, metric, penalty, kind, tau,
                 ptr(per_list), ptr(loss), ptr(dp), stream())
            return loss.reshape(())
        k, f1, dcg, sums = _fused_metric_buffers(B, p.device)
        ws_bytes = query("rlt_loss_metrics_workspace", B)
        ws = workspace(ws_bytes, p.device)
        call("rlt_loss_metrics", ptr(p), ptr(labels), ptr(coef), B, S, metric, penalty, kind, tau, metric_penalty,
             ptr(per_list), ptr(loss), ptr(dp), ptr(k), ptr(f1), ptr(dcg), ptr(sums), ptr(dcg_table(p.device)), ptr(ws), ws_bytes, stream())
        ctx.mark_non_differentiable(k, sums)
        return loss.reshape(()), k, sums

    @staticmethod
    def backward(ctx, go, *_unused):
        (dp,) = ctx.saved_tensors
        g = dp.clone()
        go = N.f32c(go).reshape(1)
        call("rlt_scale", ptr(g), ptr(go), g.numel(), stream())
        return g.view(ctx.pshape), None, None, None, None, None, None, None


class RewardAnyLossFn(Function):
    """RewardLossFn for any cut reward (rlt_reward_any_loss): `spec`, an object whose `native(S, device)` returns the
    rlt_reward_spec struct (utils.rewards.RewardSpec), builds the reward from `labels` in registers; or `r`, a (B,S) reward
    matrix the caller supplies (labels and spec None).  Returns a 0-d loss; with `with_stats` (loss, k (B) int32, stats) where
    stats = {"r_k", "r_best" (B) fp32, "best_k" (B) int32, "sums" (4) float64 = [sum r_k, sum r_best, lists cut at their best
    reward, B]}."""

    @staticmethod
    def forward(ctx, p, labels, spec, r, kind, tau, with_stats=False):
        if (spec is None) == (r is None) or (spec is None) != (labels is None):
            raise ValueError("exactly one reward source: labels + spec, or a reward matrix r")
        B, S = (labels if r is None else r).shape
        dev = p.device
        struct = keep = None
        table = None
        if spec is not None:
            struct, keep = spec.native(S, dev)
            if struct.family == N.REWARD_GAIN and struct.discount is None:
                table = dcg_table(dev)
        per_list = _empty((B,), p)
        loss = _empty((1,), p)
        dp = _empty((B, S), p)
        ctx.save_for_backward(dp)
        ctx.pshape = p.shape
        k = r_k = r_best = best_k = sums = None
        if with_stats:
            k = torch.empty((B,), dtype=torch.int32, device=dev)
            best_k = torch.empty((B,), dtype=torch.int32, device=dev)
            r_k, r_best = _empty((B,), p), _empty((B,), p)
            sums = torch.empty((4,), dtype=torch.float64, device=dev)
        ws_bytes = query("rlt_reward_any_workspace", B)
        ws = workspace(ws_bytes, dev)
        call("rlt_reward_any_loss", ptr(p), ptr(labels), None if struct is None else N.ctypes.byref(struct), ptr(r), B, S, kind, tau,
             ptr(per_list), ptr(loss), ptr(dp), ptr(k), ptr(r_k), ptr(r_best), ptr(best_k), ptr(sums), ptr(table), ptr(ws), ws_bytes,
             stream())
        del keep
        if not with_stats:
            return loss.reshape(())
        ctx.mark_non_differentiable(k, r_k, r_best, best_k, sums)
        return loss.reshape(()), k, r_k, r_best, best_k, sums

    @staticmethod
    def backward(ctx, go, *_unused):
        (dp,) = ctx.saved_tensors
        g = dp.clone()
        go = N.f32c(go).reshape(1)
        call("rlt_scale", ptr(g), ptr(go), g.numel(), stream())
        return g.view(ctx.pshape), None, None, None, None, None, None


class WassDistLossFn(Function):
    """utils/losses.py:236-311: Sinkhorn forward recorded in a workspace, explicit reverse sweep for the gradient."""

    @staticmethod
    def forward(ctx, p, labels, eps, max_iter, thresh):
        B, S = labels.shape
        loss = _empty((1,), p)
        ws_bytes = query("rlt_wass_loss_workspace", B, max_iter)
        ws = workspace(ws_bytes, p.device)
        call("rlt_wass_loss_fwd", ptr(p), ptr(labels), B, S, eps, max_iter, thresh, ptr(loss), ptr(ws), ws_bytes, stream())
        ctx.cfg = (B, S, eps, max_iter, ws_bytes)
        ctx.ws = ws
        ctx.save_for_backward(p, labels)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        p, labels = ctx.saved_tensors
        B, S, eps, max_iter, ws_bytes = ctx.cfg
        dp = _empty((B, S), p)
        go = N.f32c(go).reshape(1)
        call("rlt_wass_loss_bwd", ptr(p), ptr(labels), ptr(go), B, S, eps, max_iter, ptr(ctx.ws), ws_bytes, ptr(dp), stream())
        ctx.ws = None
        return dp, None, None, None, None


class PairSoftmaxFn(Function):
    """BiCut's two-class head: position-major logits (S*B, 2) -> dropout -> softmax over the classes -> (B,S,2)."""

    @staticmethod
    def forward(ctx, z, S, B, drop_p=0.0, seed=0):
        out = _empty((B, S, 2), z)
        call("rlt_pair_softmax_fwd", ptr(z), B, S, drop_p, seed, ptr(out), stream())
        ctx.cfg = (S, B, drop_p, seed)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        S, B, drop_p, seed = ctx.cfg
        dz = _empty((S * B, 2), out)
        call("rlt_pair_softmax_bwd", ptr(out), ptr(N.f32c(dout)), B, S, drop_p, seed, ptr(dz), stream())
        return dz, None, None, None, None


def pair_softmax(z, S, B, drop_p=0.0):
    return PairSoftmaxFn.apply(z, S, B, drop_p, next_seed() if drop_p > 0 else 0)


class BiCutLossFn(Function):
    """utils/losses.py:11-45 with its gradient, one launch."""

    @staticmethod
    def forward(ctx, out, labels, nci, alpha, r):
        B, S = labels.shape
        per_list = _empty((B,), out)
        loss = _empty((1,), out)
        dout = _empty((B, S, 2), out)
        call("rlt_bicut_loss", ptr(out), ptr(labels), B, S, int(nci), alpha, r, ptr(per_list), ptr(loss), ptr(dout), stream())
        ctx.save_for_backward(dout)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        (dout,) = ctx.saved_tensors
        g = dout.clone()
        go = N.f32c(go).reshape(1)
        call("rlt_scale", ptr(g), ptr(go), g.numel(), stream())
        return g, None, None, None, None


class MtCutLossFn(Function):
    """cut JS loss + w_r * rerank hinge + w_c * BCE, one tape node (utils/losses.py:180-191).  `with_metrics`: the cut term's
    kernel pass also yields the cut metrics; returns (loss, k, sums) as RewardLossFn does."""

    @staticmethod
    def forward(ctx, cut_p, rerank, cls, labels, metric, tau, w_r, w_c, margin, with_metrics=False):
        B, S = labels.shape
        dev = cut_p.device
        coef = dcg_coef(S, dev) if metric == N.METRIC_DCG else None
        per_list = _empty((B,), cut_p)
        cut = _empty((1,), cut_p)
        dp = _empty((B, S), cut_p)
        if with_metrics:
            k, f1, dcg, sums = _fused_metric_buffers(B, dev)
            lws_bytes = query("rlt_loss_metrics_workspace", B)
            lws = workspace(lws_bytes, dev)
            call("rlt_loss_metrics", ptr(cut_p), ptr(labels), ptr(coef), B, S, metric, -1.0, N.LOSS_JS, tau, -1.0,
                 ptr(per_list), ptr(cut), ptr(dp), ptr(k), ptr(f1), ptr(dcg), ptr(sums), ptr(dcg_table(dev)), ptr(lws), lws_bytes, stream())
        else:
            call("rlt_reward_loss", ptr(cut_p), ptr(labels), ptr(coef), B, S, metric, N.LOSS_JS, tau,
                 ptr(per_list), ptr(cut), ptr(dp), stream())
        terms = _empty((4,), cut_p)
        ws_bytes = query("rlt_mt_terms_workspace", B, S)
        ws = workspace(ws_bytes, dev)
        call("rlt_mt_terms", ptr(rerank), ptr(cls), ptr(labels), B, S, margin, ptr(terms), ptr(ws), ws_bytes, stream())
        # loss = cut + w_r * hinge + w_c * bce, in the reference's order of additions
        xs, ws_ = [cut], [1.0]
        if rerank is not None:
            xs.append(terms[0:1]); ws_.append(w_r)
        if cls is not None:
            xs.append(terms[1:2]); ws_.append(w_c)
        loss = _empty((1,), cut_p)
        warr = (N.c_float * len(ws_))(*ws_)
        call("rlt_weighted_sum", N.pointer_array(xs), warr, len(xs), ptr(loss), stream())
        ctx.save_for_backward(dp, cls, labels, terms)
        ctx.meta = (w_r, w_c, rerank is not None, cut_p.shape, None if rerank is None else rerank.shape,
                    None if cls is None else cls.shape)
        if with_metrics:
            ctx.mark_non_differentiable(k, sums)
            return loss.reshape(()), k, sums
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go, *_unused):
        dp, cls, labels, terms = ctx.saved_tensors
        w_r, w_c, has_rr, pshape, rshape, cshape = ctx.meta
        B, S = labels.shape
        go = N.f32c(go).reshape(1)
        g = dp.clone()
        call("rlt_scale", ptr(g), ptr(go), g.numel(), stream())
        d_rr = _empty((B, S), dp) if has_rr else None
        d_cl = _empty((B, S), dp) if cls is not None else None
        if has_rr or cls is not None:
            call("rlt_mt_terms_bwd", ptr(cls), ptr(labels), ptr(terms), B, S, w_r, w_c, ptr(go), ptr(d_rr), ptr(d_cl), stream())
        return (g.view(pshape), None if d_rr is None else d_rr.view(rshape), None if d_cl is None else d_cl.view(cshape),
                None, None, None, None, None, None, None)


class MtSideLossFn(Function):
    """w_r * rerank hinge + w_c * BCE of MtCutLoss without its cut term (utils/losses.py:180-191): the multi-task pass on its own,
    for a cut term that another tape node computes (a RewardSpec reward).  rerank or cls may be None."""

    @staticmethod
    def forward(ctx, rerank, cls, labels, w_r, w_c, margin):
        B, S = labels.shape
        dev = labels.device
        terms = _empty((4,), labels)
        ws_bytes = query("rlt_mt_terms_workspace", B, S)
        ws = workspace(ws_bytes, dev)
        call("rlt_mt_terms", ptr(rerank), ptr(cls), ptr(labels), B, S, margin, ptr(terms), ptr(ws), ws_bytes, stream())
        xs, ws_ = [], []
        if rerank is not None:
            xs.append(terms[0:1]); ws_.append(w_r)
        if cls is not None:
            xs.append(terms[1:2]); ws_.append(w_c)
        loss = _empty((1,), labels)
        warr = (N.c_float * len(ws_))(*ws_)
        call("rlt_weighted_sum", N.pointer_array(xs), warr, len(xs), ptr(loss), stream())
        ctx.save_for_backward(cls, labels, terms)
        ctx.meta = (w_r, w_c, None if rerank is None else rerank.shape, None if cls is None else cls.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        cls, labels, terms = ctx.saved_tensors
        w_r, w_c, rshape, cshape = ctx.meta
        B, S = labels.shape
        go = N.f32c(go).reshape(1)
        d_rr = _empty((B, S), labels) if rshape is not None else None
        d_cl = _empty((B, S), labels) if cls is not None else None
        call("rlt_mt_terms_bwd", ptr(cls), ptr(labels), ptr(terms), B, S, w_r, w_c, ptr(go), ptr(d_rr), ptr(d_cl), stream())
        return (None if d_rr is None else d_rr.view(rshape), None if d_cl is None else d_cl.view(cshape), None, None, None, None)


class RerankLossFn(Function):
    """Stand-alone RerankLoss (utils/losses.py:99-141)."""

    @staticmethod
    def forward(ctx, score, labels, margin):
        B, S = labels.shape
        terms = _empty((4,), score)
        ws_bytes = query("rlt_mt_terms_workspace", B, S)
        ws = workspace(ws_bytes, score.device)
        call("rlt_mt_terms", ptr(score), None, ptr(labels), B, S, margin, ptr(terms), ptr(ws), ws_bytes, stream())
        ctx.save_for_backward(labels, terms)
        ctx.sshape = score.shape
        return terms[0].clone()

    @staticmethod
    def backward(ctx, go):
        labels, terms = ctx.saved_tensors
        B, S = labels.shape
        go = N.f32c(go).reshape(1)
        d = _empty((B, S), labels)
        call("rlt_mt_terms_bwd", None, ptr(labels), ptr(terms), B, S, 1.0, 0.0, ptr(go), ptr(d), None, stream())
        return d.view(ctx.sshape), None, None


def _pair_rank_args(kind, sigma, gains, n_grades):
    """(kind code, gain array or None, n_grades) of a rlt_pair_rank_loss call; gains=None is the library's 2^g - 1."""
    if isinstance(kind, str):
        if kind not in N.PAIR_KINDS:
            raise ValueError(f"pair rank kind must be one of {sorted(N.PAIR_KINDS)}, got {kind!r}")
        kind = N.PAIR_KINDS[kind]
    if not (float(sigma) > 0 and math.isfinite(float(sigma))):
        raise ValueError(f"sigma must be positive and finite, got {sigma!r}")
    garr = None
    if gains is not None:
        gains = [float(g) for g in gains]
        n_grades = len(gains)
        garr = (N.c_float * n_grades)(*gains)
    if not 2 <= int(n_grades) <= N.REWARD_MAX_GRADES:
        raise ValueError(f"n_grades must be in 2..{N.REWARD_MAX_GRADES}, got {n_grades}")
    return kind, garr, int(n_grades)


def _pair_rows(t, what):
    t = N.f32c(t)
    if t.dim() == 3 and t.shape[2] == 1:
        t = t.reshape(t.shape[0], t.shape[1])
    if t.dim() != 2:
        raise ValueError(f"pair_rank: {what} must be (B,S) or (B,S,1); got {tuple(t.shape)}")
    return t


class PairRankLossFn(Function):
    """RankNet / LambdaRank loss of a rerank head's scores (rlt_pair_rank_loss): the forward makes ONE call that writes the batch
    loss and d(loss)/d(score); backward only scales that by the incoming gradient.  score, labels: (B,S) fp32."""

    @staticmethod
    def forward(ctx, score, labels, kind, sigma, gains, n_grades, normalize):
        kind, garr, n_grades = _pair_rank_args(kind, sigma, gains, n_grades)
        s = _pair_rows(score, "score")
        B, S = s.shape
        dev = s.device
        loss = _empty((1,), s)
        ds = _empty((B, S), s)
        table = dcg_table(dev) if kind == N.PAIR_LAMBDARANK else None
        ws_bytes = query("rlt_pair_rank_workspace", B, S)
        ws = workspace(ws_bytes, dev)
        call("rlt_pair_rank_loss", ptr(s), ptr(labels), B, S, kind, float(sigma), garr, n_grades, int(bool(normalize)),
             ptr(table), None, None, ptr(loss), ptr(ds), None, None, ptr(ws), ws_bytes, stream())
        ctx.save_for_backward(ds)
        ctx.sshape = score.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        (ds,) = ctx.saved_tensors
        g = ds.clone()
        go = N.f32c(go).reshape(1)
        call("rlt_scale", ptr(g), ptr(go), g.numel(), stream())
        return g.view(ctx.sshape), None, None, None, None, None, None


def pair_rank(score, labels, kind="lambdarank", sigma=1.0, gains=None, n_grades=2, normalize=True):
    """The non-tape form of rlt_pair_rank_loss: (rank (B,S) int32, n_pairs (B) int32, loss_per_list (B) fp32) - the counting
    rank of every document (on NaN-free scores the `rank` of rerank_lists), the number of pairs of unequal grade per list and
    the RankNet / LambdaRank loss of each list.  Tensors in and out, no host read."""
    N.require_cuda(score, labels)
    kind, garr, n_grades = _pair_rank_args(kind, sigma, gains, n_grades)
    s = _pair_rows(score.detach(), "score")
    y = _pair_rows(labels.detach(), "labels")
    if y.shape != s.shape:
        raise ValueError(f"pair_rank: labels {tuple(y.shape)} do not match score's {tuple(s.shape)}")
    B, S = s.shape
    dev = s.device
    rank = torch.empty((B, S), dtype=torch.int32, device=dev)
    n_pairs = torch.empty((B,), dtype=torch.int32, device=dev)
    per_list = _empty((B,), s)
    table = dcg_table(dev) if kind == N.PAIR_LAMBDARANK else None
    ws_bytes = query("rlt_pair_rank_workspace", B, S)
    ws = workspace(ws_bytes, dev)
    call("rlt_pair_rank_loss", ptr(s), ptr(y), B, S, kind, float(sigma), garr, n_grades, int(bool(normalize)),
         ptr(table), None, ptr(per_list), None, None, ptr(rank), ptr(n_pairs), ptr(ws), ws_bytes, stream())
    return rank, n_pairs, per_list


class ProbeHeadsFn(Function):
    """Probe heads on frozen features (rlt_probe_heads): x (S*B,E) -> per-head losses (n,) and activations (n,B,S), with
    each head's gradient of its own loss formed in the same pass; backward only scales it by the incoming go[h]."""

    @staticmethod
    def forward(ctx, x, w, b, labels, kinds, S, B, margin, want_out):
        n, E = w.shape
        loss = _empty((n,), x)
        out = _empty((n, B, S), x) if want_out else None
        train = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw = _empty((n, E), x) if train else None
        db = _empty((n,), x) if train else None
        karr = (N.c_int * n)(*kinds)
        ws_bytes = query("rlt_probe_heads_workspace", n, S, B, E)
        ws = workspace(ws_bytes, x.device)
        call("rlt_probe_heads", ptr(x), ptr(w), ptr(b), karr, n, S, B, E, ptr(labels), float(margin), ptr(loss), ptr(dw),
             ptr(db), ptr(out), ptr(ws), ws_bytes, stream())
        ctx.save_for_backward(dw, db)
        if out is None:
            return loss
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, go, *_unused):
        dw, db = ctx.saved_tensors
        go = N.f32c(go)
        return None, dw * go[:, None], db * go, None, None, None, None, None, None


def probe_heads(x_pm, weights, biases, kinds, labels, S, B, margin=5e-4, want_out=True):
    """Probe heads Linear(E,1) -> Sigmoid -> BCELoss (N.PROBE_BCE) or -> Softmax over positions -> RerankLoss
    (N.PROBE_RERANK) on frozen position-major features x_pm (S*B,E); labels (B,S).  weights: list of (1,E) or (E,)
    parameters, biases: list of (1,) parameters.  Returns (losses (n,), [activations (B,S,1) per head] or None); the losses
    backpropagate into the weights and biases.  No host synchronisation.
    Labels must be exactly 0 or 1.  The rerank gradient is formed as (gpos - gneg) s_i (y_i - V), an identity that holds
    only for 0/1 labels; with other values it differs from RerankLoss's (and rlt_mt_terms'), which give such entries no
    gradient of their own.  Nothing checks this (a check would cost a host synchronisation)."""
    if x_pm.requires_grad:
        raise ValueError("probe_heads: the features must be frozen (detach them or draw them under torch.no_grad())")
    N.require_cuda(x_pm, labels)
    kinds = [int(k) for k in kinds]
    if any(k not in (N.PROBE_BCE, N.PROBE_RERANK) for k in kinds):
        raise ValueError(f"probe_heads: unknown head kind in {kinds}")
    if not (len(weights) == len(biases) == len(kinds)):
        raise ValueError("probe_heads: one weight, bias and kind per head")
    w = torch.cat([wi.reshape(1, -1) for wi in weights], dim=0) if len(weights) > 1 else weights[0].reshape(1, -1)
    b = torch.cat([bi.reshape(1) for bi in biases], dim=0) if len(biases) > 1 else biases[0].reshape(1)
    res = ProbeHeadsFn.apply(N.f32c(x_pm), N.f32c(w), N.f32c(b), N.f32c(labels), kinds, S, B, margin, bool(want_out))
    if not want_out:
        return res, None
    loss, out = res
    return loss, [out[i].unsqueeze(2) for i in range(len(kinds))]


# ------------------------------------------------------------------------------ metrics
def cut_metrics(p, labels, k_in=None, penalty=-1.0):
    """Per-list (k, F1@k, DCG@k) on device; p (B,S) or (B,S,1), labels (B,S).  Returns tensors."""
    B, S = labels.shape
    dev = labels.device
    k, f1, dcg, sums = _fused_metric_buffers(B, dev)
    call("rlt_cut_metrics_ex", ptr(p), ptr(labels), ptr(k_in), B, S, float(penalty), ptr(k), ptr(f1), ptr(dcg), ptr(sums), stream())
    return k, f1, dcg, sums


def truncation_curves(labels, penalty=-1.0, curves=None, sums=None, per_list=False):
    """The truncation curves of labels (B,S) float32 on device (rlt_truncation_curves): returns (curves (3, S+1) float64 = the
    sums over lists of F1@k, DCG@k and c_k for k = 0..S, sums (3,) float64 = sum of best F1, sum of best DCG, list count,
    per-list (best F1, its first k, best DCG, its first k) or None).  With `curves` and `sums` given, this batch is ADDED
    into them (no host synchronisation), else they are fresh."""
    if (curves is None) != (sums is None):
        raise ValueError("truncation_curves: pass both `curves` and `sums` to accumulate, or neither")
    B, S = labels.shape
    dev = labels.device
    accumulate = curves is not None
    if not accumulate:
        curves = torch.empty((3, S + 1), dtype=torch.float64, device=dev)
        sums = torch.empty((3,), dtype=torch.float64, device=dev)
    best = None
    if per_list:
        best = (torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    ws_bytes = query("rlt_truncation_curves_workspace", B, S)
    ws = workspace(ws_bytes, dev)
    bf, bfk, bd, bdk = best if per_list else (None,) * 4
    call("rlt_truncation_curves", ptr(labels), B, S, float(penalty), ptr(dcg_table(dev)), int(accumulate), ptr(curves),
         ptr(bf), ptr(bfk), ptr(bd), ptr(bdk), ptr(sums), ptr(ws), ws_bytes, stream())
    return curves, sums, best


CUT_REPORT_PER_LIST = ("k", "p_k", "margin")
CUT_REPORT_LABELLED = ("f1", "dcg", "best_f1", "best_f1_k", "best_dcg", "best_dcg_k", "better")
_CUT_REPORT_DTYPES = {"k": torch.int32, "p_k": torch.float32, "margin": torch.float32, "f1": torch.float64, "dcg": torch.float64,
                      "best_f1": torch.float64, "best_f1_k": torch.int32, "best_dcg": torch.float64, "best_dcg_k": torch.int32,
                      "better": torch.int32}


def cut_report(p, labels=None, metric=N.METRIC_F1, penalty=-1.0, metric_penalty=-1.0, tau=0.9, sharpen=None, acc=None,
               per_list=True):
    """One pass over a model's output and (optionally) the labels (rlt_cut_report).  p: the cut distribution (B,S) / (B,S,1), or
    BiCut's (B,S,2) (the PAIR rule); labels (B,S) or None for label-free mode.  Returns (per-list dict, acc): the dict holds k,
    p_k, margin and, with labels, f1, dcg, best_f1, best_f1_k, best_dcg, best_dcg_k, better (empty with per_list=False); acc is
    the dict of split sums hist (S+1), pred_curve (S), reward_curve (S), sums (5) in float64 - pass the dict of an earlier call
    back as `acc` and this batch is ADDED into it.  sharpen defaults to the reference's tau * 1e-3.  No host synchronisation."""
    p = N.f32c(p.detach())
    N.require_cuda(p, labels)
    if p.dim() == 3 and p.shape[2] == 1:
        p = p.reshape(p.shape[0], p.shape[1])
    rule = N.CUT_PAIR if p.dim() == 3 and p.shape[2] == 2 else N.CUT_ARGMAX
    if p.dim() != (3 if rule == N.CUT_PAIR else 2):
        raise ValueError(f"cut_report: the output must be (B,S), (B,S,1) or (B,S,2); got {tuple(p.shape)}")
    B, S = p.shape[:2]
    dev = p.device
    if labels is not None:
        labels = N.f32c(labels)
        if tuple(labels.shape) != (B, S):
            raise ValueError(f"cut_report: labels {tuple(labels.shape)} do not match the output's {(B, S)}")
    sharpen = float(tau) * 1e-3 if sharpen is None else float(sharpen)
    accumulate = acc is not None
    if not accumulate:
        acc = {"hist": torch.zeros((S + 1,), dtype=torch.float64, device=dev),
               "pred_curve": torch.zeros((S,), dtype=torch.float64, device=dev),
               "reward_curve": torch.zeros((S,), dtype=torch.float64, device=dev),
               "sums": torch.zeros((5,), dtype=torch.float64, device=dev)}
    elif acc["pred_curve"].numel() != S:
        raise ValueError(f"cut_report: lists of {S} positions, the accumulator holds {acc['pred_curve'].numel()}")
    names = () if not per_list else CUT_REPORT_PER_LIST + (CUT_REPORT_LABELLED if labels is not None else ())
    out = {n: torch.empty((B,), dtype=_CUT_REPORT_DTYPES[n], device=dev) for n in names}
    o = lambda n: ptr(out.get(n))
    coef = dcg_coef(S, dev) if labels is not None and metric == N.METRIC_DCG else None
    ws_bytes = query("rlt_cut_report_workspace", B, S)
    ws = workspace(ws_bytes, dev)
    call("rlt_cut_report", ptr(p), rule, ptr(labels), ptr(coef), B, S, int(metric), float(penalty), float(metric_penalty),
         float(tau), sharpen, ptr(dcg_table(dev)) if labels is not None else None, int(accumulate),
         o("k"), o("p_k"), o("margin"), o("f1"), o("dcg"), o("best_f1"), o("best_f1_k"), o("best_dcg"), o("best_dcg_k"), o("better"),
         ptr(acc["hist"]), ptr(acc["pred_curve"]), ptr(acc["reward_curve"]) if labels is not None else None, ptr(acc["sums"]),
         ptr(ws), ws_bytes, stream())
    return out, acc


SWEEP_RULES = {"quantile": N.SWEEP_QUANTILE, "score": N.SWEEP_FIRST_BELOW, "below": N.SWEEP_FIRST_BELOW,
               "above": N.SWEEP_FIRST_ABOVE}


def sweep_rule(rule):
    """'quantile' | 'score' ('below') | 'above' | an RLT_SWEEP_* code -> the code."""
    code = SWEEP_RULES.get(rule, rule)
    if code not in (N.SWEEP_QUANTILE, N.SWEEP_FIRST_BELOW, N.SWEEP_FIRST_ABOVE):
        raise ValueError(f"unknown cut rule {rule!r}: one of {sorted(SWEEP_RULES)}")
    return int(code)


def cut_sweep(v, thresholds, rule, labels=None, penalty=-1.0, beta=1.0, curve=None, want_k=True):
    """T threshold cuts of every list from one pass over v and the labels (rlt_cut_sweep).  v: (B,S) / (B,S,1) values, or
    BiCut's (B,S,2) output, whose class-0 column is then read at stride 2 without a copy; thresholds: (T,) float64 tensor on
    the device, 1 <= T <= 64; rule: 'quantile' (v a cut distribution: the smallest k whose mass reaches the share tau),
    'score' (v retrieval scores: the leading positions with v >= tau, k may be 0) or 'above' (v a stop probability: the first
    position with v >= tau).  Returns (k (B,T) int32 or None with want_k=False, curve): with labels, curve is the (8,T) float64
    sums over lists of k, F1@k, DCG@k (with `penalty`), precision, recall, F_beta, [k == S] and 1 (native.SWEEP_ROWS) - pass
    the tensor of an earlier call back as `curve` and this batch is ADDED into it; without labels it is None (label-free mode:
    only the cuts).  No host synchronisation."""
    v = N.f32c(v.detach())
    N.require_cuda(v, labels, thresholds)
    if v.dim() == 3 and v.shape[2] == 1:
        v = v.reshape(v.shape[0], v.shape[1])
    stride = 2 if v.dim() == 3 and v.shape[2] == 2 else 1
    if v.dim() != (3 if stride == 2 else 2):
        raise ValueError(f"cut_sweep: the values must be (B,S), (B,S,1) or (B,S,2); got {tuple(v.shape)}")
    B, S = v.shape[:2]
    dev = v.device
    if thresholds.dtype != torch.float64 or thresholds.dim() != 1 or not thresholds.is_contiguous():
        raise ValueError("cut_sweep: thresholds must be a contiguous 1-d float64 tensor")
    T = int(thresholds.numel())
    if not 1 <= T <= N.SWEEP_MAX_T:
        raise ValueError(f"cut_sweep: {T} thresholds, outside 1..{N.SWEEP_MAX_T}")
    code = sweep_rule(rule)
    if labels is None:
        if curve is not None or not want_k:
            raise ValueError("cut_sweep: without labels only the cuts are produced (curve=None, want_k=True)")
    else:
        labels = N.f32c(labels)
        if tuple(labels.shape) != (B, S):
            raise ValueError(f"cut_sweep: labels {tuple(labels.shape)} do not match the values' {(B, S)}")
    accumulate = curve is not None
    if labels is not None and not accumulate:
        curve = torch.empty((N.SWEEP_COLS, T), dtype=torch.float64, device=dev)
    elif accumulate and (tuple(curve.shape) != (N.SWEEP_COLS, T) or curve.dtype != torch.float64 or not curve.is_contiguous()):
        raise ValueError(f"cut_sweep: the accumulator must be a contiguous ({N.SWEEP_COLS},{T}) float64 tensor")
    k = torch.empty((B, T), dtype=torch.int32, device=dev) if want_k else None
    ws, ws_bytes = None, 0
    if labels is not None:
        ws_bytes = query("rlt_cut_sweep_workspace", B, S, T)
        ws = workspace(ws_bytes, dev)
    call("rlt_cut_sweep", ptr(v), stride, code, ptr(thresholds), T, ptr(labels), B, S, float(penalty), float(beta),
         ptr(dcg_table(dev)) if labels is not None else None, int(accumulate), ptr(k), ptr(curve), ptr(ws), ws_bytes, stream())
    return k, curve


RERANK_MAX_ARRAYS = 4


def rerank_lists(pred, *arrays, want_perm=True, want_rank=False, want_sorted=False):
    """Stable per-list sort by descending `pred` with up to four companion arrays carried along (rlt_rerank_lists).  pred: (B,S)
    or (B,S,1) head values; arrays: (B,S) / (B,S,1) tensors - labels, retrieval scores, the cut distribution.  The order of a
    list is np.argsort(-pred[b], kind="stable"): NaNs last, +0 and -0 tied.  Returns (perm, rank, sorted_pred, [permuted arrays]):
    perm (B,S) int32 = original index at each new position, rank its inverse, sorted_pred = pred in the new order, each None
    unless asked for; the permuted arrays are fresh (B,S) fp32 tensors with the same bits.  Tensors in and out, no host read.
    Not a tape node: an input that requires grad under grad mode raises."""
    if len(arrays) > RERANK_MAX_ARRAYS:
        raise ValueError(f"rerank_lists: {len(arrays)} companion arrays, at most {RERANK_MAX_ARRAYS}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (pred,) + arrays):
        raise RuntimeError("rerank_lists is not differentiable: detach the inputs or call it under torch.no_grad()")
    N.require_cuda(pred, *arrays)

    def rows(t, what):
        t = N.f32c(t.detach())
        if t.dim() == 3 and t.shape[2] == 1:
            t = t.reshape(t.shape[0], t.shape[1])
        if t.dim() != 2:
            raise ValueError(f"rerank_lists: {what} must be (B,S) or (B,S,1); got {tuple(t.shape)}")
        return t
    pred = rows(pred, "pred")
    B, S = pred.shape
    dev = pred.device
    src = [rows(t, "a companion array") for t in arrays]
    for t in src:
        if tuple(t.shape) != (B, S):
            raise ValueError(f"rerank_lists: a companion array {tuple(t.shape)} does not match pred's {(B, S)}")
    if not (src or want_perm or want_rank or want_sorted):
        raise ValueError("rerank_lists: nothing asked for")
    dst = [torch.empty_like(t) for t in src]
    perm = torch.empty((B, S), dtype=torch.int32, device=dev) if want_perm else None
    rank = torch.empty((B, S), dtype=torch.int32, device=dev) if want_rank else None
    sorted_pred = _empty((B, S), pred) if want_sorted else None
    call("rlt_rerank_lists", ptr(pred), B, S, N.pointer_array(src) if src else None, N.pointer_array(dst) if dst else None,
         len(src), ptr(perm), ptr(rank), ptr(sorted_pred), stream())
    return perm, rank, sorted_pred, dst


def neighbor_features(doc_ids, table, out=None, col=0, validate=True):
    """AttnCut's neighbour-similarity statistics (rlt_neighbor_features): doc_ids (B,S) int32 rows of `table` in rank order ->
    per position the cosine similarity to the neighbouring documents, the tf-idf column first, then the doc2vec one.
    `table`: an object with `n_docs`, `d2v` ((n_docs,D) float32 or None) and `indptr` / `indices` / `values` (int64 / int32 /
    float64 CSR, or None) on the device of doc_ids - dataloader.doc_features.DocTable.to(device) is one.  `out`: a float32
    tensor (B,S,F) whose columns col.. receive the result in place (F = 3, col = 1: the packed model input), or None for a
    fresh (B,S,columns).  An id outside [0, n_docs) raises ValueError; that test is the one host synchronisation here and
    `validate=False` leaves it out for ids the caller built from the table's own map."""
    if doc_ids.dim() != 2 or doc_ids.dtype != torch.int32:
        raise ValueError("neighbor_features: doc_ids must be a (B, S) int32 tensor")
    B, S = doc_ids.shape
    if B < 1 or S < 2:
        raise ValueError(f"neighbor_features: needs at least one list of at least 2 documents, got {B} x {S}")
    d2v, indptr, indices, values = table.d2v, table.indptr, table.indices, table.values
    if d2v is None and indptr is None:
        raise ValueError("neighbor_features: the table holds neither tf-idf rows nor doc2vec rows")
    N.require_cuda(doc_ids, d2v, indptr, indices, values, out)
    n_docs = int(table.n_docs)
    if d2v is not None and (d2v.dtype != torch.float32 or d2v.dim() != 2 or d2v.shape[0] != n_docs or d2v.stride(1) != 1):
        raise ValueError("neighbor_features: d2v must be (n_docs, D) float32 with unit column stride")
    if indptr is not None and (indptr.dtype != torch.int64 or indices.dtype != torch.int32 or values.dtype != torch.float64
                               or indptr.numel() != n_docs + 1 or not (indptr.is_contiguous() and indices.is_contiguous()
                                                                       and values.is_contiguous())):
        raise ValueError("neighbor_features: CSR arrays must be contiguous indptr (n_docs+1) int64, indices int32, values float64")
    doc_ids = doc_ids if doc_ids.is_contiguous() else doc_ids.contiguous()
    if validate:
        lo, hi = torch.aminmax(doc_ids)
        if int(lo) < 0 or int(hi) >= n_docs:
            raise ValueError(f"neighbor_features: document row outside [0, {n_docs}): min {int(lo)}, max {int(hi)}")
    ncol = (d2v is not None) + (indptr is not None)
    if out is None:
        out = torch.empty((B, S, ncol), dtype=torch.float32, device=doc_ids.device)
        col = 0
    if out.dtype != torch.float32 or out.dim() != 3 or tuple(out.shape[:2]) != (B, S) or out.stride(2) != 1 \
            or (B > 1 and out.stride(0) != S * out.stride(1)) or col < 0 or col + ncol > out.shape[2]:
        raise ValueError(f"neighbor_features: out must be float32 (B, S, F) with rows of equal stride and F >= col + {ncol}")
    call("rlt_neighbor_features", ptr(doc_ids), B, S, n_docs, ptr(d2v), 0 if d2v is None else d2v.shape[1],
         0 if d2v is None else d2v.stride(0), ptr(indptr), ptr(indices), ptr(values), ptr(out), out.stride(1), int(col), stream())
    return out


def reward_matrix(labels, metric, tau=1.0, want_q=False, penalty=-1.0):
    B, S = labels.shape
    coef = dcg_coef(S, labels.device) if metric == N.METRIC_DCG else None
    r = _empty((B, S), labels)
    q = _empty((B, S), labels) if want_q else None
    call("rlt_reward_matrix_ex", ptr(labels), ptr(coef), B, S, metric, float(penalty), tau, ptr(r), ptr(q), stream())
    return (r, q) if want_q else r


def reward_spec_matrix(labels, spec, tau=1.0, want_q=False):
    """The (B,S) fp32 reward of a spec (utils.rewards.RewardSpec) and, with `want_q`, q = softmax(r / tau)."""
    B, S = labels.shape
    struct, keep = spec.native(S, labels.device)
    table = dcg_table(labels.device) if struct.family == N.REWARD_GAIN and struct.discount is None else None
    r = _empty((B, S), labels)
    q = _empty((B, S), labels) if want_q else None
    call("rlt_reward_spec_matrix", ptr(labels), B, S, N.ctypes.byref(struct), float(tau), ptr(table), ptr(r), ptr(q), stream())
    del keep
    return (r, q) if want_q else r


def reward_eval(labels=None, spec=None, r=None, k=None, allow_empty=True, acc=None, per_list=True, split=True):
    """One evaluation pass over a reward row (rlt_reward_eval).  The reward: `labels` (B,S) + `spec` (utils.rewards.RewardSpec),
    or `r`, a (B,S) fp32 matrix.  k: (B,T) / (B,) int32 cuts of T rules or systems on the same lists, or None.  Returns
    (per-list dict, acc): the dict holds best (B) fp32 and best_k (B) int32 - the row's largest reward over kmin..S, kmin = 0 with
    allow_empty, and its first position - and, with cuts, r_at (B,T) fp32 and better (B,T) int32 (empty with per_list=False);
    acc is the dict of float64 split sums curve (S+1), best_hist (S+1), sums (3 + 3T: lists, sum best, clamped cuts, then per
    cut sum r_at, #(r_at == best), sum better) - pass the dict of an earlier call back as `acc` and this batch is ADDED into it;
    with split=False no split sum is formed and acc is None (`acc` must then be None too).  Tensors in and out, no host read."""
    if (labels is None) == (r is None) or (labels is None) != (spec is None):
        raise ValueError("reward_eval: the reward is labels + spec, or a matrix r")
    rows = N.f32c(labels if r is None else r)
    N.require_cuda(rows, k)
    if rows.dim() != 2:
        raise ValueError(f"reward_eval: rows must be (B,S); got {tuple(rows.shape)}")
    B, S = rows.shape
    dev = rows.device
    T = 0
    if k is not None:
        k = k.reshape(B, -1)
        k = k if k.dtype == torch.int32 and k.is_contiguous() else k.to(torch.int32).contiguous()
        T = int(k.shape[1])
        if not 1 <= T <= N.SWEEP_MAX_T:
            raise ValueError(f"reward_eval: {T} cuts per list, outside 1..{N.SWEEP_MAX_T}")
    struct = keep = table = None
    if spec is not None:
        struct, keep = spec.native(S, dev)
        table = dcg_table(dev) if struct.family == N.REWARD_GAIN and struct.discount is None else None
    accumulate = acc is not None
    if accumulate and not split:
        raise ValueError("reward_eval: an accumulator was passed with split=False")
    if split and not accumulate:
        acc = {"curve": torch.zeros((S + 1,), dtype=torch.float64, device=dev),
               "best_hist": torch.zeros((S + 1,), dtype=torch.float64, device=dev),
               "sums": torch.zeros((3 + 3 * T,), dtype=torch.float64, device=dev)}
    elif accumulate and (acc["curve"].numel() != S + 1 or acc["sums"].numel() != 3 + 3 * T):
        raise ValueError(f"reward_eval: lists of {S} positions with {T} cuts do not fit the accumulator")
    out = {}
    if per_list:
        out = {"best": torch.empty((B,), dtype=torch.float32, device=dev), "best_k": torch.empty((B,), dtype=torch.int32, device=dev)}
        if T:
            out["r_at"] = torch.empty((B, T), dtype=torch.float32, device=dev)
            out["better"] = torch.empty((B, T), dtype=torch.int32, device=dev)
    if not out and acc is None:
        raise ValueError("reward_eval: nothing asked for (per_list=False, split=False)")
    o = lambda n: ptr(out.get(n))
    s = lambda n: ptr(acc[n]) if acc is not None else None
    ws_bytes = query("rlt_reward_eval_workspace", B, S, T)
    ws = workspace(ws_bytes, dev)
    call("rlt_reward_eval", ptr(rows) if r is None else None, None if struct is None else N.ctypes.byref(struct),
         ptr(rows) if r is not None else None, B, S, ptr(k), T, int(bool(allow_empty)), ptr(table), int(accumulate),
         o("r_at"), o("better"), o("best"), o("best_k"), s("curve"), s("best_hist"), s("sums"), ptr(ws), ws_bytes, stream())
    del keep
    return out, acc


# ------------------------------------------------------------------------------ optimizer
def grad_norm(flat_grad, offsets=None, max_norm=None, state=None):
    """rlt_grad_norm on a flat fp32 gradient bucket (numel % 4 == 0, on the GPU) in one read; no host synchronisation.
    offsets: (n_seg + 1) int64 DEVICE tensor of ascending multiples of 4 from 0 to numel - FlatModel.offsets - for per-segment
    figures, None for the bucket alone.  max_norm None / 0 / inf: no clipping (coef == 1).  state: an rlt_opt_state
    (N.OPT_STATE_WORDS int64 zeros, device) to update, a fresh one otherwise.
    Returns a dict of device tensors: norm, sumsq, max_abs (float64), coef (float32), nonfinite (int64), `state` itself, and
    with offsets seg_sumsq, seg_max_abs (float64), seg_nonfinite (int64)."""
    N.require_cuda(flat_grad, offsets)
    if flat_grad.dtype != torch.float32 or flat_grad.dim() != 1 or not flat_grad.is_contiguous():
        raise ValueError("grad_norm: a contiguous 1-D float32 bucket is required")
    dev, n = flat_grad.device, flat_grad.numel()
    n_seg = 0
    if offsets is not None:
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
            raise ValueError("grad_norm: offsets must be a contiguous int64 vector of n_seg + 1 entries")
        n_seg = offsets.numel() - 1
    if state is None:
        state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device=dev)
    seg = torch.zeros(max(n_seg, 1), N.GRAD_SEG_WORDS, dtype=torch.int64, device=dev)
    ws_bytes = query("rlt_grad_norm_workspace", n, n_seg)
    ws = N.byte_buffer(ws_bytes, dev)
    call("rlt_grad_norm", ptr(flat_grad), n, ptr(offsets), n_seg, float(max_norm or 0.0), ptr(ws), ws_bytes, ptr(seg), ptr(state),
         stream())
    f64 = state.view(torch.float64)
    out = {"norm": f64[N.OPT_NORM], "sumsq": f64[N.OPT_SUMSQ], "max_abs": f64[N.OPT_MAX_ABS],
           "coef": state.view(torch.float32)[N.OPT_COEF_F32], "nonfinite": state[N.OPT_NONFINITE], "state": state}
    if n_seg:
        seg64 = seg.view(torch.float64)
        out.update(seg_sumsq=seg64[:, 0], seg_nonfinite=seg[:, 1], seg_max_abs=seg64[:, 2])
    return out


def paired_compare(base, systems, resamples, seed, keep_stats=True):
    """rlt_paired_compare: the paired randomization test and the paired bootstrap of M systems against a baseline on the same
    Q queries.  base (Q,), systems (M, Q) or (Q,) float32 on the GPU, in one query order; `resamples` replicates of each test from
    the 32-bit `seed`.  Returns a dict of device tensors - record (M, N.CMP_WORDS) int64 (the float64 words through
    .view(torch.float64)), and with keep_stats rand_stat and boot_stat (M, resamples) float64, else None.  No host synchronisation."""
    N.require_cuda(base, systems)
    if systems.dim() == 1:
        systems = systems.unsqueeze(0)
    if base.dim() != 1 or systems.dim() != 2 or systems.shape[1] != base.numel():
        raise ValueError(f"paired_compare: base (Q,) and systems (M, Q) expected; got {tuple(base.shape)} and {tuple(systems.shape)}")
    base, systems = N.f32c(base.detach()), N.f32c(systems.detach())
    M, Q = systems.shape
    R = int(resamples)
    dev = base.device
    record = torch.empty((M, N.CMP_WORDS), dtype=torch.int64, device=dev)
    rand_stat = torch.empty((M, R), dtype=torch.float64, device=dev) if keep_stats else None
    boot_stat = torch.empty((M, R), dtype=torch.float64, device=dev) if keep_stats else None
    ws_bytes = query("rlt_paired_compare_workspace", Q, M, R)
    if ws_bytes == 0:
        raise ValueError(f"paired_compare: 1 <= Q <= {N.CMP_MAX_Q}, 1 <= M <= {N.CMP_MAX_SYSTEMS}, 0 <= resamples <= {N.CMP_MAX_R}; "
                         f"got Q = {Q}, M = {M}, resamples = {R}")
    ws = N.byte_buffer(ws_bytes, dev)
    call("rlt_paired_compare", ptr(base), ptr(systems), Q, Q, M, R, int(seed) & 0xFFFFFFFF, ptr(ws), ws_bytes, ptr(record),
         ptr(rand_stat) if keep_stats and R else None, ptr(boot_stat) if keep_stats and R else None, stream())
    return {"record": record, "rand_stat": rand_stat, "boot_stat": boot_stat}
