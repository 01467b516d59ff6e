"""rlt_seq_attention_append (csrc/attention_seq_append.hip) through the raw C ABI: one random qkv (S*B, 3E) goes through
rlt_seq_attention_fwd_ex with RLT_SEQ_MASK_CAUSAL, then the same rows are fed to the append kernel chunk by chunk.

  zero tolerance   out and lse of every chunking equal the one-shot call's as fp32 VALUES (np.array_equal: +0 == -0, the one thing
                   the zero-staged rows behind the chunk may change); after the last chunk the cache IS the K | V columns of qkv
  restatement      the same ids against tests/seq_causal_restate.py in float64, at the bound tests/test_seq_causal_gpu.py holds the
                   one-shot kernel to (relative max-norm FWD_TOL for out, lse_bound per row)
  retired lists    active = [1, 0, 1]: list 1's out, lse and cache rows keep their NaN sentinel, lists 0 and 2 keep their bits
  the cache        rows >= t0+C, NaN before the call, are neither read nor written; two calls give the same bits"""
import functools
import math

import numpy as np
import pytest
import torch

import seq_attention_restate as R
import seq_causal_restate as C

pytestmark = pytest.mark.gpu
CAUSAL = 1
HEADS = ((64, 1), (64, 2), (16, 3), (16, 4), (16, 5))          # (HD, H): H = 3, 5 at head dim 16 leave a narrower last group
LENGTHS = (1, 31, 32, 33, 64, 65, 127, 128, 129, 300)
SHAPES = [(S, B, H, HD) for HD, H in HEADS for S in LENGTHS for B in (1, 3)]
ids = lambda s: "S%d-B%d-H%d-HD%d" % s


def chunkings(S):
    """name -> chunk sizes summing to S: all-1s, 7s, 32s, 33s, 64s, one chunk, and an uneven sequence whose second chunk crosses a
    32-boundary and whose third crosses a 64- and a 128-boundary in the middle"""
    def fixed(c):
        return [min(c, S - t) for t in range(0, S, c)]
    uneven, t = [], 0
    for c in (5, 40, 100, 17, S):
        if t < S:
            uneven.append(min(c, S - t))
            t += uneven[-1]
    return {"ones": fixed(1), "sevens": fixed(7), "32s": fixed(32), "33s": fixed(33), "64s": fixed(64), "whole": [S], "uneven": uneven}


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def one_shot(N, qkv_d, S, B, H, HD):
    from rlt_hip.native import ptr
    out, lse = nan(S * B, H * HD), nan(B, H, S)
    N.call("rlt_seq_attention_fwd_ex", ptr(qkv_d), S, B, H, HD, 0.0, 0, CAUSAL, ptr(out), ptr(lse), N.PRECISION_FP32, N.stream())
    return out, lse


def append_all(N, qkv_d, chunks, S, B, H, HD, Smax=None, active=None, cache=None, prec=None, after=None):
    """feed the rows chunk by chunk -> out (S*B, E), lse (B, H, S), cache (Smax*B, 2E) on the device; buffers start as NaN.
    after(t0, C, cache): called behind every chunk."""
    from rlt_hip.native import ptr
    E = H * HD
    Smax = S if Smax is None else Smax
    cache = nan(Smax * B, 2 * E) if cache is None else cache
    out, lse = nan(S * B, E), nan(B, H, S)
    t0 = 0
    for c in chunks:
        chunk = qkv_d[t0 * B:(t0 + c) * B]
        o, l = nan(c * B, E), nan(B, H, c)
        N.call("rlt_seq_attention_append", ptr(chunk), ptr(cache), t0, c, Smax, B, H, HD, ptr(active), ptr(o), ptr(l),
               N.PRECISION_DEFAULT if prec is None else prec, N.stream())
        out[t0 * B:(t0 + c) * B] = o
        lse[:, :, t0:t0 + c] = l
        if after is not None:
            after(t0, c, cache)
        t0 += c
    assert t0 == S
    return out, lse, cache


@functools.lru_cache(maxsize=None)
def inputs(shape):
    qkv, _ = C.inputs("randn", *shape)
    qkv.setflags(write=False)
    return qkv


# ------------------------------------------------------------------------------------------------ 1. zero tolerance, and fp64
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_every_chunking_equals_the_one_shot_forward_and_the_restatement(N, shape):
    S, B, H, HD = shape
    E = H * HD
    qkv = inputs(shape)
    qkv_d = torch.from_numpy(qkv).to(dev())
    o1, l1 = one_shot(N, qkv_d, *shape)
    o1, l1 = o1.cpu().numpy(), l1.cpu().numpy()
    assert np.isfinite(o1).all() and np.isfinite(l1).all()
    got = None
    for name, chunks in chunkings(S).items():
        out, lse, cache = (t.cpu().numpy() for t in append_all(N, qkv_d, chunks, *shape))
        assert np.array_equal(out, o1), (name, "out", float(np.abs(out - o1).max()))
        assert np.array_equal(lse, l1), (name, "lse", float(np.abs(lse - l1).max()))
        assert np.array_equal(cache.view(np.uint32), qkv[:, E:].view(np.uint32)), (name, "cache")     # K | V, bit for bit
        got = out, lse
    # the same id against float64, at the one-shot kernel's bound
    o_ref, l_ref, _ = C.forward(qkv, S, B, H, HD)
    q, k, _ = R.heads(qkv, S, B, H, HD)
    score_max = np.where(C.causal(S), np.abs(q @ k.transpose(0, 1, 3, 2)), 0.0).max(-1) / math.sqrt(HD)
    errs = {"out": R.rel(got[0].astype(np.float64), o_ref),
            "lse": float((np.abs(got[1].astype(np.float64) - l_ref) / R.lse_bound(l_ref, score_max)).max())}
    print(shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["out"] < R.FWD_TOL and errs["lse"] <= 1.0, errs


@pytest.mark.parametrize("prec", ("fp32", "bf16x6", "bf16x3"))
def test_the_three_precision_codes_run_the_same_kernel(N, prec):
    shape = (65, 3, 5, 16)
    qkv_d = torch.from_numpy(inputs(shape)).to(dev())
    o1, l1 = one_shot(N, qkv_d, *shape)
    out, lse, _ = append_all(N, qkv_d, chunkings(65)["sevens"], *shape, prec=N.precision_code(prec))
    assert np.array_equal(out.cpu().numpy(), o1.cpu().numpy()) and np.array_equal(lse.cpu().numpy(), l1.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 2. retired lists
@pytest.mark.parametrize("shape", [(129, 3, 2, 64), (65, 3, 5, 16)], ids=ids)
def test_a_retired_list_is_not_touched(N, shape):
    S, B, H, HD = shape
    E = H * HD
    qkv_d = torch.from_numpy(inputs(shape)).to(dev())
    chunks = chunkings(S)["uneven"]
    full = [t.cpu().numpy() for t in append_all(N, qkv_d, chunks, *shape)]
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev())
    out, lse, cache = (t.cpu().numpy() for t in append_all(N, qkv_d, chunks, *shape, active=active))
    assert active.tolist() == [1, 0, 1]                                                  # read only
    out, cache, fo, fc = (a.reshape(S, B, -1) for a in (out, cache, full[0], full[2]))
    assert np.isnan(out[:, 1]).all() and np.isnan(lse[1]).all() and np.isnan(cache[:, 1]).all()
    for b in (0, 2):
        assert np.array_equal(out[:, b].view(np.uint32), fo[:, b].view(np.uint32))
        assert np.array_equal(lse[b].view(np.uint32), full[1][b].view(np.uint32))
        assert np.array_equal(cache[:, b].view(np.uint32), fc[:, b].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. the cache behind the chunk
@pytest.mark.parametrize("shape", [(70, 3, 1, 64), (70, 3, 3, 16)], ids=ids)
def test_cache_rows_behind_the_chunk_are_neither_read_nor_written(N, shape):
    S, B, H, HD = shape
    E = H * HD
    Smax = S + 9
    qkv = inputs(shape)
    qkv_d = torch.from_numpy(qkv).to(dev())
    o1, l1 = one_shot(N, qkv_d, *shape)

    def after(t0, c, cache):
        rows = cache.view(Smax, B, 2 * E)
        assert bool(torch.isnan(rows[t0 + c:]).all()), (t0, c)                          # not written
        assert bool(torch.isfinite(rows[:t0 + c]).all()), (t0, c)

    out, lse, cache = append_all(N, qkv_d, [3, 30, 1, 36], *shape, Smax=Smax, after=after)
    # not read: with NaN behind every chunk the outputs are finite and those of the one-shot call
    assert np.array_equal(out.cpu().numpy(), o1.cpu().numpy()) and np.array_equal(lse.cpu().numpy(), l1.cpu().numpy())
    assert np.array_equal(cache.cpu().numpy()[:S * B].view(np.uint32), qkv[:, E:].view(np.uint32))


def test_two_calls_give_the_same_bits(N):
    shape = (129, 3, 4, 16)
    qkv_d = torch.from_numpy(inputs(shape)).to(dev())
    a = append_all(N, qkv_d, chunkings(129)["33s"], *shape)
    b = append_all(N, qkv_d, chunkings(129)["33s"], *shape)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))


def test_the_python_wrapper(N):
    from rlt_hip import ops
    S, B, H, HD = shape = (40, 3, 2, 64)
    E = H * HD
    qkv_d = torch.from_numpy(inputs(shape)).to(dev())
    o1, l1 = one_shot(N, qkv_d, *shape)
    cache = torch.empty(S * B, 2 * E, device=dev())
    out, lse = ops.seq_attention_append(qkv_d[:33 * B].contiguous(), cache, 0, 33, S, B, H, want_lse=True)
    out2 = ops.seq_attention_append(qkv_d[33 * B:].contiguous(), cache, 33, 7, S, B, H)
    assert torch.equal(torch.cat([out, out2]), o1) and torch.equal(lse, l1[:, :, :33])
    with pytest.raises(ValueError):
        ops.seq_attention_append(qkv_d[:B].contiguous(), cache, 40, 1, S, B, H)           # past the cache
    with pytest.raises(ValueError):
        ops.seq_attention_append(qkv_d[:B].contiguous(), cache[:-1], 0, 1, S, B, H)
    with pytest.raises(ValueError):
        ops.seq_attention_append(qkv_d[:B].contiguous(), cache, 0, 1, S, B, H, active=torch.ones(B, device=dev()))
