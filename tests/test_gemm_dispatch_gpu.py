"""Every dispatch branch of the GEMM family (csrc/gemm.hip and the family files it dispatches to: gemm_f32, gemm3, gemm6, gemm6c, gemm6e, gemm6s) through the raw C ABI (rlt_hip.native), `pytest -m gpu`.
One test id per (kernel family, operand layout, variant, operand kind; the table: tests/gemm_cases.py); the id names the branch, and
rlt_gemm_last_dispatch - what the library itself recorded where it launched, and what rlt_gemm_plan returns for the same call - is
ASSERTED against it, so a moved threshold fails with "expected gemm6b, got
gemm6c" instead of silently moving coverage.  The precision mode is the call's argument; no environment switch is read or set here.

Operand kinds (the last component of an id), all through the same launch shape:
  int     small integers, |a|, |b| <= 7                                       } exact: every element must EQUAL the float64 reference,
  wideA   A wide, B from {-1, 0, 1} with <= 16 non-zeros per output element   } zero tolerance (tests/gemm_operands.py states the
  wideB   B wide, A from {-1, 0, 1}                                           } operands and why they are exact; test_gemm_operands.py)
  full    randn, and randn with the low 16 significand bits forced to ones (tools/gpu_probe.py _low_mantissa), against float64:
          max |C - ref| <= (2e-6 sqrt(K) + 1e-6) max |ref| for fp32 and bf16x6, six times that for bf16x3 (the probe's mfma_tol), and for
          bf16x6 the probe's x6_adversarial criterion against the exact-fp32 mode run on the same operands:
          err_x6 <= 1.25 err_fp32 + min(sqrt(K) 2^-25, 2 err_fp32) + 2^-27, err = max |C - ref| / max sum_k |a b|.
The non-zeros of the sign operand: one in the first K tile, one in the last (short) one - so in the last K slab, the z tail of the
reduce - and one in each sixteenth of K between them; that reaches every slab up to 16 of them, and at most 16 of the 24 / 121 slabs
of the two long-K cases per output element (the slabs differ from element to element; the dense `int` kind has terms in all of them);
with a fused column sum of A the wide A itself is the sparse one (16 non-zeros per row of op(A), B dense +-1), so that the column
sums stay exact as well.  Integer bias, bias2, C0 (accumulate), ReLU, relu_mask, mask_scale = 1.25 and drop_p = 0.5 keep the result
exact: the two scales are one fp32 multiplication of an exact value, restated in float64 and rounded once.

Memory safety, every id: A and B are stored with padded leading dimensions, the padding is NaN; C has ldc > N and three extra rows, the
column sum and the bit words a tail - all sentinels, none of which may change.
"""
import functools
import math
import zlib

import pytest
import torch

import gemm_operands as G
from gemm_cases import ACC, CASES, LAYOUTS, MODES, RELU

pytestmark = pytest.mark.gpu

SENT = -12345.0
BITS_SENT = 0x5A5A5A5A
KINDS = ("int", "wideA", "wideB", "full")
E_WORKSPACE = -3


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rlt_hip import native
    native.load()
    # before any launch, on the CPU: the pools the exact operands are drawn from split exactly and fill every plane
    G.check_small()
    for mode in MODES:
        G.check_pool(mode, G.wide_pool(mode))
    return native


# ---------------------------------------------------------------------------------------------------------------- operands
def _gen(*key):
    g = torch.Generator(device="cuda")
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _ints(g, shape, lim=G.SMALL_MAX):
    return torch.randint(-lim, lim + 1, shape, generator=g, device="cuda").float()


def _wide(g, shape, mode):
    lo, hi = G.WIDE_RANGE[mode]
    v = 2 * torch.randint(lo // 2, hi // 2, shape, generator=g, device="cuda") + 1
    return (v * (2 * torch.randint(0, 2, shape, generator=g, device="cuda") - 1)).float()


def _sparse_sign(g, rows, K):
    """rows x K of {-1, 0, 1}, at most MAX_NNZ non-zeros per row: one in the first K tile, one in the last (short) tile, one in each
    sixteenth of K between them"""
    n = min(K, G.MAX_NNZ)
    u = torch.rand((rows, n), generator=g, device="cuda")
    pos = ((torch.arange(n, device="cuda") + u) * (K / n)).long().clamp_(max=K - 1)
    first = min(32, K)
    last0 = (K - 1) // 32 * 32
    pos[:, 0] = torch.randint(0, first, (rows,), generator=g, device="cuda")
    pos[:, -1] = torch.randint(last0, K, (rows,), generator=g, device="cuda")
    sgn = (2 * torch.randint(0, 2, (rows, n), generator=g, device="cuda") - 1).float()
    return torch.zeros(rows, K, device="cuda").scatter_(1, pos, sgn)


def _low_mantissa(x, pattern=0xFFFF):
    return ((x.contiguous().view(torch.int32) & ~0xFFFF) | pattern).view(torch.float32)


@functools.lru_cache(maxsize=8)
def operands(mode_class, M, Nn, K, kind, sparse_wide):
    """logical A (M x K), B (K x N) as fp32 and the float64 products A B and |A| |B| (the term scale), shared between the ids of a shape.
    mode_class: the wide pool (bf16x3 has its own).  -> list of (A, B, A B, max |A| |B|) - two entries for `full`."""
    g = _gen(mode_class, M, Nn, K, kind)
    if kind == "int":
        pairs = [(_ints(g, (M, K)), _ints(g, (K, Nn)))]
        G.check_sum_bound(G.SMALL_MAX, G.SMALL_MAX, K, extra=3 * G.SMALL_MAX)
    elif kind in ("wideA", "wideB"):
        if kind == "wideA":
            if sparse_wide:
                A, B = _wide(g, (M, K), mode_class) * _sparse_sign(g, M, K).abs(), (2 * torch.randint(0, 2, (K, Nn), generator=g, device="cuda") - 1).float()
                terms = int((A != 0).sum(1).max())
            else:
                A, B = _wide(g, (M, K), mode_class), _sparse_sign(g, Nn, K).t().contiguous()
                terms = int((B != 0).sum(0).max())
            wide, sign = A, B
        else:
            A, B = _sparse_sign(g, M, K), _wide(g, (K, Nn), mode_class)
            terms = int((A != 0).sum(1).max())
            wide, sign = B, A
        # on the host, before any launch: the drawn values are in the checked pool, the sign operand is one, the sums stay integers of fp32
        lo, hi = G.WIDE_RANGE[mode_class]
        w = wide[wide != 0].abs()
        assert float(w.min()) >= lo and float(w.max()) < hi and bool((w.long() % 2 == 1).all())
        assert float(sign.abs().max()) == 1.0 and 1 <= terms <= G.MAX_NNZ
        G.check_sum_bound(float(w.max()), 1, terms, extra=3 * G.SMALL_MAX)
        pairs = [(A, B)]
    else:
        A, B = torch.randn((M, K), generator=g, device="cuda"), torch.randn((K, Nn), generator=g, device="cuda")
        pairs = [(A, B), (_low_mantissa(A), _low_mantissa(B))]
    out = []
    for A, B in pairs:
        Ad, Bd = A.double(), B.double()
        out.append((A, B, Ad @ Bd, float((Ad.abs() @ Bd.abs()).max())))
    return out


def store(logical, transposed, ld_pad, off):
    """the operand as the library reads it: op stored [rows][ld], ld = rows' length rounded up to 4 + ld_pad, NaN in the padding, the
    pointer `off` floats behind a 512-byte aligned allocation.  -> (tensor whose data_ptr is the operand, ld, the whole buffer)"""
    m = logical.t() if transposed else logical
    rows, cols = m.shape
    ld = (cols + 3) // 4 * 4 + ld_pad
    buf = torch.full((off + rows * ld + 8,), float("nan"), device="cuda")
    view = buf[off:off + rows * ld].view(rows, ld)
    view[:, :cols] = m
    return view, ld, buf


def unpack_bits(words, M, Nn):
    w = words[:(M + 31) // 32 * Nn].view(-1, Nn)
    r = torch.arange(M, device="cuda")
    return ((w[r >> 5] >> (r & 31).unsqueeze(1)) & 1).bool()


# ---------------------------------------------------------------------------------------------------------------- one launch
def launch(N, c, A, B, epi, precision, ws_mode=None):
    """-> dict(rc, C (M x N view), Cbuf, colsum, bits, dispatch)"""
    M, Nn, K, ta, tb = c["M"], c["N"], c["K"], c["ta"], c["tb"]
    Av, lda, _a = store(A, ta, c.get("lda_pad", 4), c.get("a_off", 0))
    Bv, ldb, _b = store(B, tb, c.get("ldb_pad", 4), c.get("b_off", 0))
    ldc = (Nn + 3) // 4 * 4 + 4
    Cbuf = torch.full((M + 3, ldc), SENT, device="cuda")
    if c.get("acc"):
        Cbuf[:M, :Nn] = epi["C0"]
    flags = (RELU if c.get("relu") else 0) | (ACC if c.get("acc") else 0)
    boff = c.get("bias_off", 0)
    bias = bias2 = None
    if c.get("bias"):
        bias = torch.empty(Nn + boff, device="cuda")[boff:].copy_(epi["bias"])
    if c.get("bias2"):
        bias2 = epi["bias2"].clone()
    ws_mode = ws_mode or c.get("ws", "query")
    nbytes = N.query("rlt_gemm_workspace", ta, tb, M, Nn, K)
    if ws_mode == "null":
        assert nbytes > 0, "the case is about a shape that wants split-K"
        ws, ws_bytes = None, 0
    elif ws_mode == "small":
        assert nbytes > 0
        ws, ws_bytes = torch.full((nbytes // 4 + 16,), SENT, device="cuda"), nbytes - 4
    else:
        ws, ws_bytes = torch.full((nbytes // 4 + 16,), SENT, device="cuda"), nbytes
    colsum = torch.full((M + 8,), SENT, device="cuda") if c.get("colsum") else None
    bits = None
    if c.get("bits"):
        nw = N.query("rlt_gemm_bits_words", M, Nn)
        assert nw == (M + 31) // 32 * Nn
        bits = torch.full((nw + 64,), BITS_SENT, dtype=torch.int32, device="cuda")
        if c["bits"] == "in":
            bits[:nw] = epi["bits_in"]
    mask = None
    if c.get("mask"):
        mask = torch.full((M, Nn + 3), float("nan"), device="cuda")
        mask[:, :Nn] = epi["mask"]
    drop_p, seed = (0.5, 4242) if c.get("drop") else (0.0, 0)
    lib = N.load()
    head = (ta, tb, M, Nn, K, N.ptr(Av), lda, N.ptr(Bv), ldb, N.ptr(Cbuf), ldc)
    if bits is not None:
        rc = lib.rlt_gemm_bits(*head, N.ptr(bias), flags, drop_p, seed, N.ptr(bits) if c["bits"] == "out" else None,
                               N.ptr(bits) if c["bits"] == "in" else None, 1.25, precision, N.stream())
    elif mask is not None or colsum is not None or drop_p:
        rc = lib.rlt_gemm_ex(*head, N.ptr(bias), N.ptr(bias2), flags, N.ptr(mask), Nn + 3, 1.25, N.ptr(colsum), drop_p, seed,
                             N.ptr(ws), ws_bytes, precision, N.stream())
    else:
        rc = lib.rlt_gemm(*head, N.ptr(bias), N.ptr(bias2), flags, N.ptr(ws), ws_bytes, precision, N.stream())
    disp = N.gemm_last_dispatch()
    # the plan of this very call - alignment and presence read off the pointers handed over - is what the library recorded
    given = dict(A=Av, B=Bv, C=Cbuf, bias=bias, bias2=None if bits is not None else bias2, bits_out=bits if c.get("bits") == "out" else None,
                 bits_in=bits if c.get("bits") == "in" else None, relu_mask=mask, colsum=colsum)
    call = N.gemm_call(ta, tb, M, Nn, K, lda, ldb, ldc, flags, present=[n for n, t in given.items() if t is not None and n not in ("A", "B", "C")],
                       misaligned=[n for n, t in given.items() if t is not None and t.data_ptr() % 16], drop=drop_p > 0,
                       ws_bytes=None if ws is None or bits is not None else ws_bytes)
    assert N.gemm_plan(call, precision) == (rc, disp), (N.gemm_plan(call, precision), rc, disp)
    torch.cuda.synchronize()
    # sentinels, unconditional: nothing outside M x N, the M column sums, the mask words
    assert bool((Cbuf[M:] == SENT).all()) and bool((Cbuf[:, Nn:] == SENT).all()), "C written outside M x N"
    if colsum is not None:
        assert bool((colsum[M:] == SENT).all()), "column sums written beyond M"
    if bits is not None:
        assert bool((bits[(M + 31) // 32 * Nn:] == BITS_SENT).all()), "mask words written beyond ceil(M / 32) N"
        if c["bits"] == "in":
            assert torch.equal(bits[:(M + 31) // 32 * Nn], epi["bits_in"]), "input mask words changed"
    if ws is not None:
        assert bool((ws[(ws_bytes + 3) // 4:] == SENT).all()), "workspace written beyond its size"
    return dict(rc=rc, C=Cbuf[:M, :Nn], Cbuf=Cbuf, colsum=colsum, bits=bits, dispatch=disp)


def epilogue_inputs(c, exact, g):
    M, Nn = c["M"], c["N"]
    draw = (lambda shape: _ints(g, shape)) if exact else (lambda shape: torch.randn(shape, generator=g, device="cuda"))
    e = dict(bias=draw((Nn,)), bias2=draw((Nn,)), C0=draw((M, Nn)))
    mk = draw((M, Nn))
    mk[0, :min(Nn, 2)] = torch.tensor([0.0, -0.0], device="cuda")[:min(Nn, 2)]           # mask > 0 is false for both zeros
    e["mask"] = mk
    e["bits_in"] = torch.randint(-2 ** 31, 2 ** 31, ((M + 31) // 32 * Nn,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    return e


def reference(N, c, AB, epi):
    """the epilogue of gemm_epilogue (csrc/gemm_common.h) in float64: bias, accumulate, ReLU, mask * mask_scale, dropout"""
    M, Nn = c["M"], c["N"]
    v = AB.clone()
    if c.get("bias"):
        v += epi["bias"].double()
    if c.get("bias2"):
        v += epi["bias2"].double()
    if c.get("acc"):
        v += epi["C0"].double()
    if c.get("relu"):
        v = v.clamp_min(0.0)
    if c.get("mask"):
        v = torch.where(epi["mask"] > 0, v * 1.25, torch.zeros_like(v))
    if c.get("bits") == "in":
        v = torch.where(unpack_bits(epi["bits_in"], M, Nn), v * 1.25, torch.zeros_like(v))
    if c.get("drop"):
        mk = torch.empty(M, Nn, device="cuda")
        N.call("rlt_dropout_mask", 4242, M, Nn, 0.5, N.ptr(mk), N.stream())
        keep = float((mk > 0).float().mean())
        assert bool(((mk == 0) | (mk == 2.0)).all()) and 0.4 < keep < 0.6
        v = v * mk.double()
    return v


def expect_dispatch(name, c, got):
    want = c["want"]
    seen = {k: got[k] for k in want}
    assert seen == want, f"{name}: expected {want}, got {got}"


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_gemm_branch(N, name, kind):
    c = CASES[name]
    M, Nn, K, mode = c["M"], c["N"], c["K"], c["mode"]
    exact = kind != "full"
    pool = "bf16x3" if mode == "bf16x3" else "bf16x6"
    sets = operands(pool if kind.startswith("wide") else "any", M, Nn, K, kind, bool(c.get("colsum")) and kind == "wideA")
    epi = epilogue_inputs(c, exact, _gen(name, kind))
    for which, (A, B, AB, scale) in enumerate(sets):
        ref = reference(N, c, AB, epi)
        out = launch(N, c, A, B, epi, MODES[mode])
        assert out["rc"] == 0, out["rc"]
        expect_dispatch(name, c, out["dispatch"])
        C = out["C"]
        cs_ref = A.double().sum(1)
        if exact:
            assert float(ref.abs().max()) < G.EXACT_LIMIT
            bad = C != ref.float()
            assert not bool(bad.any()), (f"{name} {kind}: {int(bad.sum())} of {M * Nn} elements differ from the exact reference, first at "
                                         f"{bad.nonzero()[0].tolist()}: got {C[bad][0].item()!r}, reference {ref[bad][0].item()!r}")
            if c.get("colsum"):
                assert float(cs_ref.abs().max()) < G.EXACT_LIMIT
                assert torch.equal(out["colsum"][:M], cs_ref.float()), f"{name} {kind}: fused column sums of A differ from the exact reference"
        else:
            tol = (2e-6 * math.sqrt(K) + 1e-6) * (6.0 if mode == "bf16x3" else 1.0)          # tools/gpu_probe.py: gemm section, mfma_tol
            err = float((C.double() - ref).abs().max())
            print(f"{name} full[{which}]: max|err| / max|ref| = {err / float(ref.abs().max()):.3e} (tol {tol:.3e})")
            assert err <= tol * float(ref.abs().max()), (name, which, err / float(ref.abs().max()), tol)
            if c.get("colsum"):
                cerr = float((out["colsum"][:M].double() - cs_ref).abs().max() / cs_ref.abs().max())
                assert cerr <= 1e-5, (name, "colsum", cerr)                                   # tools/gpu_probe.py: "gemm_ex colsum"
            if mode == "bf16x6":
                # tools/gpu_probe.py x6_adversarial: against the exact-fp32 mode on the same operands, errors in units of the terms
                o32 = launch(N, c, A, B, epi, MODES["fp32"])
                assert o32["rc"] == 0 and o32["dispatch"]["family"] == "gemm"
                e32 = float((o32["C"].double() - ref).abs().max()) / scale
                e6 = err / scale
                print(f"{name} full[{which}]: err bf16x6 {e6:.3e}, fp32 {e32:.3e}, ratio {e6 / max(e32, 1e-300):.2f}")
                assert e6 <= 1.25 * e32 + min(math.sqrt(K) * 2.0 ** -25, 2.0 * e32) + 2.0 ** -27, (name, which, e6, e32)
        if c.get("bits") == "out":
            got = unpack_bits(out["bits"], M, Nn)
            assert torch.equal(got, C > 0), f"{name} {kind}: mask bits differ from (C > 0)"
            if exact:
                assert torch.equal(got, ref > 0)


SPLIT_SHAPES = [("fp32", "nt", 128, 128, 2048), ("bf16x3", "tn", 256, 256, 2048), ("bf16x6", "nn", 256, 256, 2048)]


@pytest.mark.parametrize("mode,lay,M,Nn,K", SPLIT_SHAPES, ids=[f"{s[0]}-{s[1]}" for s in SPLIT_SHAPES])
def test_workspace_too_small_is_refused_before_any_launch(N, mode, lay, M, Nn, K):
    ta, tb = LAYOUTS[lay]
    c = dict(mode=mode, ta=ta, tb=tb, M=M, N=Nn, K=K, bias=True, colsum=bool(ta))
    A, B, _, _ = operands("any", M, Nn, K, "int", False)[0]
    out = launch(N, c, A, B, epilogue_inputs(c, True, _gen("small")), MODES[mode], ws_mode="small")
    assert out["rc"] == E_WORKSPACE
    assert out["dispatch"]["family"] == "none"
    assert bool((out["Cbuf"] == SENT).all()) and bool((out["colsum"] == SENT).all() if ta else True)


# ---------------------------------------------------------------------------------------------------------------- side kernels
def _guarded(n, pad=64):
    return torch.full((n + pad,), SENT, device="cuda")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("Nn", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("T", [511, 512, 513, 1025])
def test_colsum(N, T, Nn, acc):
    g = _gen("colsum", T, Nn)
    ldx = Nn + 3
    X = torch.full((T, ldx), float("nan"), device="cuda")
    X[:, :Nn] = _ints(g, (T, Nn))
    out0 = _ints(g, (Nn,))
    out = _guarded(Nn)
    out[:Nn] = out0
    nb = N.query("rlt_colsum_workspace", T, Nn)
    ws = _guarded(nb // 4)
    N.call("rlt_colsum", N.ptr(X), ldx, T, Nn, N.ptr(out), acc, N.ptr(ws), nb, N.stream())
    torch.cuda.synchronize()
    ref = X[:, :Nn].long().sum(0) + (out0.long() if acc else 0)
    assert torch.equal(out[:Nn].long(), ref) and bool((out[Nn:] == SENT).all()) and bool((ws[nb // 4:] == SENT).all())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("Gn", [1, 5])
@pytest.mark.parametrize("Nn", [63, 64, 65, 129])
@pytest.mark.parametrize("R", [1, 3, 4, 5, 300])
def test_segment_colsum(N, R, Nn, Gn, acc):
    g = _gen("segment", R, Nn, Gn)
    ldx, ldo = Nn + 1, Nn + 2
    X = torch.full((Gn * R, ldx), float("nan"), device="cuda")
    X[:, :Nn] = _ints(g, (Gn * R, Nn))
    out0 = _ints(g, (Gn, Nn))
    out = torch.full((Gn + 1, ldo), SENT, device="cuda")
    out[:Gn, :Nn] = out0
    N.call("rlt_segment_colsum", N.ptr(X), ldx, Gn, R, Nn, N.ptr(out), ldo, acc, N.stream())
    torch.cuda.synchronize()
    ref = X[:, :Nn].long().view(Gn, R, Nn).sum(1) + (out0.long() if acc else 0)
    assert torch.equal(out[:Gn, :Nn].long(), ref)
    assert bool((out[Gn:] == SENT).all()) and bool((out[:, Nn:] == SENT).all())


@pytest.mark.parametrize("with_db", [0, 1])
@pytest.mark.parametrize("M", [4, 1024, 1028])
@pytest.mark.parametrize("T", [1000, 5000, 4099])  # rows per workgroup = ceil(T / 2048): one; three with a last chunk of two rows / of one row
@pytest.mark.parametrize("I", [1, 2, 3])
def test_narrow_dw(N, I, T, M, with_db):
    g = _gen("narrow", I, T, M)
    lda, ldx = M + 4, I + 2
    A = torch.full((T, lda), float("nan"), device="cuda")
    A[:, :M] = _ints(g, (T, M))
    X = torch.full((T, ldx), float("nan"), device="cuda")
    X[:, :I] = _ints(g, (T, I))
    G.check_sum_bound(G.SMALL_MAX, G.SMALL_MAX, T)
    dW, db = _guarded(M * I), _guarded(M)
    nb = N.query("rlt_narrow_dw_workspace", T, M)
    ws = _guarded(nb // 4)
    N.call("rlt_narrow_dw", N.ptr(A), lda, N.ptr(X), ldx, I, T, M, N.ptr(dW), N.ptr(db) if with_db else None, N.ptr(ws), nb, N.stream())
    torch.cuda.synchronize()
    assert torch.equal(dW[:M * I].view(M, I).double(), A[:, :M].double().t() @ X[:, :I].double())           # (integers below 2^24: exact in both)
    assert bool((dW[M * I:] == SENT).all()) and bool((ws[nb // 4:] == SENT).all())
    if with_db:
        assert torch.equal(db[:M].long(), A[:, :M].long().sum(0)) and bool((db[M:] == SENT).all())
    else:
        assert bool((db == SENT).all())


EW_SIZES = [1, 1023, 1025, 4096 * 1024 + 1025]      # the last one: past one pass of the 4096 x 1024 grid


@pytest.mark.parametrize("n", EW_SIZES)
def test_relu_bwd(N, n):
    g = _gen("relu_bwd", n)
    Y = _ints(g, (n,), 2)
    Y[::7] = 0.0
    Y[3::11] = -0.0
    Y[5::13] = float("nan")
    dX0 = _ints(g, (n,)) + 0.5
    dX = _guarded(n)
    dX[:n] = dX0
    N.call("rlt_relu_bwd", N.ptr(dX), N.ptr(Y), n, N.stream())
    torch.cuda.synchronize()
    assert torch.equal(dX[:n], torch.where(Y > 0, dX0, torch.zeros_like(dX0))) and bool((dX[n:] == SENT).all())


@pytest.mark.parametrize("n", EW_SIZES)
def test_scale(N, n):
    g = _gen("scale", n)
    x0 = torch.randn(n, generator=g, device="cuda")
    x = _guarded(n)
    x[:n] = x0
    s = torch.tensor([0.125], device="cuda")           # a power of two: exact
    N.call("rlt_scale", N.ptr(x), N.ptr(s), n, N.stream())
    torch.cuda.synchronize()
    assert torch.equal(x[:n], x0 * 0.125) and bool((x[n:] == SENT).all())
