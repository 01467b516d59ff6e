"""The RLT_GEMM_ACCUMULATE epilogue of the bf16x6 tiles gemm6c and gemm6e (csrc/gemm_common.h: accumulate_blocks), through the raw C ABI
(rlt_gemm_ex), `pytest -m gpu`.  That epilogue reads C in batches ordered by hand - a block's 16 values together, the next block's
before this block's stores - so what is to be shown is that every element still gets fl(fl(acc + bias) + C_old), ReLU after, whatever
the tile walk, the layout of B, the leading dimension of C and whether C is the buffer an earlier GEMM wrote.

The reference is exact.  The same product is run WITHOUT RLT_GEMM_ACCUMULATE and without ReLU into D; the plain epilogue stores
D = fl(acc + bias) and is not touched by the batched read (it is the other branch of write_output_simple, the loop it was before), which is what makes it a valid reference: the expected output is relu?(fl(D + C_old)), one fp32 addition
done by torch, and the comparison is bitwise.  Both launches must report the same kernel family and persistent form (asserted from
rlt_gemm_plan and rlt_gemm_last_dispatch), so that `acc` is the same number in both and the test cannot quietly exercise another
kernel.

Shapes: N = 256; M = 256 is one 256 x 256 tile, not persistent; K = 64 is two K tiles (the pipeline minimum), on gemm6c, whose
element-wise accumulate epilogue is held to the same equation; K = 768 (the in_proj dX length, which the dispatch sends to gemm6e), 1024
and 2048 reach gemm6e (no workspace is handed over, so those are not split along K); M = 256 * 264 at K = 64 has more tiles than the
256 workgroups of the persistent form, which then walks tiles (gemm6c), and the same M at K = 1024 does it on gemm6e.  NN and NT, ldc = N and N + 4 (the padding columns are sentinels and must stay).
"""
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

RELU, ACC = 1, 2
BF16X6 = 2
SENT = -12345.0
NN_ = 256
COMBOS = {"acc": dict(bias=False, relu=False), "acc-bias": dict(bias=True, relu=False), "acc-bias-relu": dict(bias=True, relu=True)}
# (M, K) -> (family, persistent)
SHAPES = {(256, 64): ("gemm6c", 0), (256, 768): ("gemm6e", 0), (256, 1024): ("gemm6e", 0), (256, 2048): ("gemm6e", 0),
          (256 * 264, 64): ("gemm6c", 1), (256 * 264, 1024): ("gemm6e", 1)}


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rlt_hip import native
    native.load()
    return native


def _gen(*key):
    g = torch.Generator(device="cuda")
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


_OPERANDS = {}


def operands(M, K, tb):
    """A [M][K], B as stored ([N][K] for NT, [K][N] for NN), bias, C_old: drawn once per shape and layout, never written"""
    key = (M, K, tb)
    if key not in _OPERANDS:
        g = _gen(M, K, tb)
        rn = lambda *shape: torch.randn(shape, generator=g, device="cuda")
        _OPERANDS[key] = (rn(M, K), rn(NN_, K) if tb else rn(K, NN_), rn(NN_), rn(M, NN_))
    return _OPERANDS[key]


def gemm(N, tb, M, K, A, B, Cbuf, ldc, bias, flags, want):
    """one rlt_gemm_ex call without a workspace; the plan of the call and the record of the launch must both be `want`"""
    family, persistent = want
    call = N.gemm_call(0, tb, M, NN_, K, K, B.shape[1], ldc, flags, present=["bias"] if bias is not None else [])
    rc, plan = N.gemm_plan(call, BF16X6)
    assert rc == 0 and (plan["family"], plan["persistent"], plan["ns"]) == (family, persistent, 1), plan
    rc = N.load().rlt_gemm_ex(0, tb, M, NN_, K, N.ptr(A), K, N.ptr(B), B.shape[1], N.ptr(Cbuf), ldc, N.ptr(bias), None, flags,
                              None, 0, 1.0, None, 0.0, 0, None, 0, BF16X6, N.stream())
    assert rc == 0, rc
    assert N.gemm_last_dispatch() == plan, (N.gemm_last_dispatch(), plan)


def c_buffer(M, ldc, fill=None):
    buf = torch.full((M + 1, ldc), SENT, device="cuda")
    if fill is not None:
        buf[:M, :NN_] = fill
    return buf


def check_sentinels(buf, M):
    assert bool((buf[M:] == SENT).all()) and bool((buf[:, NN_:] == SENT).all()), "C written outside M x N"


def assert_bitwise(got, want, what):
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {got.numel()} elements differ, first at {bad.nonzero()[0].tolist()}: "
                                 f"got {got[bad][0].item()!r}, expected {want[bad][0].item()!r}")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("pad", [0, 4], ids=["ldcN", "ldcN+4"])
@pytest.mark.parametrize("lay", ["nn", "nt"])
@pytest.mark.parametrize("M,K", list(SHAPES), ids=[f"{m}x{k}" for m, k in SHAPES])
def test_accumulate_equals_plain_plus_c(N, M, K, lay, pad, combo):
    tb = int(lay == "nt")
    opt = COMBOS[combo]
    A, B, bias, C0 = operands(M, K, tb)
    bias = bias if opt["bias"] else None
    ldc = NN_ + pad
    D = c_buffer(M, ldc)
    gemm(N, tb, M, K, A, B, D, ldc, bias, 0, SHAPES[M, K])
    C = c_buffer(M, ldc, C0)
    gemm(N, tb, M, K, A, B, C, ldc, bias, ACC | (RELU if opt["relu"] else 0), SHAPES[M, K])
    torch.cuda.synchronize()
    check_sentinels(D, M)
    check_sentinels(C, M)
    want = D[:M, :NN_] + C0                      # fl(D + C_old) in fp32
    if opt["relu"]:
        want = torch.where(want > 0, want, torch.zeros_like(want))
    assert_bitwise(C[:M, :NN_], want, f"{SHAPES[M, K][0]} {M}x{NN_}x{K} {lay} ldc {ldc} {combo}")


@pytest.mark.parametrize("M,K", [(256, 64), (256, 768), (256, 1024)], ids=["gemm6c", "gemm6e-K768", "gemm6e"])
def test_accumulate_against_float64(N, M, K):
    """float64 product plus C_old; the bound of tests/test_gemm_dispatch_gpu.py for bf16x6 (`full` operands):
    max |C - ref| <= (2e-6 sqrt(K) + 1e-6) max |ref|"""
    A, B, _, C0 = operands(M, K, 0)
    C = c_buffer(M, NN_, C0)
    gemm(N, 0, M, K, A, B, C, NN_, None, ACC, SHAPES[M, K])
    torch.cuda.synchronize()
    ref = A.double() @ B.double() + C0.double()
    tol = 2e-6 * math.sqrt(K) + 1e-6
    err = float((C[:M].double() - ref).abs().max()) / float(ref.abs().max())
    print(f"{SHAPES[M, K][0]} K = {K}: max|err| / max|ref| = {err:.3e} (tol {tol:.3e})")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("M,K", [(256, 64), (256 * 264, 64), (256, 768), (256, 2048), (256 * 264, 1024)],
                         ids=["gemm6c", "gemm6c-persistent", "gemm6e-K768", "gemm6e", "gemm6e-persistent"])
def test_accumulate_in_place_on_a_gemm_output(N, M, K):
    """the training step's pattern (dz2): C is the buffer a previous plain GEMM wrote, the second product accumulates into it"""
    A1, B1, bias, _ = operands(M, K, 1)
    A2, B2, _, _ = operands(M, K, 0)
    ldc = NN_ + 4
    C = c_buffer(M, ldc)
    gemm(N, 1, M, K, A1, B1, C, ldc, bias, 0, SHAPES[M, K])
    first = C[:M, :NN_].clone()
    D = c_buffer(M, ldc)
    gemm(N, 0, M, K, A2, B2, D, ldc, None, 0, SHAPES[M, K])
    gemm(N, 0, M, K, A2, B2, C, ldc, None, ACC, SHAPES[M, K])
    torch.cuda.synchronize()
    check_sentinels(C, M)
    assert_bitwise(C[:M, :NN_], D[:M, :NN_] + first, f"in place, {SHAPES[M, K][0]} {M}x{NN_}x{K}")
