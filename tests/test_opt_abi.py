"""The guarded optimizer step's C ABI without a GPU (include/rlt_hip.h: rlt_grad_norm, rlt_adam_step_guarded): symbols exported
and bound, the workspace query answers and grows with n, and bad arguments are answered with the documented codes before any
launch - host buffers stand in for device memory, nothing is launched."""
import ctypes

import pytest

ARG, SHAPE, WORKSPACE, ALIGN = -1, -2, -3, -4


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def _buf(nbytes):
    raw = (ctypes.c_uint8 * (nbytes + 64))()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    return raw, base


def test_symbols_exported_bound_and_the_constants(native):
    lib = native.load()
    for name in ("rlt_grad_norm_chunk", "rlt_grad_norm_grid", "rlt_grad_norm_workspace", "rlt_grad_norm", "rlt_adam_step_guarded"):
        assert name in native.EXPORTS and hasattr(lib, name)
    C, G = native.query("rlt_grad_norm_chunk"), lib.rlt_grad_norm_grid()
    assert C >= 1024 and C % 1024 == 0 and G >= 1        # a chunk is whole 16-byte groups of a 256-lane workgroup
    assert lib.rlt_abi_version() == 5
    assert native.OPT_STATE_WORDS * 8 == 104 and native.OPT_COEF_F32 == 2 * 11


def test_workspace_query_needs_no_gpu_and_grows_with_n(native):
    q = lambda n, s: native.query("rlt_grad_norm_workspace", n, s)
    C = native.query("rlt_grad_norm_chunk")
    assert q(4, 0) > 0
    assert q(4, 0) <= q(C, 0) < q(2 * C + 8, 0) < q(64 * C, 0) < q(237_600_000, 0)
    assert q(1_846_785 // 4 * 4, 60) > q(1_846_785 // 4 * 4, 0)        # per-segment records
    assert q(237_600_000, 0) >= 237_600_000 // C * 24                   # a record per chunk: sum of squares, count, maximum
    assert q(0, 0) == 0 and q(6, 0) == 0 and q(8, -1) == 0


def test_grad_norm_argument_errors(native):
    lib = native.load()
    n = 64
    keep_g, g = _buf(4 * n)
    keep_s, state = _buf(104)
    ws_bytes = native.query("rlt_grad_norm_workspace", n, 3)
    keep_w, ws = _buf(ws_bytes)
    keep_o, seg_out = _buf(24 * 3)
    offs = (ctypes.c_int64 * 4)(0, 8, 40, n)
    P = ctypes.c_void_p
    call = lambda g_=g, n_=n, off=offs, ns=3, mx=1.0, ws_=ws, wb=ws_bytes, so=seg_out, st=state: lib.rlt_grad_norm(
        P(g_) if g_ else None, n_, off, ns, mx, P(ws_) if ws_ else None, wb, P(so) if so else None, P(st) if st else None, None)
    # null pointers, n == 0, inconsistent segment arguments, a NaN bound
    assert call(g_=0) == ARG and call(ws_=0) == ARG and call(st=0) == ARG and call(n_=0) == ARG
    assert call(off=None) == ARG and call(so=0) == ARG and call(ns=-1) == ARG and call(ns=0) == ARG      # ns=0 with a table given
    assert call(mx=float("nan")) == ARG
    assert call(n_=n - 2, off=None, ns=0, so=0) == SHAPE
    assert call(g_=g + 4) == ALIGN and call(st=state + 4) == ALIGN
    # a short or misaligned workspace
    assert call(wb=ws_bytes - 1) == WORKSPACE and call(wb=0) == WORKSPACE and call(ws_=ws + 8) == WORKSPACE
    # a segment table the host can read is checked: descending, not starting at 0, not ending at n, off the 4-element grid
    for bad in ((0, 40, 8, n), (4, 8, 40, n), (0, 8, 40, n - 4), (0, 6, 40, n), (0, 8, 40, n + 4)):
        assert call(off=(ctypes.c_int64 * 4)(*bad)) == ARG, bad


def test_guarded_step_argument_errors(native):
    lib = native.load()
    n = 64
    keep, base = _buf(4 * 4 * n + 128)
    p, g, m, v, state = (base + i * 4 * n for i in range(5))
    P = ctypes.c_void_p
    call = lambda p_=p, g_=g, m_=m, v_=v, n_=n, st=state: lib.rlt_adam_step_guarded(
        P(p_) if p_ else None, P(g_) if g_ else None, P(m_) if m_ else None, P(v_) if v_ else None, n_, P(st) if st else None,
        1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None)
    assert call(p_=0) == ARG and call(g_=0) == ARG and call(m_=0) == ARG and call(v_=0) == ARG and call(st=0) == ARG
    assert call(n_=0) == ARG and call(n_=n - 1) == SHAPE
    assert call(p_=p + 4) == ALIGN and call(v_=v + 8) == ALIGN and call(st=state + 4) == ALIGN
