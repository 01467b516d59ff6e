"""rlt_seq_attention_* (within-list attention, csrc/attention_seq.hip) at the C ABI without a device: the three names are declared
and bound, every argument error comes back before any launch in the order include/rlt_hip.h states (RLT_E_ARG, RLT_E_SHAPE,
RLT_E_ALIGN, RLT_E_WORKSPACE), and the workspace query is 0 for a bad precision code or head dim.  Host buffers only: nothing here
reaches a launch."""
import ctypes

import pytest

NAMES = ("rlt_seq_attention_bwd_workspace", "rlt_seq_attention_fwd", "rlt_seq_attention_bwd")
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


@pytest.fixture(scope="module")
def mem():
    buf = (ctypes.c_uint8 * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 4)


def test_names_are_declared_and_bound(native):
    lib = native.load()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.rlt_abi_version() == 5


def test_workspace_query(native):
    q = lambda *a: native.query("rlt_seq_attention_bwd_workspace", *a)
    for prec in (native.PRECISION_DEFAULT, native.PRECISION_FP32, native.PRECISION_BF16X3, native.PRECISION_BF16X6):
        assert q(300, 4096, 4, 64, 0.0, prec) == 0 and q(300, 8192, 8, 16, 0.2, prec) == 0      # no sum crosses a workgroup
    assert q(300, 4096, 4, 64, 0.0, 3) == 0 and q(300, 4096, 4, 64, 0.0, -2) == 0                # a bad precision code
    assert q(300, 4096, 4, 32, 0.0, native.PRECISION_DEFAULT) == 0                               # a bad head dim


def test_errors_in_the_stated_order(native, mem):
    lib = native.load()
    _, x, off = mem
    D = native.PRECISION_DEFAULT

    def fwd(qkv=x, S=8, B=2, H=2, HD=16, p=0.0, out=x, lse=x, prec=D):
        return lib.rlt_seq_attention_fwd(qkv, S, B, H, HD, p, 1, out, lse, prec, None)

    def bwd(qkv=x, out=x, dout=x, lse=x, S=8, B=2, H=2, HD=16, p=0.0, dqkv=x, ws=None, ws_bytes=0, prec=D):
        return lib.rlt_seq_attention_bwd(qkv, out, dout, lse, S, B, H, HD, p, 1, dqkv, ws, ws_bytes, prec, None)

    # RLT_E_ARG: precision first, then NULL pointers, non-positive sizes, drop_p outside [0, 1) - each ahead of every later class
    for bad in (3, -2, 7):
        assert fwd(prec=bad) == E_ARG and bwd(prec=bad) == E_ARG
        assert fwd(prec=bad, qkv=None, HD=32, out=off) == E_ARG
    for name in ("qkv", "out", "lse"):
        assert fwd(**{name: None}) == E_ARG and fwd(**{name: None}, HD=32, S=2000) == E_ARG
    for name in ("qkv", "out", "dout", "lse", "dqkv"):
        assert bwd(**{name: None}) == E_ARG and bwd(**{name: None}, HD=32, S=2000) == E_ARG
    for fn in (fwd, bwd):
        for name in ("S", "B", "H"):
            assert fn(**{name: 0}) == E_ARG and fn(**{name: -3}) == E_ARG
            assert fn(**{name: 0}, HD=48) == E_ARG                                               # ahead of RLT_E_SHAPE
        for p in (-0.1, 1.0, 1.5, float("nan")):
            assert fn(p=p) == E_ARG and fn(p=p, HD=32, qkv=off) == E_ARG
        # RLT_E_SHAPE: head dim, S > 1024, the index limits - ahead of RLT_E_ALIGN
        for hd in (8, 32, 128, 0, -16):
            assert fn(HD=hd) == E_SHAPE and fn(HD=hd, qkv=off) == E_SHAPE
        assert fn(S=1025) == E_SHAPE and fn(S=1025, qkv=off) == E_SHAPE
        assert fn(S=1024, B=2 ** 31 - 1, H=1, HD=16) == E_SHAPE                                  # S*B*3E past 2^40 elements
        assert fn(S=1024, B=2 ** 20, H=2 ** 20, HD=64) == E_SHAPE
        assert fn(S=1, B=2 ** 31 - 1, H=2 ** 31 - 1, HD=64) == E_SHAPE                           # nothing wraps on the way
        assert fn(S=1, B=2 ** 24, H=1, HD=16) == E_SHAPE                                         # 2^24 workgroups
        assert fn(S=1, B=2 ** 22, H=16, HD=16, qkv=off) == E_SHAPE
        # RLT_E_ALIGN
        assert fn(qkv=off) == E_ALIGN and fn(lse=off) == E_ALIGN and fn(out=off) == E_ALIGN
    assert bwd(dout=off) == E_ALIGN and bwd(dqkv=off) == E_ALIGN and bwd(ws=off, ws_bytes=64) == E_ALIGN
    # RLT_E_WORKSPACE: ws_bytes below the query's answer - 0 bytes today, so no call can be short of it and ws may be NULL
    assert native.query("rlt_seq_attention_bwd_workspace", 8, 2, 2, 16, 0.0, D) == 0
