"""rlt_seq_attention_fwd_ex / _bwd_ex (within-list attention with a mask code, csrc/attention_seq.hip) at the C ABI without a device:
both names are declared and bound, the mask code is checked with the other argument errors - after the precision code and the
pointers, ahead of RLT_E_SHAPE, RLT_E_ALIGN and RLT_E_WORKSPACE - and every other error comes back in the order of the calls
without _ex.  Host buffers only: nothing here reaches a launch."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rlt_seq_attention_fwd_ex", "rlt_seq_attention_bwd_ex")
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
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    lib = native.load()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+RLT_SEQ_MASK_NONE\s+0\b", header) and re.search(r"#define\s+RLT_SEQ_MASK_CAUSAL\s+1\b", header)
    assert (native.SEQ_MASK_NONE, native.SEQ_MASK_CAUSAL) == (0, 1)
    assert lib.rlt_abi_version() == 5


def test_errors_in_the_stated_order(native, mem):
    lib = native.load()
    _, x, off = mem
    D = native.PRECISION_DEFAULT

    def fwd(qkv=x, S=8, B=2, H=2, HD=16, p=0.0, mask=1, out=x, lse=x, prec=D):
        return lib.rlt_seq_attention_fwd_ex(qkv, S, B, H, HD, p, 1, mask, out, lse, prec, None)

    def bwd(qkv=x, out=x, dout=x, lse=x, S=8, B=2, H=2, HD=16, p=0.0, mask=1, dqkv=x, ws=None, ws_bytes=0, prec=D):
        return lib.rlt_seq_attention_bwd_ex(qkv, out, dout, lse, S, B, H, HD, p, 1, mask, dqkv, ws, ws_bytes, prec, None)

    for fn in (fwd, bwd):
        # the mask code: RLT_E_ARG, ahead of every later class - with host pointers, so nothing can have been launched
        for bad in (2, -1, 7, 2 ** 31 - 1):
            assert fn(mask=bad) == E_ARG
            assert fn(mask=bad, HD=32) == E_ARG and fn(mask=bad, S=1025) == E_ARG                # ahead of RLT_E_SHAPE
            assert fn(mask=bad, qkv=off) == E_ARG and fn(mask=bad, lse=off) == E_ARG             # ahead of RLT_E_ALIGN
            assert fn(mask=bad, HD=48, qkv=off) == E_ARG
        for mask in (0, 1):
            # the other argument errors are those of the calls without _ex, under both masks
            for bad in (3, -2, 7):
                assert fn(prec=bad, mask=mask) == E_ARG and fn(prec=bad, mask=5, HD=32, qkv=off) == E_ARG
            assert fn(qkv=None, mask=mask) == E_ARG and fn(lse=None, mask=mask, HD=32, S=2000) == E_ARG
            for name in ("S", "B", "H"):
                assert fn(**{name: 0}, mask=mask) == E_ARG and fn(**{name: -3}, mask=mask, HD=48) == E_ARG
            for p in (-0.1, 1.0, float("nan")):
                assert fn(p=p, mask=mask) == E_ARG and fn(p=p, mask=mask, HD=32, qkv=off) == E_ARG
            for hd in (8, 32, 128, 0):
                assert fn(HD=hd, mask=mask) == E_SHAPE and fn(HD=hd, mask=mask, qkv=off) == E_SHAPE
            assert fn(S=1025, mask=mask) == E_SHAPE and fn(S=1, B=2 ** 24, H=1, HD=16, mask=mask) == E_SHAPE
            assert fn(qkv=off, mask=mask) == E_ALIGN and fn(lse=off, mask=mask) == E_ALIGN and fn(out=off, mask=mask) == E_ALIGN
    assert bwd(mask=9, dout=off) == E_ARG and bwd(mask=9, ws=off, ws_bytes=64) == E_ARG
    assert bwd(dout=off) == E_ALIGN and bwd(dqkv=off) == E_ALIGN and bwd(ws=off, ws_bytes=64) == E_ALIGN
    assert bwd(dqkv=None, mask=9) == E_ARG and fwd(out=None, mask=9) == E_ARG
    # the workspace query takes no mask: 0 bytes under both, so RLT_E_WORKSPACE cannot be reached and ws may be NULL
    assert native.query("rlt_seq_attention_bwd_workspace", 8, 2, 2, 16, 0.0, D) == 0
