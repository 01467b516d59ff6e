"""rlt_hazard_head_fwd / _bwd_workspace / _bwd (csrc/hazard.hip) at the C ABI without a device: the names are declared, bound and
in EXPORTS; the error classes come back in the order the header states - RLT_E_ARG, RLT_E_SHAPE, RLT_E_ALIGN, RLT_E_WORKSPACE -
and the workspace query is 0 for arguments out of range.  Host buffers only: nothing here reaches a launch."""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rlt_hazard_head_fwd", "rlt_hazard_head_bwd_workspace", "rlt_hazard_head_bwd")
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
    assert lib.rlt_abi_version() == 5
    for words in ("PREFIX GUARANTEE", "RLT_E_ARG", "RLT_E_SHAPE", "RLT_E_ALIGN", "RLT_E_WORKSPACE", "Algorithmic bytes"):
        assert words in header[header.index("hazard cut head"):header.index("probe heads (the probing study)")], words


def test_errors_in_the_stated_order(native, mem):
    lib = native.load()
    _, x, off = mem
    big = 1 << 30

    def fwd(xp=x, w=x, b=x, offset=x, S=8, B=2, E=64, p=x, stop=x, z=x):
        return lib.rlt_hazard_head_fwd(xp, w, b, offset, S, B, E, p, stop, z, None)

    def bwd(xp=x, w=x, z=x, dp=x, dstop=x, S=8, B=2, E=64, dx=x, acc=0, dw=x, db=x, ws=x, ws_bytes=big):
        return lib.rlt_hazard_head_bwd(xp, w, z, dp, dstop, S, B, E, dx, acc, dw, db, ws, ws_bytes, None)

    shape_bad = ({"S": 1025}, {"E": 32}, {"E": 96}, {"E": 1088}, {"E": 2048})
    for fn, required in ((fwd, ("xp", "w", "b", "p", "z")), (bwd, ("xp", "w", "z", "dp", "dx", "dw", "db", "ws"))):
        # RLT_E_ARG first: a required pointer NULL or a size not positive, whatever else is wrong
        for name in required:
            assert fn(**{name: None}) == E_ARG, name
            assert fn(**{name: None}, S=1025) == E_ARG and fn(**{name: None}, E=96) == E_ARG
            if name != "xp":
                assert fn(**{name: None}, xp=off) == E_ARG
        for name in ("S", "B", "E"):
            for bad in (0, -3):
                assert fn(**{name: bad}) == E_ARG and fn(**{name: bad}, xp=off) == E_ARG and fn(**{name: bad}, w=off) == E_ARG
        assert fn(S=0, E=96) == E_ARG and fn(B=-1, S=2000) == E_ARG
        # then RLT_E_SHAPE, ahead of alignment (and of the workspace)
        for kw in shape_bad:
            assert fn(**kw) == E_SHAPE and fn(**kw, xp=off) == E_SHAPE and fn(**kw, w=off) == E_SHAPE, kw
        # then RLT_E_ALIGN
        assert fn(xp=off) == E_ALIGN and fn(w=off) == E_ALIGN
    # the optional pointers are optional: with host pointers a call that passes every check would launch, so they are probed
    # through the error that follows them
    assert fwd(offset=None, stop=None, xp=off) == E_ALIGN and bwd(dstop=None, xp=off) == E_ALIGN
    assert bwd(dx=off) == E_ALIGN
    # RLT_E_WORKSPACE last
    need = native.query("rlt_hazard_head_bwd_workspace", 8, 2, 64)
    assert need == 2 * (64 + 4) * 4
    assert bwd(ws_bytes=need - 1) == E_WORKSPACE and bwd(ws_bytes=0) == E_WORKSPACE
    assert bwd(ws_bytes=0, dx=off) == E_ALIGN and bwd(ws_bytes=0, S=1025) == E_SHAPE and bwd(ws_bytes=0, dp=None) == E_ARG
    for kw in shape_bad:
        assert bwd(**kw, ws_bytes=0) == E_SHAPE


def test_workspace_query_is_zero_out_of_range(native):
    q = lambda S, B, E: native.query("rlt_hazard_head_bwd_workspace", S, B, E)
    assert q(300, 4096, 256) == 4096 * 260 * 4 and q(1, 1, 64) == 68 * 4 and q(1024, 3, 1024) == 3 * 1028 * 4
    for S, B, E in ((0, 2, 64), (-1, 2, 64), (8, 0, 64), (8, -2, 64), (8, 2, 0), (8, 2, -64), (1025, 2, 64), (8, 2, 32),
                    (8, 2, 96), (8, 2, 1088), (8, 2, 2048)):
        assert q(S, B, E) == 0, (S, B, E)
