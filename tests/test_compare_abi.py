"""The paired comparison's C ABI without a GPU (include/rlt_hip.h: rlt_paired_compare, its workspace query and its plan): symbols
exported and bound, the workspace query and the plan answer without a device, and bad arguments are answered with the documented
codes before any launch - host buffers stand in for device memory, nothing is launched."""
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
    for name in ("rlt_paired_compare", "rlt_paired_compare_workspace", "rlt_paired_compare_plan"):
        assert name in native.EXPORTS and hasattr(lib, name)
    assert lib.rlt_abi_version() == 5
    assert native.CMP_WORDS == 16 and native.CMP_RESERVED == native.CMP_WORDS - 1
    assert ctypes.sizeof(native.PairedComparePlan) == 4 * len(native.CMP_PLAN_FIELDS)
    import re, os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rlt_hip.h")).read()
    words = dict(re.findall(r"#define RLT_CMP_([A-Z0-9_]+) (\d+)", header))
    for name, value in words.items():
        assert getattr(native, "CMP_" + name) == int(value), name
    assert len(words) == 17


def test_workspace_query_needs_no_gpu_and_grows(native):
    q = lambda Q, M, R: native.query("rlt_paired_compare_workspace", Q, M, R)
    assert q(1, 1, 0) > 0
    assert q(1, 1, 0) < q(300, 1, 0) < q(300, 3, 0) < q(300, 3, 100) < q(20000, 3, 100) < q(1 << 20, 3, 100) < q(1 << 20, 3, 10000)
    assert q(1 << 20, 4, 10000) >= 8 * 4 * (1 << 20) + 16 * 32 * 4 * 10001          # d, and the partials of 32 chunks
    for Q, M, R in ((0, 1, 1), (1, 0, 1), (1, 1, -1), ((1 << 26) + 1, 1, 1), (1, 9, 1), (1, 1, (1 << 20) + 1), (-5, 1, 1)):
        assert q(Q, M, R) == 0, (Q, M, R)
    assert q(1 << 26, 8, 0) > 8 * 8 * (1 << 26)          # a size_t: beyond 2^32 bytes


def test_plan(native):
    p = native.paired_compare_plan(300, 4, 1000)
    assert p["form"] == "resident" and p["chunks"] == 1 and p["lds_bytes"] == 300 * 4 * 8 and p["replicates_per_wave"] >= 1
    for M in range(1, 9):
        p = native.paired_compare_plan(300, M, 10)
        qmax, C = p["resident_max_q"], p["chunk"]
        assert qmax * M * 8 <= 160 * 1024 < (qmax + 1) * M * 8
        assert C % 64 == 0 and C > qmax + 1
        assert native.paired_compare_plan(qmax, M, 10)["form"] == "resident"
        assert native.paired_compare_plan(qmax, M, 10)["lds_bytes"] == qmax * M * 8
        over = native.paired_compare_plan(qmax + 1, M, 10)
        assert over["form"] == "chunked" and over["chunks"] == 1 and over["lds_bytes"] == 0
        assert native.paired_compare_plan(2 * C + 5, M, 10)["chunks"] == 3 and native.paired_compare_plan(C, M, 10)["chunks"] == 1
    # many replicates of a small problem: several per wavefront, and still at least 1024 workgroups
    p = native.paired_compare_plan(250, 4, 1 << 20)
    assert p["replicates_per_wave"] == 16
    lib = native.load()
    out = native.PairedComparePlan()
    assert lib.rlt_paired_compare_plan(300, 1, 10, None) == ARG
    for Q, M, R, code in ((0, 1, 1, ARG), (1, 0, 1, ARG), (1, 1, -1, ARG), ((1 << 26) + 1, 1, 1, SHAPE), (1, 9, 1, SHAPE),
                          (1, 1, (1 << 20) + 1, SHAPE)):
        assert lib.rlt_paired_compare_plan(Q, M, R, ctypes.byref(out)) == code, (Q, M, R)


def test_argument_errors(native):
    lib = native.load()
    Q, M, R, ld = 40, 2, 8, 48
    keep_b, base = _buf(4 * Q)
    keep_s, sys = _buf(4 * M * ld)
    ws_bytes = native.query("rlt_paired_compare_workspace", Q, M, R)
    keep_w, ws = _buf(ws_bytes)
    keep_r, rec = _buf(8 * native.CMP_WORDS * M)
    keep_a, rs = _buf(8 * M * R)
    keep_c, bs = _buf(8 * M * R)
    P = ctypes.c_void_p
    o = lambda v: P(v) if v else None
    call = lambda b=base, s=sys, ld_=ld, Q_=Q, M_=M, R_=R, w=ws, wb=ws_bytes, r=rec, a=rs, c=bs: lib.rlt_paired_compare(
        o(b), o(s), ld_, Q_, M_, R_, 7, o(w), wb, o(r), o(a), o(c), None)
    assert call(b=0) == ARG and call(s=0) == ARG and call(w=0) == ARG and call(r=0) == ARG
    assert call(Q_=0) == ARG and call(M_=0) == ARG and call(R_=-1) == ARG and call(Q_=-3) == ARG
    assert call(ld_=Q - 1) == ARG
    big = native.query("rlt_paired_compare_workspace", 1 << 26, 8, 1 << 20)
    assert call(Q_=(1 << 26) + 1, ld_=(1 << 26) + 1, wb=big) == SHAPE and call(M_=9, wb=big) == SHAPE
    assert call(R_=(1 << 20) + 1, wb=big) == SHAPE
    assert call(b=base + 2) == ALIGN and call(s=sys + 1) == ALIGN and call(r=rec + 4) == ALIGN
    assert call(a=rs + 4) == ALIGN and call(c=bs + 4) == ALIGN
    assert call(wb=ws_bytes - 1) == WORKSPACE and call(wb=0) == WORKSPACE and call(w=ws + 8) == WORKSPACE
    assert call(Q_=Q + 8, wb=ws_bytes) == WORKSPACE          # a workspace sized for a smaller problem
