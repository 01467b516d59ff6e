"""rlt_stream_compact_plan and rlt_kv_cache_compact (csrc/stream_compact.hip) at the C ABI without a device: the names are declared,
bound and in EXPORTS, the header section states its contract, and the error classes come back in the order the header states -
RLT_E_ARG, RLT_E_SHAPE, RLT_E_ALIGN - with the no-launch returns behind them.  Host buffers only: nothing here reaches a launch."""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rlt_stream_compact_plan", "rlt_kv_cache_compact")
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


@pytest.fixture(scope="module")
def mem():
    """eleven distinct 16-byte aligned host addresses 64 bytes apart, and for each the address 4 and 2 bytes further"""
    buf = (ctypes.c_uint8 * 40960)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    at = [base + 64 * i for i in range(11)]
    return buf, at


def V(a):
    return None if a is None else ctypes.c_void_p(a)


def test_names_are_bound_and_the_header_section_states_the_contract(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    lib = native.load()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.rlt_abi_version() == 5                     # the additions are additive
    assert header.index("streaming: the hazard head") < header.index("streaming: compacting the live lists") < header.index("probe heads (the probing study)")
    sec = header[header.index("streaming: compacting the live lists"):header.index("probe heads (the probing study)")]
    for words in ("stable partition", "ASCENDING", "UNTOUCHED", "bitwise", "not synchronised", "no atomics", "two\n *   calls give the same bits",
                  "must not overlap", "no in-place form", "neither read nor written", "RLT_E_ARG", "RLT_E_SHAPE", "RLT_E_ALIGN",
                  "Algorithmic bytes", "without a launch", "csrc/stream_compact.hip", "tests/test_stream_compact_gpu.py",
                  "tests/test_stream_compact_abi.py", "once per row"):
        assert words in sec, words
    assert native._SIGNATURES["rlt_stream_compact_plan"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6
    assert native._SIGNATURES["rlt_kv_cache_compact"][1] == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p]


def test_plan_errors_in_the_stated_order(native, mem):
    lib = native.load()
    _, at = mem
    names = ("active", "origin", "carry", "k", "slot_src", "origin_out", "carry_out", "k_full", "n_live")
    good = dict(zip(names, at))

    def plan(B=8, B_full=8, **kw):
        a = {**good, **kw}
        return lib.rlt_stream_compact_plan(V(a["active"]), V(a["origin"]), V(a["carry"]), V(a["k"]), B, B_full, V(a["slot_src"]),
                                           V(a["origin_out"]), V(a["carry_out"]), V(a["k_full"]), V(a["n_live"]), None)

    off4 = {n: good[n] + 4 for n in names}      # off 8 bytes, on 4
    off2 = {n: good[n] + 2 for n in names}      # off 4 bytes
    big = {"B_full": (1 << 30) + 1}
    # RLT_E_ARG first, whatever else is wrong: the required pointers
    for name in ("active", "slot_src", "origin_out", "n_live"):
        assert plan(**{name: None}) == E_ARG, name
        assert plan(**{name: None}, **big) == E_ARG and plan(**{name: None}, carry=off4["carry"]) == E_ARG
    # one half of a pair without the other
    for a, b in (("carry", "carry_out"), ("k", "k_full")):
        assert plan(**{a: None}) == E_ARG and plan(**{b: None}) == E_ARG, (a, b)
        assert plan(**{a: None}, **big) == E_ARG and plan(**{b: None}, active=off2["active"]) == E_ARG
    # the sizes
    for kw in ({"B": 0}, {"B": -3}, {"B_full": 0}, {"B": 4, "B_full": -1}, {"B": 9, "B_full": 8}, {"B": 2 ** 31 - 1, "B_full": 8}):
        assert plan(**kw) == E_ARG and plan(**kw, carry=off4["carry"]) == E_ARG, kw
    assert plan(B=(1 << 30) + 2, B_full=(1 << 30) + 1) == E_ARG                        # B > B_full ahead of the index limit
    # an output in the place of an input
    for out in ("slot_src", "origin_out", "k_full", "n_live"):
        for inp in ("active", "origin", "k"):
            assert plan(**{out: good[inp]}) == E_ARG and plan(**{out: good[inp]}, **big) == E_ARG, (out, inp)
    assert plan(carry_out=good["carry"]) == E_ARG and plan(carry_out=good["carry"], active=off2["active"]) == E_ARG
    assert plan(k_full=good["k"], origin=None) == E_ARG
    # then RLT_E_SHAPE: the index limit
    assert plan(**big) == E_SHAPE and plan(**big, carry=off4["carry"]) == E_SHAPE and plan(**big, active=off2["active"]) == E_SHAPE
    assert plan(B=1 << 30, B_full=1 << 30, active=off2["active"]) == E_ALIGN          # the limit itself is admitted
    # then RLT_E_ALIGN: the float64 arrays off 8 bytes, the int arrays off 4
    for name in ("carry", "carry_out"):
        assert plan(**{name: off4[name]}) == E_ALIGN and plan(**{name: off2[name]}) == E_ALIGN, name
    for name in ("active", "origin", "k", "slot_src", "origin_out", "k_full", "n_live"):
        assert plan(**{name: off2[name]}) == E_ALIGN, name
    # the optional pointers are optional: probed through the error that follows them
    assert plan(origin=None, carry=None, carry_out=None, k=None, k_full=None, active=off2["active"]) == E_ALIGN
    assert plan(origin=None, k=None, k_full=None, carry=off4["carry"]) == E_ALIGN
    assert plan(B=1, B_full=1, n_live=off2["n_live"]) == E_ALIGN and plan(B=3, B_full=8, n_live=off2["n_live"]) == E_ALIGN


def test_cache_compact_errors_in_the_stated_order_and_the_no_launch_returns(native, mem):
    lib = native.load()
    _, at = mem
    src, dst, smap = at[0], at[0] + 16384, at[10]                # `mem` is 40 KiB: two ranges of up to 16 KiB

    def cc(s=src, d=dst, m=smap, t0=2, B_src=4, B_dst=2, W=8):
        return lib.rlt_kv_cache_compact(V(s), V(d), V(m), t0, B_src, B_dst, W, None)

    # RLT_E_ARG first
    for kw in ({"s": None}, {"d": None}, {"m": None}):
        assert cc(**kw) == E_ARG and cc(**kw, W=6) == E_ARG and cc(**kw, W=4096, t0=0) == E_ARG, kw
    assert cc(s=None, d=dst + 4) == E_ARG and cc(d=None, s=src + 4) == E_ARG
    for kw in ({"t0": -1}, {"B_src": 0}, {"B_src": -2}, {"B_dst": -1}, {"B_dst": 5}, {"B_src": 1, "B_dst": 2}, {"W": 0}, {"W": -4}):
        assert cc(**kw) == E_ARG and cc(**kw, s=src + 4) == E_ARG, kw
        if "W" not in kw:
            assert cc(**kw, W=6) == E_ARG and cc(**{"t0": 0, **kw}, W=4096) == E_ARG, kw
    # overlap of [src, src + t0*B_src*W) and [dst, dst + t0*B_dst*W): t0 = 2, B_src = 4, B_dst = 2, W = 8 -> 256 and 128 bytes
    assert cc(d=src) == E_ARG                                    # in place
    assert cc(d=src + 128) == E_ARG and cc(d=src + 240) == E_ARG and cc(d=src + 252) == E_ARG      # dst starts inside src
    assert cc(s=dst + 64) == E_ARG and cc(s=dst + 112) == E_ARG                                    # src starts inside dst
    assert cc(d=src + 128, W=6) == E_ARG and cc(d=src + 16, t0=2 ** 31 - 1, B_src=2 ** 31 - 1, B_dst=2 ** 31 - 1, W=2 ** 31 - 1) == E_ARG
    # then RLT_E_SHAPE
    for kw in ({"W": 6}, {"W": 2}, {"W": 2052, "t0": 1, "B_src": 1, "B_dst": 0}, {"W": 4096, "t0": 0}, {"t0": 2 ** 31 - 1, "B_src": 2 ** 31 - 1, "B_dst": 0, "W": 4},
               {"t0": 1 << 20, "B_src": 1 << 20, "B_dst": 0, "W": 4}, {"t0": 0, "B_src": (1 << 30) + 1, "W": 4}):
        assert cc(**kw) == E_SHAPE and cc(**kw, s=src + 4) == E_SHAPE and cc(**kw, d=dst + 8) == E_SHAPE, kw
    # then RLT_E_ALIGN; ranges that only touch are no overlap
    assert cc(s=src + 4) == E_ALIGN and cc(d=dst + 8) == E_ALIGN and cc(s=src + 4, t0=0) == E_ALIGN and cc(d=dst + 4, B_dst=0) == E_ALIGN
    assert cc(s=src + 4, d=src + 4 + 256) == E_ALIGN and cc(s=dst + 128 + 8, d=dst) == E_ALIGN
    assert cc(W=2048, t0=1, B_src=1, B_dst=1, s=src + 4) == E_ALIGN                     # the widest row is admitted
    # the no-launch returns: 0 with host pointers, nothing was read or written
    assert cc(t0=0) == 0 and cc(B_dst=0) == 0 and cc(t0=0, B_dst=0) == 0
    assert cc(t0=0, d=src) == 0 and cc(B_dst=0, d=src) == 0                             # empty ranges do not overlap
