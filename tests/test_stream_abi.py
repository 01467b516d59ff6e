"""rlt_seq_attention_append (csrc/attention_seq_append.hip) and rlt_hazard_head_append (csrc/hazard.hip) at the C ABI without a
device: the names are declared, bound and in EXPORTS (that the header's exports are exactly native.EXPORTS: tests/test_abi.py), and
the error classes come back in the order the header states - RLT_E_ARG, RLT_E_SHAPE, RLT_E_ALIGN.  Host buffers only: nothing here reaches a launch."""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rlt_seq_attention_append", "rlt_hazard_head_append")
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4


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


def test_names_are_bound_and_the_header_sections_state_the_contract(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    lib = native.load()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.rlt_abi_version() == 5                     # the additions are additive
    att = header[header.index("streaming: K/V-cached append attention"):header.index("BiLSTM recurrence (M2)")]
    for words in ("PREFIX STATEMENT", "UNTOUCHED", "RLT_E_ARG", "RLT_E_SHAPE", "RLT_E_ALIGN", "Algorithmic bytes", "(Smax*B, 2E)"):
        assert words in att, words
    hz = header[header.index("streaming: the hazard head"):header.index("probe heads (the probing study)")]
    for words in ("PREFIX STATEMENT", "UNTOUCHED", "RLT_E_ARG", "RLT_E_SHAPE", "RLT_E_ALIGN", "Algorithmic bytes", "carry (B)"):
        assert words in hz, words


def test_attention_append_errors_in_the_stated_order(native, mem):
    lib = native.load()
    _, x, off = mem

    def app(chunk=x, cache=x, t0=0, C=4, Smax=8, B=2, H=2, HD=16, active=x, out=x, lse=x, prec=native.PRECISION_DEFAULT):
        return lib.rlt_seq_attention_append(chunk, cache, t0, C, Smax, B, H, HD, active, out, lse, prec, None)

    # RLT_E_ARG first, whatever else is wrong
    for name in ("chunk", "cache", "out"):
        assert app(**{name: None}) == E_ARG, name
        assert app(**{name: None}, HD=32) == E_ARG and app(**{name: None}, Smax=2000) == E_ARG
        others = [n for n in ("chunk", "cache", "out", "lse") if n != name]
        assert all(app(**{name: None, o: off}) == E_ARG for o in others)
    for name in ("C", "Smax", "B", "H"):
        for bad in (0, -3):
            assert app(**{name: bad}) == E_ARG and app(**{name: bad}, HD=32) == E_ARG and app(**{name: bad}, chunk=off) == E_ARG, (name, bad)
    assert app(t0=-1) == E_ARG and app(t0=-1, HD=7) == E_ARG
    assert app(t0=5, C=4, Smax=8) == E_ARG and app(t0=8, C=1, Smax=8) == E_ARG and app(t0=0, C=9, Smax=8) == E_ARG
    assert app(t0=2 ** 31 - 1, C=2 ** 31 - 1, Smax=8) == E_ARG                          # the sum does not wrap
    assert app(t0=5, C=4, Smax=8, HD=32) == E_ARG and app(t0=5, C=4, Smax=8, out=off) == E_ARG
    assert app(prec=77) == E_ARG and app(prec=77, HD=32) == E_ARG
    # then RLT_E_SHAPE: the limits of rlt_seq_attention_fwd_ex with Smax for S
    for kw in ({"HD": 32}, {"HD": 0}, {"HD": 8}, {"HD": 128}, {"Smax": 1025}, {"B": 1 << 24, "H": 4, "HD": 64}):
        assert app(**kw) == E_SHAPE and app(**kw, chunk=off) == E_SHAPE and app(**kw, cache=off) == E_SHAPE, kw
    # then RLT_E_ALIGN; lse and active are optional, probed through the error that follows them
    for name in ("chunk", "cache", "out", "lse"):
        assert app(**{name: off}) == E_ALIGN, name
    assert app(lse=None, active=None, out=off) == E_ALIGN
    assert app(t0=4, C=4, Smax=8, out=off) == E_ALIGN and app(t0=7, C=1, Smax=8, out=off) == E_ALIGN     # the last admissible chunks


def test_hazard_append_errors_in_the_stated_order(native, mem):
    lib = native.load()
    _, x, off = mem

    def app(xp=x, w=x, b=x, offset=x, t0=0, C=8, B=2, E=64, final=0, carry=x, tau=0.5, active=x, k=x, stop=x, p=x, z=x):
        return lib.rlt_hazard_head_append(xp, w, b, offset, t0, C, B, E, final, carry, tau, active, k, stop, p, z, None)

    for name in ("xp", "w", "b", "carry", "stop"):
        assert app(**{name: None}) == E_ARG, name
        assert app(**{name: None}, C=1025) == E_ARG and app(**{name: None}, E=96) == E_ARG
        if name != "xp":
            assert app(**{name: None}, xp=off) == E_ARG
    assert app(k=None) == E_ARG and app(k=None, E=96) == E_ARG                          # a decision needs somewhere to write k
    for name in ("C", "B", "E"):
        for bad in (0, -3):
            assert app(**{name: bad}) == E_ARG and app(**{name: bad}, xp=off) == E_ARG, (name, bad)
    assert app(t0=-1) == E_ARG and app(t0=-1, E=96) == E_ARG and app(t0=2 ** 31 - 1, C=8) == E_ARG
    for kw in ({"C": 1025}, {"E": 32}, {"E": 96}, {"E": 1088}, {"E": 2048}):
        assert app(**kw) == E_SHAPE and app(**kw, xp=off) == E_SHAPE and app(**kw, w=off) == E_SHAPE, kw
    assert app(xp=off) == E_ALIGN and app(w=off) == E_ALIGN
    # the optional pointers are optional
    assert app(offset=None, active=None, k=None, p=None, z=None, xp=off) == E_ALIGN
    assert app(t0=300, C=1024, xp=off) == E_ALIGN                                       # t0 is not bounded by the chunk limit
