"""The C ABI of the reward losses for any cut reward without a GPU (include/rlt_hip.h: rlt_reward_spec, rlt_reward_spec_matrix,
rlt_reward_any_workspace, rlt_reward_any_loss): symbols and constants declared, bound and exported, the workspace query answers
without a device, and every bad argument is answered with its documented code before any launch - host buffers stand in for
device memory, nothing is launched."""
import ctypes
import os
import re

import pytest

ARG, SHAPE, WORKSPACE, ALIGN = -1, -2, -3, -4
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rlt_reward_spec_matrix", "rlt_reward_any_workspace", "rlt_reward_any_loss")


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def _buf(nbytes):
    raw = (ctypes.c_uint8 * (nbytes + 64))()
    return raw, (ctypes.addressof(raw) + 63) // 64 * 64


def test_symbols_and_constants(native):
    lib = native.load()
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.rlt_abi_version() == 5
    defines = dict(re.findall(r"#define RLT_REWARD_([A-Z_]+)\s+(\d+)", header))
    assert defines == {"FBETA": "0", "GAIN": "1", "MAX_GRADES": "8"}
    assert (native.REWARD_FBETA, native.REWARD_GAIN, native.REWARD_MAX_GRADES) == (0, 1, 8)
    # the struct of the header: int family, n_grades, normalize; float beta; float gain[8]; const float* discount
    S = native.RewardSpecStruct
    assert [f[0] for f in S._fields_] == ["family", "n_grades", "normalize", "beta", "gain", "discount"]
    assert ctypes.sizeof(S) == 56 and S.gain.offset == 16 and S.discount.offset == 48
    assert re.search(r"typedef struct \{[^}]*int\s+family;[^}]*int\s+n_grades;[^}]*int\s+normalize;[^}]*float\s+beta;[^}]*"
                     r"float\s+gain\[RLT_REWARD_MAX_GRADES\];[^}]*const float\*\s+discount;[^}]*\} rlt_reward_spec;", header)


def test_workspace_query(native):
    q = lambda B: native.query("rlt_reward_any_workspace", B)
    assert q(0) == 0 and q(-3) == 0
    last = 0
    for B in list(range(1, 70)) + [255, 256, 257, 4096, 8191, 8192, 8193, 100000, 1 << 20, (1 << 31) - 1]:
        assert q(B) >= last and q(B) >= 32, B
        last = q(B)


class Call:
    """A valid call of rlt_reward_any_loss on host buffers; each test breaks one argument."""

    def __init__(self, native, B=6, S=40):
        self.native, self.lib = native, native.load()
        self.B, self.S = B, S
        self.keep = []
        n = 4 * B * S

        def buf(nbytes):
            raw, base = _buf(nbytes)
            self.keep.append(raw)
            return base
        self.p, self.y, self.r, self.dp = buf(n), buf(n), buf(n), buf(n)
        self.per, self.loss, self.k, self.rk, self.rb, self.bk = (buf(4 * B) for _ in range(6))
        self.sums, self.table = buf(32), buf(native.query("rlt_dcg_table_bytes"))
        self.ws_bytes = native.query("rlt_reward_any_workspace", B)
        self.ws = buf(self.ws_bytes)
        self.fbeta = native.reward_spec_struct(native.REWARD_FBETA, beta=2.0)
        self.gain = native.reward_spec_struct(native.REWARD_GAIN, gains=(-1.0, 1.0, 3.0), normalize=True)

    def loss_call(self, **kw):
        a = dict(p=self.p, labels=self.y, spec=self.fbeta, r_in=None, B=self.B, S=self.S, kind=self.native.LOSS_JS, tau=0.85,
                 per=self.per, loss=self.loss, dp=self.dp, k=self.k, rk=self.rk, rb=self.rb, bk=self.bk, sums=self.sums,
                 table=self.table, ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        spec = None if a["spec"] is None else ctypes.byref(a["spec"])
        return self.lib.rlt_reward_any_loss(a["p"], a["labels"], spec, a["r_in"], a["B"], a["S"], a["kind"], a["tau"], a["per"],
                                            a["loss"], a["dp"], a["k"], a["rk"], a["rb"], a["bk"], a["sums"], a["table"], a["ws"],
                                            a["ws_bytes"], None)

    def matrix_call(self, **kw):
        a = dict(labels=self.y, B=self.B, S=self.S, spec=self.gain, tau=1.0, table=self.table, r=self.r, q=self.dp)
        a.update(kw)
        spec = None if a["spec"] is None else ctypes.byref(a["spec"])
        return self.lib.rlt_reward_spec_matrix(a["labels"], a["B"], a["S"], spec, a["tau"], a["table"], a["r"], a["q"], None)


@pytest.fixture()
def call(native):
    return Call(native)


def test_short_workspace_is_the_last_check(call):
    """Everything valid but the workspace: RLT_E_WORKSPACE, i.e. every other check passed - and nothing was launched."""
    assert call.loss_call(ws_bytes=call.ws_bytes - 1) == WORKSPACE
    assert call.loss_call(ws_bytes=0) == WORKSPACE
    assert call.loss_call(spec=call.gain, ws_bytes=0) == WORKSPACE
    assert call.loss_call(labels=None, spec=None, r_in=call.r, ws_bytes=0) == WORKSPACE
    assert call.loss_call(dp=None, per=None, k=None, rk=None, rb=None, bk=None, sums=None, loss=None, ws_bytes=0) == WORKSPACE


def test_reward_source(call):
    assert call.loss_call(r_in=call.r) == ARG                               # both
    assert call.loss_call(labels=None, spec=None) == ARG                    # neither
    assert call.loss_call(spec=None) == ARG                                 # labels without a spec
    assert call.loss_call(labels=None) == ARG                               # a spec without labels
    assert call.loss_call(labels=None, r_in=call.r) == ARG                  # a matrix and a spec
    assert call.loss_call(spec=None, r_in=call.r) == ARG                    # a matrix and labels


def test_null_and_dimension_arguments(call):
    assert call.loss_call(p=None) == ARG
    assert call.loss_call(ws=None) == ARG
    for B, S in ((0, 40), (-1, 40), (6, 0), (6, -4)):
        assert call.loss_call(B=B, S=S) == ARG
        assert call.matrix_call(B=B, S=S) == ARG
    assert call.matrix_call(labels=None) == ARG
    assert call.matrix_call(spec=None) == ARG
    assert call.matrix_call(r=None, q=None) == ARG
    assert call.matrix_call(table=None) == ARG                              # GAIN without discounts needs the table
    assert call.loss_call(spec=call.gain, table=None) == ARG
    assert call.loss_call(table=None, ws_bytes=0) == WORKSPACE              # FBETA does not read it


def test_spec_ranges(call):
    N = call.native
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        bad = N.reward_spec_struct(N.REWARD_FBETA, beta=beta)
        assert call.loss_call(spec=bad) == ARG, beta
        assert call.matrix_call(spec=bad) == ARG, beta
    for n in (0, 1, 9, -2):
        bad = N.reward_spec_struct(N.REWARD_GAIN, gains=(0.0, 1.0))
        bad.n_grades = n
        assert call.loss_call(spec=bad) == ARG, n
        assert call.matrix_call(spec=bad) == ARG, n
    for n in (2, 8):
        ok = N.reward_spec_struct(N.REWARD_GAIN, gains=(0.5,) * n)
        assert call.loss_call(spec=ok, ws_bytes=0) == WORKSPACE, n
    for family in (-1, 2, 7):
        bad = N.reward_spec_struct(N.REWARD_FBETA, beta=1.0)
        bad.family = family
        assert call.loss_call(spec=bad) == ARG, family
        assert call.matrix_call(spec=bad) == ARG, family
    bad = N.reward_spec_struct(N.REWARD_GAIN, gains=(0.0, float("nan"), 1.0))
    assert call.loss_call(spec=bad) == ARG


def test_kind_and_tau(call):
    for kind in (-1, 4, 100):
        assert call.loss_call(kind=kind) == ARG
    for kind in range(4):
        assert call.loss_call(kind=kind, ws_bytes=0) == WORKSPACE
    for tau in (0.0, -0.5, float("nan")):
        assert call.loss_call(tau=tau) == ARG
        assert call.matrix_call(tau=tau) == ARG


def test_shape(call):
    assert call.loss_call(S=1025) == SHAPE
    assert call.loss_call(S=1028) == SHAPE
    assert call.matrix_call(S=1025) == SHAPE
    assert call.loss_call(S=1024, ws_bytes=0) in (WORKSPACE,)               # 1024 itself is inside (the buffers are not touched)


def test_misaligned_rows(call):
    """S % 4 == 0: rows are read and written 16 bytes at a time."""
    for name in ("p", "labels", "dp"):
        assert call.loss_call(**{name: getattr(call, {"labels": "y"}.get(name, name)) + 4}) == ALIGN, name
        assert call.loss_call(**{name: getattr(call, {"labels": "y"}.get(name, name)) + 8}) == ALIGN, name
    assert call.loss_call(labels=None, spec=None, r_in=call.r + 4) == ALIGN
    assert call.matrix_call(labels=call.y + 4) == ALIGN
    assert call.matrix_call(r=call.r + 4) == ALIGN
    assert call.matrix_call(q=call.dp + 8) == ALIGN
    # S % 4 != 0: 4-byte alignment suffices, 2 does not
    assert call.loss_call(S=39, p=call.p + 4, labels=call.y + 4, dp=call.dp + 12, ws_bytes=0) == WORKSPACE
    assert call.loss_call(S=39, p=call.p + 2) == ALIGN
    assert call.loss_call(sums=call.sums + 4) == ALIGN
    assert call.loss_call(ws=call.ws + 4) == ALIGN
