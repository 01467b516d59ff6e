"""Every BiLSTM recurrence kernel the default switches can select (csrc/lstm.hip, csrc/lstm6w.hip), through the raw C ABI
(rlt_bilstm_rec_fwd / _fwd_x / _bwd) against the float64 restatement of tests/lstm_restate.py.  `pytest -m gpu`.

One test id per (kernel, shape); the id names the kernel and native.bilstm_rec_plan is asserted before the launch:

    f32-*          bilstm_fwd_kernel<XIN> / bilstm_bwd_kernel                 fp32 mode, 32 lists per workgroup
    x3-*           bilstm3_fwd_kernel<XIN> / bilstm3_bwd8_kernel              bf16x3 mode, 32 lists per workgroup
    x6w_single-*   bilstm6w_fwd_kernel<XIN, true> / bilstm6w_bwd_kernel<true>    bf16x6 mode up to 2048 lists, 16 per workgroup
    x6w_halves-*   bilstm6w_fwd_kernel<XIN, false> / bilstm6w_bwd_kernel<false>  bf16x6 mode from 2049 lists, two 16-list halves
with fwd = rlt_bilstm_rec_fwd (in place on `gates`), fwdx = rlt_bilstm_rec_fwd_x (fused input projection), bwd =
rlt_bilstm_rec_bwd: 12 kernels.  The bf16x6 two-phase forward (bilstm6_fwd_kernel) is reachable only from 2^20 lists or under an
environment switch: it stays with tests/test_lstm_plan.py and the x6_fallbacks section of tools/gpu_probe.py.  No environment
variable is read or set here.

Shapes, the smallest that reach each edge: 32-list kernels B in {1, 31, 32, 33, 64, 65}, S in {1, 9}; x6w single B in {1, 15, 16,
17, 33, 2048}; x6w two halves B in {2049, 2064, 2065, 2080} (one list in the last workgroup / its second half empty / one list in
the second half / every workgroup full); the x6w kernels are software pipelines, so S in {1, 2, 3, 9} at every B (prologue and
epilogue without a steady state).  I = 3 everywhere, I = 1 and 2 at one ragged B per kernel.

Operand classes, each seeded from its case name; weights and biases ~ U(+-128^-1/2) (nn.LSTM's initialisation) in all of them:
    default      pre-activations (fwd) or x (fwdx) and d_hout ~ randn
    sat30/sat100 pre-activations randn x 30 / x 100 (fwdx: x scaled so that x W_ih^T has that spread): sigmoid and tanh of the
                 x6w kernels are formed from exp2 and v_rcp_f32, which overflow / flush to zero there
    tagged       list b's pre-activations (x) and d_hout are a function of b alone, different for every list: lists swapped or
                 duplicated within a workgroup show

Every forward id compares the activated gates, c and h with float64 in the metric of tools/gpu_probe.py (max |err| / max |ref|
over the tensor) at its `lstm` section's bound, 2e-5 in all three modes.  Every backward id feeds the kernel the REFERENCE's stash
(float64 activated gates and c, rounded to float32) and compares dgates at that section's gradient bound, 1e-4; the *-chained ids
run the device's own forward in front, as production does.  Outputs start as NaN (an element not written fails its comparison);
256 NaN floats behind `gates`, `h_out`, `c_out` must still be NaN and the inputs bitwise unchanged.  *-twice ids: the same call
from the same inputs gives bitwise-equal outputs.  test_refused_calls_write_nothing: the argument checks of the three entry points.

Largest observed errors per kernel (MI355X), forward max(gates, c, h) / backward dgates, over all ids of the kernel; in
brackets the fwdx ids outside the saturated classes:
    f32         fwd 3.3e-07  fwdx 6.9e-06 (2.8e-07)  bwd 1.9e-07
    x3          fwd 3.6e-06  fwdx 1.1e-05 (1.6e-06)  bwd 1.6e-06
    x6w_single  fwd 3.6e-07  fwdx 4.0e-06 (1.1e-06)  bwd 1.8e-07
    x6w_halves  fwd 4.4e-07  fwdx 1.1e-05 (1.0e-06)  bwd 2.6e-07
The fwdx figures of sat100 are float32's own: with |x| ~ 2000 the three products of a pre-activation are ~500 each and cancel, so
x W_ih^T evaluated in plain float32 is already 8e-5 off in a pre-activation and 1.4e-5 off in tanh of it (torch on the CPU, operands of the same
distribution).  255 ids, 3 s."""
import math
import zlib

import pytest
import torch

import lstm_restate as R

pytestmark = pytest.mark.gpu

HID, GUARD = 128, 256
FWD_TOL, BWD_TOL = 2e-5, 1e-4
KERNELS = {"f32": ("fp32", 32), "x3": ("bf16x3", 32), "x6w_single": ("bf16x6", 16), "x6w_halves": ("bf16x6", 32)}
BATCHES = {"f32": (1, 31, 32, 33, 64, 65), "x3": (1, 31, 32, 33, 64, 65), "x6w_single": (1, 15, 16, 17, 33, 2048),
           "x6w_halves": (2049, 2064, 2065, 2080)}
STEPS = {"f32": (1, 9), "x3": (1, 9), "x6w_single": (1, 2, 3, 9), "x6w_halves": (1, 2, 3, 9)}
RAGGED = {"f32": 33, "x3": 33, "x6w_single": 17, "x6w_halves": 2065}      # one ragged B per kernel for the one-off cases


def _cases():
    """(kernel, part, B, S, I, class, extra): part fwd / fwdx / bwd; extra '' / 'chained' / 'twice'"""
    out = []
    for k in KERNELS:
        for part in ("fwd", "fwdx", "bwd"):
            out += [(k, part, B, S, 3, "default", "") for B in BATCHES[k] for S in STEPS[k]]
            out += [(k, part, RAGGED[k], 9, 3, cls, "") for cls in ("sat30", "sat100")]
            out += [(k, part, RAGGED[k], 3 if k.startswith("x6w") else 9, 3, "tagged", "")]
            out += [(k, part, RAGGED[k], 3, 3, "default", "twice")]
        out += [(k, "fwdx", RAGGED[k], 3, I, "default", "") for I in (1, 2)]
        out += [(k, "bwd", RAGGED[k], 9, 3, "default", "chained")]
    # the float64 reference is shared by the kernels and parts that run one (shape, class): keep them next to each other
    return sorted(out, key=lambda c: (c[2], c[3], c[4], c[5]))


CASES = _cases()


def case_id(c):
    k, part, B, S, I, cls, extra = c
    return f"{k}-{part}-B{B}-S{S}" + (f"-I{I}" if part == "fwdx" else "") + ("" if cls == "default" else f"-{cls}") + (f"-{extra}" if extra else "")


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rlt_hip import native
    native.load()
    return native


def rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def guarded(n, dev):
    """n NaN floats to be written, GUARD NaN floats behind them -> (buffer, sentinel view)"""
    full = torch.full((n + GUARD,), float("nan"), device=dev)
    return full[:n], full[n:]


def bits(t):
    return t.contiguous().view(torch.int32)


def untouched(guards):
    return all(bool(torch.isnan(g).all()) for g in guards)


class Operands:
    """Inputs of one (B, S, I, class) in float32 on the device and the float64 results; computed once, read-only afterwards.
    pre: the pre-activations rlt_bilstm_rec_fwd starts from; x: the input rows of rlt_bilstm_rec_fwd_x (its pre-activations are
    x W_ih^T + b_ih + b_hh).  The backward ids use the stash of `pre`."""

    def __init__(self, B, S, I, cls):
        dev = torch.device("cuda")
        name = f"{cls}-B{B}-S{S}-I{I}"
        g = torch.Generator(device=dev).manual_seed(zlib.crc32(name.encode()))
        bound = HID ** -0.5
        uni = lambda *shape: (torch.rand(*shape, generator=g, device=dev) * 2 - 1) * bound
        self.w_hh = [uni(4 * HID, HID) for _ in (0, 1)]
        self.w_ih = [uni(4 * HID, I) for _ in (0, 1)]
        self.b_ih = [uni(4 * HID) for _ in (0, 1)]
        self.b_hh = [uni(4 * HID) for _ in (0, 1)]
        T = S * B
        if cls == "tagged":
            b = torch.arange(B, device=dev, dtype=torch.float64).repeat(S)[:, None]                     # row s * B + b -> b
            row = torch.arange(8 * HID, device=dev, dtype=torch.float64)[None, :]
            self.pre = (2.0 * torch.sin(0.37 * (b + 1) + 0.011 * row)).float().reshape(T, 2, 4 * HID)
            self.x = torch.sin(0.37 * (b + 1) + torch.arange(I, device=dev, dtype=torch.float64)[None, :]).float()
            self.d_hout = torch.cos(0.53 * (b + 1) + 0.07 * row[:, :2 * HID]).float()
            assert len({tuple(r) for r in self.x[:B].tolist()}) == B                                    # every list its own tag
        else:
            scale = {"default": 1.0, "sat30": 30.0, "sat100": 100.0}[cls]
            self.pre = torch.randn(T, 2, 4 * HID, generator=g, device=dev) * scale
            # x W_ih^T of x ~ randn has the spread sqrt(I / (3 * 128)) (W_ih ~ U(+-128^-1/2)): scale x to reach `scale`
            self.x = torch.randn(T, I, generator=g, device=dev) * (1.0 if cls == "default" else scale * math.sqrt(3 * HID / I))
            self.d_hout = torch.randn(T, 2 * HID, generator=g, device=dev)
        self.B, self.S, self.I = B, S, I
        self.ref = R.forward(self.pre, self.w_hh, S, B)
        self.pre_x = R.preactivations(self.x, self.w_ih, self.b_ih, self.b_hh)
        if cls in ("sat30", "sat100"):
            assert float(self.pre_x.std()) > 0.8 * scale
        self.ref_x = R.forward(self.pre_x, self.w_hh, S, B)
        self.dgates = R.backward(self.ref[0], self.ref[1], self.w_hh, self.d_hout, S, B)
        self.inputs = [self.pre, self.x, self.d_hout] + self.w_hh + self.w_ih + self.b_ih + self.b_hh
        self.saved = [bits(t).clone() for t in self.inputs]

    def unchanged(self):
        return all(torch.equal(bits(t), s) for t, s in zip(self.inputs, self.saved))


_CACHE = {}


def operands(B, S, I, cls):
    key = (B, S, I, cls)
    if key not in _CACHE:
        _CACHE.clear()                       # (the ids are sorted by this key: one set of operands at a time)
        _CACHE[key] = Operands(B, S, I, cls)
    return _CACHE[key]


def run_forward(N, op, part, code):
    """-> (gates, c, h) views and their sentinels"""
    dev, T, p = op.pre.device, op.S * op.B, N.ptr
    gates, g_end = guarded(T * 8 * HID, dev)
    h, h_end = guarded(T * 2 * HID, dev)
    c, c_end = guarded(T * 2 * HID, dev)
    if part == "fwd":
        gates.copy_(op.pre.reshape(-1))
        N.call("rlt_bilstm_rec_fwd", p(gates), p(op.w_hh[0]), p(op.w_hh[1]), op.S, op.B, p(h), p(c), code, N.stream())
    else:
        N.call("rlt_bilstm_rec_fwd_x", p(op.x), op.I, p(op.w_ih[0]), p(op.b_ih[0]), p(op.b_hh[0]), p(op.w_ih[1]), p(op.b_ih[1]),
               p(op.b_hh[1]), p(op.w_hh[0]), p(op.w_hh[1]), op.S, op.B, p(gates), p(h), p(c), code, N.stream())
    torch.cuda.synchronize()
    return (gates.reshape(T, 2, 4 * HID), c.reshape(T, 2, HID), h.reshape(T, 2 * HID)), (g_end, h_end, c_end)


def run_backward(N, op, act, c, code):
    """act, c: the stash the kernel is fed (float32) -> dgates view, its sentinel, the kernel's own copy of c"""
    dev, T, p = op.pre.device, op.S * op.B, N.ptr
    gates, g_end = guarded(T * 8 * HID, dev)
    gates.copy_(act.reshape(-1))
    c_in = c.float().contiguous().clone()
    N.call("rlt_bilstm_rec_bwd", p(gates), p(c_in), p(op.w_hh[0]), p(op.w_hh[1]), p(op.d_hout), op.S, op.B, code, N.stream())
    torch.cuda.synchronize()
    return gates.reshape(T, 2, 4 * HID), g_end, c_in


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_kernel(N, case):
    kernel, part, B, S, I, cls, extra = case
    prec, lists = KERNELS[kernel]
    code = N.precision_code(prec)
    plan = N.bilstm_rec_plan(B, int(part == "fwdx"), code)
    which = "bwd" if part == "bwd" else "fwd"
    assert (plan[which], plan[which + "_lists"]) == (kernel, lists), plan
    op = operands(B, S, I, cls)

    if part != "bwd":
        (gates, c, h), ends = run_forward(N, op, part, code)
        ref = op.ref if part == "fwd" else op.ref_x
        errs = {"gates": rel(gates, ref[0]), "c": rel(c, ref[1]), "h": rel(h, ref[2]), "dgates": 0.0}
        print(case_id(case), errs)
        assert max(errs["gates"], errs["c"], errs["h"]) <= FWD_TOL, errs
        assert untouched(ends), "written behind gates, h_out or c_out"
        if extra == "twice":
            (gates2, c2, h2), _ = run_forward(N, op, part, code)
            assert torch.equal(bits(gates), bits(gates2)) and torch.equal(bits(c), bits(c2)) and torch.equal(bits(h), bits(h2))
    else:
        if extra == "chained":
            assert plan["fwd"] == kernel
            (act, c, _), _ = run_forward(N, op, "fwd", code)
        else:
            act, c = op.ref[0].float(), op.ref[1].float()
        dg, g_end, c_in = run_backward(N, op, act, c, code)
        errs = {"gates": 0.0, "c": 0.0, "h": 0.0, "dgates": rel(dg, op.dgates)}
        print(case_id(case), errs)
        assert errs["dgates"] <= BWD_TOL, errs
        assert untouched([g_end]), "written behind gates"
        assert torch.equal(bits(c_in), bits(c.float().contiguous())), "the backward wrote to c"
        if extra == "twice":
            dg2, _, _ = run_backward(N, op, act, c, code)
            assert torch.equal(bits(dg), bits(dg2))
    assert op.unchanged(), "an input was written to"


E_SHAPE, E_ALIGN, PATTERN = -2, -4, 12345.0


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_refused_calls_write_nothing(N, prec):
    """a `gates` pointer off by 4 bytes is RLT_E_ALIGN in all three entry points, I = 0 and I = 4 are RLT_E_SHAPE in _fwd_x; no
    refused call touches an output"""
    import ctypes
    B, S, I = 5, 2, 3
    op, code, lib, p, st = operands(B, S, I, "default"), N.precision_code(prec), N.load(), N.ptr, N.stream()
    T = S * B
    dev = op.pre.device
    gates = torch.full((T * 8 * HID + 4,), PATTERN, device=dev)
    h = torch.full((T * 2 * HID,), PATTERN, device=dev)
    c = torch.full((T * 2 * HID,), PATTERN, device=dev)
    off = ctypes.c_void_p(gates.data_ptr() + 4)
    w = (p(op.w_hh[0]), p(op.w_hh[1]))
    xw = (p(op.w_ih[0]), p(op.b_ih[0]), p(op.b_hh[0]), p(op.w_ih[1]), p(op.b_ih[1]), p(op.b_hh[1]))
    assert lib.rlt_bilstm_rec_fwd(off, *w, S, B, p(h), p(c), code, st) == E_ALIGN
    assert lib.rlt_bilstm_rec_fwd_x(p(op.x), I, *xw, *w, S, B, off, p(h), p(c), code, st) == E_ALIGN
    assert lib.rlt_bilstm_rec_bwd(off, p(c), *w, p(op.d_hout), S, B, code, st) == E_ALIGN
    for bad_i in (0, 4):
        assert lib.rlt_bilstm_rec_fwd_x(p(op.x), bad_i, *xw, *w, S, B, p(gates), p(h), p(c), code, st) == E_SHAPE
    torch.cuda.synchronize()
    for t in (gates, h, c):
        assert bool((t == PATTERN).all()), "a refused call wrote to an output"
    assert op.unchanged()
