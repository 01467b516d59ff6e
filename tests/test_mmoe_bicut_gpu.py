"""The kernels MMOECut / MOECut / PLECut, BiCut and Choopy's input rest on (csrc/mmoe.hip, csrc/bicut.hip, the layout helpers and
rlt_choopy_embed of csrc/heads.hip) at their edges against float64, through the raw C ABI (rlt_hip.native).  `pytest -m gpu`.
The branch a case reaches is named in its test id:

    gate-dw-C*-B*-S*    rlt_mmoe_gate_bwd: gate_dw_kernel's blockIdx.y column blocks and `c < C` tail (C > 256, C % 256), its b0
                        loop and `nb` tail (B > 64, B % 64); gate_dh_kernel / gate_fwd_kernel with idle wavefronts (S < 4) and
                        idle lanes (C % 64); n_tasks 1..3, n_e 1..8, accumulate_dh 0 / 1
    mix-fwd-E* / mix-bwd-E*   one float4 = one token (E = 4), the `c < E` tail of mix_bwd_kernel (E % 256), two rounds (E = 512)
    pair-*              the two-class head, pair-gridstride: 1,053,443 tokens, the first size past one sweep of the 4096 x 256 grid
    bicut-last0-*       BiCutLoss with the last class-0 position placed at a lane boundary
    pm-* / choopy-*     the layout maps and the Choopy embedding, pm-gridcap: past the 4096-workgroup grid cap

The reference is tests/mmoe_bicut_restate.py (float64 numpy, pinned by tests/test_mmoe_bicut_restate.py).  Bounds:

  * the linear MMOE kernels (gate_dh, gate_dw, mix_fwd, mix_bwd) get small integers and dyadic rationals, so that every fp32
    partial sum is exact in any order (asserted on the restatement: every sum of absolute terms below 2^20 grid units): the
    device result equals the float64 one element by element.
  * the softmax-bearing paths with random operands: the bounds tools/gpu_probe.py's embed_mmoe section holds them to - gates 2e-5,
    gradients 1e-4, max |err| / max |ref| per output tensor; a gate row sums to 1 within 1e-6.
  * pair softmax: forward 1e-6, backward 1e-5 in the same form (the bicut section's bounds).
  * BiCutLoss: dout |err| <= 1e-6 |ref| element by element (at most three fp32 roundings of a float64-exact value, 1.8e-7) and
    exactly 0 past the mask; per_list within 1e-5 of the sum of its absolute terms; loss within 1e-5 max(1, |ref|).
  * the layout maps and the embedding are copies: bit for bit through an int32 view, -0.0 and NaN payloads planted.

Every output is allocated with sentinel padding behind it and pre-filled with the sentinel: a store beyond the array and an
element never written both show."""
import numpy as np
import pytest
import torch

import mmoe_bicut_restate as R
from test_scan_dispatch_gpu import N, SENTINEL, Tally, dev, padded, rel, unpad      # noqa: F401  (N: the module's fixture)

pytestmark = pytest.mark.gpu

E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4          # RLT_E_* of include/rlt_hip.h
F64 = np.float64


def dyadic(g, shape, bound, den):
    """multiples of 1 / den in [-bound, bound], float32 (exact)"""
    return (g.integers(-bound * den, bound * den + 1, size=shape) / den).astype(np.float32)


def exact(t, what, case, got, ref, abs_sum, unit):
    """ref and every partial sum on the grid `unit` and below 2^20 of it (then exact in fp32 in any order); got == ref"""
    assert float(np.max(abs_sum)) / unit < 2 ** 20, (what, case)
    assert np.array_equal(ref / unit, np.rint(ref / unit)), (what, case)
    t.add(what, case, float((got.astype(F64) != ref).sum()), 0)


# ---------------------------------------------------------------------------------------------- MMOE gates
def gate_fwd(N, h, w, S, B):
    nt, ne, C = len(w), w[0].shape[1], h.shape[1]
    hd, wd = dev(h), [dev(x) for x in w]
    gates = padded(nt * B * ne, torch.float32)
    N.call("rlt_mmoe_gate_fwd", N.ptr(hd), N.pointer_array(wd), nt, ne, S, B, C, N.ptr(gates), N.stream())
    torch.cuda.synchronize()
    return unpad(gates, nt * B * ne, "gates").reshape(nt, B, ne)


def gate_bwd(N, h, w, gates, dgates, S, B, dh0):
    """dh0: None (accumulate_dh = 0, dh holds the sentinel) or the values dh is pre-filled with (accumulate_dh = 1)"""
    nt, ne, C = len(w), w[0].shape[1], h.shape[1]
    hd, wd, gd, dgd = dev(h), [dev(x) for x in w], dev(gates), dev(dgates)
    dh = padded(S * B * C, torch.float32)
    if dh0 is not None:
        dh[:S * B * C] = dev(dh0).reshape(-1)
    dw = [padded(S * C * ne, torch.float32) for _ in range(nt)]
    ws_bytes = N.query("rlt_mmoe_gate_bwd_workspace", nt, ne, S, B, C)
    assert ws_bytes == nt * B * ne * 4
    ws = N.byte_buffer(ws_bytes, "cuda")
    N.call("rlt_mmoe_gate_bwd", N.ptr(hd), N.pointer_array(wd), N.ptr(gd), N.ptr(dgd), nt, ne, S, B, C, N.ptr(dh),
           0 if dh0 is None else 1, N.pointer_array(dw), N.ptr(ws), ws_bytes, N.stream())
    torch.cuda.synchronize()
    return (unpad(dh, S * B * C, "dh").reshape(S * B, C),
            np.stack([unpad(dw[t], S * C * ne, f"dw_gate[{t}]").reshape(S * C, ne) for t in range(nt)]))


# (S, C, B, n_tasks, n_e, accumulate_dh): every S in {1, 2, 3, 5}, C in {1, 63, 64, 65, 256, 257, 320}, B in {1, 63, 64, 65, 130},
# n_tasks in {1, 2, 3}, n_e in {1, 2, 4, 8}, both accumulate_dh - spread over the cases, not the full product
GATE_CASES = [(1, 1, 1, 1, 1, 0), (2, 63, 63, 2, 2, 1), (3, 64, 64, 3, 4, 0), (5, 65, 65, 1, 8, 1), (1, 256, 130, 2, 8, 0),
              (2, 257, 3, 3, 2, 1), (3, 320, 130, 3, 8, 0), (5, 320, 1, 1, 1, 1), (3, 257, 65, 2, 1, 0), (1, 63, 130, 3, 4, 1),
              (2, 1, 64, 3, 8, 0), (5, 256, 63, 2, 4, 1)]
RANDOM_NE = (3, 5, 6, 7)


def gate_id(c):
    S, C, B, nt, ne, acc = c
    return f"gate-dw-C{C}-B{B}-S{S}-nt{nt}-ne{ne}-acc{acc}"


@pytest.mark.parametrize("case", GATE_CASES, ids=gate_id)
def test_gate_bwd_exact(N, case):
    """rlt_mmoe_gate_bwd with uniform gates 1 / n_e handed in (the ABI takes the gates as an input): h integers in [-4, 4],
    w_gate and dgates multiples of 1 / 8 in [-1, 1], dh pre-filled with multiples of 1 / 4 under accumulate_dh.  dlogit is then
    a multiple of 1 / (8 n_e^2), dh of 1 / (64 n_e^2), dw_gate of 1 / (8 n_e^2): all three exact.  n_e = 1: dh exactly zero
    (unchanged under accumulate_dh) and dw_gate exactly zero."""
    S, C, B, nt, ne, acc = case
    g = np.random.default_rng(list(case))
    h = g.integers(-4, 5, size=(S * B, C)).astype(np.float32)
    w = [dyadic(g, (S * C, ne), 1, 8) for _ in range(nt)]
    gates = np.full((nt, B, ne), 1.0 / ne, dtype=np.float32)
    dgates = dyadic(g, (nt, B, ne), 1, 8)
    dh0 = dyadic(g, (S * B, C), 4, 4) if acc else None
    dh, dw = gate_bwd(N, h, w, gates, dgates, S, B, dh0)
    dl, dh_ref, dw_ref = R.gate_bwd(h, w, gates, dgates, S, B)
    absl = np.abs(dl)                                           # the sums of absolute terms of the two linear maps
    flat_abs = R.flatten_lists(np.abs(h), S, B)
    dh_abs = sum(absl[t] @ np.abs(w[t]).astype(F64).T for t in range(nt)).reshape(B, S, C).transpose(1, 0, 2).reshape(S * B, C)
    dw_abs = np.stack([flat_abs.T @ absl[t] for t in range(nt)])
    if acc:
        dh_ref, dh_abs = dh_ref + dh0, dh_abs + np.abs(dh0)
    t = Tally()
    exact(t, "dh", gate_id(case), dh, dh_ref, dh_abs, 1.0 / (64 * ne * ne))
    exact(t, "dw_gate", gate_id(case), dw, dw_ref, dw_abs, 1.0 / (8 * ne * ne))
    if ne == 1:
        assert (dw == 0).all() and np.array_equal(dh, dh0 if acc else np.zeros_like(dh))
    else:
        assert np.abs(dw_ref).max() > 0 and np.abs(dh_ref).max() > 0
    t.done()


def random_gate_operands(S, C, B, nt, ne, seed):
    g = np.random.default_rng(seed)
    h = g.standard_normal((S * B, C)).astype(np.float32)
    w = [(g.standard_normal((S * C, ne)) / np.sqrt(S * C)).astype(np.float32) for _ in range(nt)]
    return g, h, w


def check_gates_and_gradients(N, t, name, h, w, S, B, g, acc):
    """gate_fwd, then gate_bwd from the DEVICE's gates (the chain embed_mmoe's bounds are stated for) and a random dgates"""
    nt, ne = len(w), w[0].shape[1]
    gates = gate_fwd(N, h, w, S, B)
    ref = R.gates(h, w, S, B)
    assert np.isfinite(gates).all(), name
    t.add("gates", name, rel(gates, ref), 2e-5)
    t.add("gate row sum", name, float(np.abs(gates.astype(F64).sum(-1) - 1.0).max()), 1e-6)
    dgates = g.standard_normal((nt, B, ne)).astype(np.float32)
    dh0 = g.standard_normal(h.shape).astype(np.float32) if acc else None
    dh, dw = gate_bwd(N, h, w, gates, dgates, S, B, dh0)
    _, dh_ref, dw_ref = R.gate_bwd(h, w, ref, dgates, S, B)
    assert np.isfinite(dh).all() and np.isfinite(dw).all(), name
    t.add(f"dh accumulate={acc}", name, rel(dh, dh_ref + (dh0 if acc else 0.0)), 1e-4)
    for k in range(nt):
        t.add("dw_gate", f"{name} task {k}", rel(dw[k], dw_ref[k]), 1e-4)


@pytest.mark.parametrize("i", range(len(GATE_CASES)), ids=lambda i: gate_id(GATE_CASES[i][:4] + (RANDOM_NE[i % 4], GATE_CASES[i][5])))
def test_gate_softmax_paths_random(N, i):
    """rlt_mmoe_gate_fwd and rlt_mmoe_gate_bwd (n_e in {3, 5, 6, 7}) at the same edge shapes: h ~ N(0, 1), w_gate ~ N(0, 1) /
    sqrt(S C) as in embed_mmoe."""
    S, C, B, nt, _, acc = GATE_CASES[i]
    ne = RANDOM_NE[i % 4]
    g, h, w = random_gate_operands(S, C, B, nt, ne, 1000 + i)
    t = Tally()
    check_gates_and_gradients(N, t, gate_id((S, C, B, nt, ne, acc)), h, w, S, B, g, acc)
    t.done()


def test_gate_logits_near_100(N):
    """The max subtraction: integer h in [-4, 4] and w_gate = k m / 64 (m an integer in [-8, 8], k one integer for the whole
    case) so that the largest |logit| is 100 within 5 % - exact in fp32 (sums below 2^20 / 64), so that gate_fwd's error is
    that of its softmax alone.  Such a list's gates are one-hot to fp32 and its gate gradient vanishes (below 1e-30 in
    float64, rounding noise of 1e-7 dgates on the device); list 0 has four non-zero entries of +-1 only and keeps logits
    below 10, so that the largest reference gradient is of order one and the relative bounds bind."""
    S, C, B, nt, ne = 3, 65, 5, 3, 5
    g = np.random.default_rng(77)
    h = g.integers(-4, 5, size=(S * B, C)).astype(np.float32)
    hb = h.reshape(S, B, C)
    hb[:, 0, :] = 0.0
    hb[0, 0, :4] = np.array([1, -1, 1, 1], dtype=np.float32)
    m = [g.integers(-8, 9, size=(S * C, ne)).astype(F64) for _ in range(nt)]
    top = np.abs(R.gate_logits(h, m, S, B)).max() / 64.0
    k = int(round(100.0 / top))
    w = [(x * k / 64.0).astype(np.float32) for x in m]
    z = R.gate_logits(h, w, S, B)
    assert all(np.array_equal(w[i].astype(F64) * 64, m[i] * k) for i in range(nt))
    assert 95 <= np.abs(z).max() <= 105 and np.abs(z[:, 0]).max() < 10 and (z.max(-1) - z.min(-1)).max() > 100
    assert R.flatten_lists(np.abs(h), S, B).sum(1).max() * 8 * k < 2 ** 20
    t = Tally()
    check_gates_and_gradients(N, t, "gate-logits-near-100", h, w, S, B, g, 0)
    t.done()


# ---------------------------------------------------------------------------------------------- MMOE mixture
# (E, S, B, n_e, n_tasks): every E in {4, 12, 252, 256, 260, 512}, S in {1, 3, 5}, B in {1, 3, 65}, n_e in {1, 3, 8}, n_tasks in {1, 3}
MIX_CASES = [(4, 1, 1, 1, 1), (12, 3, 3, 3, 3), (252, 5, 65, 8, 1), (256, 1, 3, 3, 3), (260, 3, 65, 1, 3), (512, 5, 1, 8, 3),
             (4, 5, 65, 3, 1), (252, 3, 1, 8, 3)]


def mix_operands(case):
    E, S, B, ne, nt = case
    g = np.random.default_rng(list(case))
    x = g.integers(-4, 5, size=(ne, S * B, E)).astype(np.float32)
    gates = dyadic(g, (nt, B, ne), 1, 8)
    dm = g.integers(-4, 5, size=(nt, S * B, E)).astype(np.float32)
    return x, gates, dm


@pytest.mark.parametrize("case", MIX_CASES, ids=lambda c: "mix-fwd-E%d-S%d-B%d-ne%d-nt%d" % c)
def test_mix_fwd_exact(N, case):
    """rlt_mmoe_mix_fwd: experts integers in [-4, 4], gates multiples of 1 / 8 in [-1, 1]: mixed on the grid 1 / 8, exact"""
    E, S, B, ne, nt = case
    x, gates, _ = mix_operands(case)
    xd, gd = [dev(x[e]) for e in range(ne)], dev(gates)
    mixed = padded(nt * S * B * E, torch.float32)
    N.call("rlt_mmoe_mix_fwd", N.pointer_array(xd), N.ptr(gd), nt, ne, S, B, E, N.ptr(mixed), N.stream())
    torch.cuda.synchronize()
    t = Tally()
    exact(t, "mixed", str(case), unpad(mixed, nt * S * B * E, "mixed").reshape(nt, S * B, E), R.mix_fwd(x, gates, B),
          R.mix_fwd(np.abs(x), np.abs(gates), B), 1.0 / 8)
    t.done()


@pytest.mark.parametrize("case", MIX_CASES, ids=lambda c: "mix-bwd-E%d-S%d-B%d-ne%d-nt%d" % c)
def test_mix_bwd_exact(N, case):
    """rlt_mmoe_mix_bwd: dmixed and experts integers in [-4, 4]: dexperts on the grid 1 / 8, dgates integers below 16 S E"""
    E, S, B, ne, nt = case
    x, gates, dm = mix_operands(case)
    xd, gd, dmd = [dev(x[e]) for e in range(ne)], dev(gates), dev(dm)
    dx = [padded(S * B * E, torch.float32) for _ in range(ne)]
    dg = padded(nt * B * ne, torch.float32)
    N.call("rlt_mmoe_mix_bwd", N.pointer_array(xd), N.ptr(gd), N.ptr(dmd), nt, ne, S, B, E, N.pointer_array(dx), N.ptr(dg), N.stream())
    torch.cuda.synchronize()
    dx_ref, dg_ref = R.mix_bwd(x, gates, dm, B)
    dx_abs, dg_abs = R.mix_bwd(np.abs(x), np.abs(gates), np.abs(dm), B)
    t = Tally()
    got = np.stack([unpad(dx[e], S * B * E, f"dexperts[{e}]").reshape(S * B, E) for e in range(ne)])
    exact(t, "dexperts", str(case), got, dx_ref, dx_abs, 1.0 / 8)
    exact(t, "dgates", str(case), unpad(dg, nt * B * ne, "dgates").reshape(nt, B, ne), dg_ref, dg_abs, 1.0)
    assert np.abs(dg_ref).max() > 0
    t.done()


def test_mmoe_argument_checks(N):
    """host-side refusals, nothing launched: the outputs keep their sentinel"""
    lib = N.load()
    S, B, C, E, nt, ne = 2, 3, 8, 8, 2, 3
    z = lambda *shape: torch.zeros(*shape, device="cuda")                                 # noqa: E731
    h, w, gates, dgates = z(S * B, C), [z(S * C, 8) for _ in range(nt)], z(nt, B, 8), z(nt, B, 8)
    x = [z(S * B, E + 4) for _ in range(9)]
    dx = [padded(S * B * (E + 4), torch.float32) for _ in range(9)]
    out, dh = padded(nt * S * B * (E + 4), torch.float32), padded(S * B * C, torch.float32)
    dw = [padded(S * C * 8, torch.float32) for _ in range(nt)]
    ws_bytes = N.query("rlt_mmoe_gate_bwd_workspace", nt, ne, S, B, C)
    ws = N.byte_buffer(ws_bytes, "cuda")
    st = N.stream()
    xp, dxp, wp, dwp = N.pointer_array(x), N.pointer_array(dx), N.pointer_array(w), N.pointer_array(dw)
    for bad_e in (2, 6, 7):                                                               # E % 4 != 0
        assert lib.rlt_mmoe_mix_fwd(xp, N.ptr(gates), nt, ne, S, B, bad_e, N.ptr(out), st) == E_SHAPE
        assert lib.rlt_mmoe_mix_bwd(xp, N.ptr(gates), N.ptr(out), nt, ne, S, B, bad_e, dxp, N.ptr(dgates), st) == E_SHAPE
    for bad_nt, bad_ne in ((nt, 9), (nt, 0), (4, ne), (0, ne)):                           # n_e = 9 (and the other limits)
        assert lib.rlt_mmoe_mix_fwd(xp, N.ptr(gates), bad_nt, bad_ne, S, B, E, N.ptr(out), st) == E_SHAPE
        assert lib.rlt_mmoe_mix_bwd(xp, N.ptr(gates), N.ptr(out), bad_nt, bad_ne, S, B, E, dxp, N.ptr(dgates), st) == E_SHAPE
        assert lib.rlt_mmoe_gate_fwd(N.ptr(h), wp, bad_nt, bad_ne, S, B, C, N.ptr(out), st) == E_SHAPE
        assert lib.rlt_mmoe_gate_bwd(N.ptr(h), wp, N.ptr(gates), N.ptr(dgates), bad_nt, bad_ne, S, B, C, N.ptr(dh), 0, dwp,
                                     N.ptr(ws), ws_bytes, st) == E_SHAPE
    off = (N.c_void_p * ne)(*[x[e].data_ptr() + (4 if e == 1 else 0) for e in range(ne)])  # an expert pointer 4 bytes off
    assert lib.rlt_mmoe_mix_fwd(off, N.ptr(gates), nt, ne, S, B, E, N.ptr(out), st) == E_ALIGN
    assert lib.rlt_mmoe_mix_bwd(off, N.ptr(gates), N.ptr(out), nt, ne, S, B, E, dxp, N.ptr(dgates), st) == E_ALIGN
    doff = (N.c_void_p * ne)(*[dx[e].data_ptr() + (4 if e == 2 else 0) for e in range(ne)])
    assert lib.rlt_mmoe_mix_bwd(xp, N.ptr(gates), N.ptr(out), nt, ne, S, B, E, doff, N.ptr(dgates), st) == E_ALIGN
    assert lib.rlt_mmoe_mix_fwd(xp, N.ptr(gates), nt, ne, S, B, E, N.c_void_p(out.data_ptr() + 4), st) == E_ALIGN
    assert lib.rlt_mmoe_gate_bwd(N.ptr(h), wp, N.ptr(gates), N.ptr(dgates), nt, ne, S, B, C, N.ptr(dh), 0, dwp,
                                 N.ptr(ws), ws_bytes - 1, st) == E_WORKSPACE            # a short workspace
    assert lib.rlt_mmoe_gate_bwd(N.ptr(h), wp, N.ptr(gates), N.ptr(dgates), nt, ne, S, B, C, N.ptr(dh), 0, dwp,
                                 N.ptr(ws), 0, st) == E_WORKSPACE
    assert lib.rlt_mmoe_gate_fwd(N.ptr(h), wp, nt, ne, 0, B, C, N.ptr(out), st) == E_ARG
    torch.cuda.synchronize()
    for buf in [out, dh] + dx + dw:
        assert (buf == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- pair softmax
def export_mask(N, seed, T, p):
    """rlt_dropout_mask(seed, S * B, 2, p): out[t][col] = rlt_keep(seed, t, col) ? 1 / (1 - p) : 0 (csrc/common.h, the function
    and the threshold bicut.hip's kernels call with row = the position-major token t, col = the class)"""
    m = padded(2 * T, torch.float32)
    N.call("rlt_dropout_mask", seed, T, 2, p, N.ptr(m), N.stream())
    torch.cuda.synchronize()
    m = unpad(m, 2 * T, "mask").reshape(T, 2)
    assert np.isin(m, [np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(p))]).all()
    return m


def pair_fwd(N, z, B, S, p, seed):
    zd = dev(z)
    out = padded(2 * B * S, torch.float32)
    N.call("rlt_pair_softmax_fwd", N.ptr(zd), B, S, p, seed, N.ptr(out), N.stream())
    torch.cuda.synchronize()
    return unpad(out, 2 * B * S, "out").reshape(B, S, 2)


def pair_bwd(N, out, dout, B, S, p, seed):
    od, dd = dev(out), dev(dout)
    dz = padded(2 * B * S, torch.float32)
    N.call("rlt_pair_softmax_bwd", N.ptr(od), N.ptr(dd), B, S, p, seed, N.ptr(dz), N.stream())
    torch.cuda.synchronize()
    return unpad(dz, 2 * B * S, "dz").reshape(S * B, 2)


def check_pair(N, t, name, B, S, p, seed):
    g = np.random.default_rng(B * 1009 + S + seed)
    T = S * B
    z = g.standard_normal((T, 2)).astype(np.float32)
    dout = g.standard_normal((B, S, 2)).astype(np.float32)
    keep = export_mask(N, seed, T, p) if p > 0 else np.ones((T, 2), dtype=np.float32)
    out = pair_fwd(N, z, B, S, p, seed)
    out_ref = R.pair_softmax(z, keep, S, B)
    t.add("fwd", name, rel(out, out_ref), 1e-6)
    t.add("row sum", name, float(np.abs(out.astype(F64).sum(2) - 1.0).max()), 1e-6)
    dz = pair_bwd(N, out, dout, B, S, p, seed)                                             # from the device's own forward
    dz_ref = R.pair_softmax_bwd(out_ref, dout, keep, S, B)
    t.add("bwd", name, rel(dz, dz_ref), 1e-5)
    t.add("dz at dropped logits", name, float((dz[keep == 0] != 0).sum()), 0)
    if T > 4096 * 256:                                                                     # the second round of the grid-stride loop
        tail = slice(4096 * 256, None)
        t.add("fwd, second round", name, rel(R.to_position_major(out)[tail], R.to_position_major(out_ref)[tail]), 1e-6)
        t.add("bwd, second round", name, rel(dz[tail], dz_ref[tail]), 1e-5)


@pytest.mark.parametrize("p", [0.0, 0.3, 0.5], ids=lambda p: f"p{p:g}")
@pytest.mark.parametrize("B,S", [(1, 1), (3, 5), (6, 9), (64, 4), (65, 300)], ids=["pair-B1-S1", "pair-B3-S5", "pair-B6-S9", "pair-B64-S4", "pair-B65-S300"])
def test_pair_softmax(N, B, S, p):
    """rlt_pair_softmax_fwd / _bwd against softmax(z * keep) and keep * softmax' with keep the exported mask (1 at p = 0): the
    output is list-major, the mask indexed by the position-major token, in forward and backward alike"""
    t = Tally()
    check_pair(N, t, f"pair-B{B}-S{S}-p{p:g}", B, S, p, 1234 + S)
    t.done()


def test_pair_softmax_gridstride(N):
    """pair-gridstride: (B, S) = (4099, 257), 1,053,443 tokens: 4867 of them belong to the loop's second round"""
    t = Tally()
    check_pair(N, t, "pair-gridstride", 4099, 257, 0.3, 99)
    t.done()


def recover_mask(out, big_col, p):
    """(B, S, 2) outputs of logits (20, -10) [big_col 0] / (-10, 20) [big_col 1] -> which logits were kept, from the output
    alone: log(larger / smaller) = (1 - p)^-1 * {30: both kept, 20: only the 20 kept, 10: only the -10 kept, 0: neither}"""
    o = out.astype(F64)
    d = np.abs(np.log(o[..., 0]) - np.log(o[..., 1])) * (1.0 - p)
    q = np.rint(d / 10.0)
    assert np.abs(d - 10.0 * q).max() < 0.01 and q.min() >= 0 and q.max() <= 3, "outputs are none of the four values"
    keep_big, keep_small = (q == 3) | (q == 2), (q == 3) | (q == 1)
    keep = np.empty(out.shape, dtype=bool)
    keep[..., 0] = np.where(big_col == 0, keep_big, keep_small)
    keep[..., 1] = np.where(big_col == 1, keep_big, keep_small)
    return keep


@pytest.mark.parametrize("p", [0.3, 0.5], ids=lambda p: f"pair-mask-p{p:g}")
def test_pair_softmax_mask_from_the_forward_alone(N, p):
    """The exported mask must not be the only witness of the mask the kernels use.  Tokens alternate between the logits
    (20, -10) and (-10, 20): the four keep / drop combinations give the four outputs sigmoid(-d / (1 - p)), d = 30, 20, 10, 0,
    orders of magnitude apart and all normal fp32 numbers.  (With (20, -20) and (-20, 20) the softmax, a function of the
    difference alone, gives the same output whichever of the two logits is dropped: three values for four combinations.)
    The mask recovered from the forward output equals the export; its kept share is within 5 binomial standard deviations
    of 1 - p; two seeds give different masks.  Backward: dz is exactly 0 at the dropped logits of the recovered mask.  That
    dz is non-zero where kept is asserted on a second launch with the same seed and shape and logits in [-1, 1] (outputs above 0.017; the mask is
    a function of seed, token and class alone): saturated outputs of exactly 1.0 make y (g - y.g) cancel to 0 in fp32 at
    kept logits too.  dout rows are (u, -v), u, v in [0.5, 1.5]: never degenerate."""
    B, S = 65, 300
    T = S * B
    big_col = (np.arange(S)[None, :] * B + np.arange(B)[:, None]) % 2                      # (B, S): token t = s * B + b is of kind t % 2
    z = np.where((np.arange(T) % 2 == 0)[:, None], np.float32([20, -10]), np.float32([-10, 20])).astype(np.float32)
    g = np.random.default_rng(5)
    dout = (g.uniform(0.5, 1.5, (B, S, 2)) * np.array([1.0, -1.0])).astype(np.float32)
    masks = []
    for seed in (2024, 2025):
        out = pair_fwd(N, z, B, S, p, seed)
        keep = recover_mask(out, big_col, p)                                              # (B, S, 2)
        keep_pm = R.to_position_major(keep)
        export = export_mask(N, seed, T, p)
        assert np.array_equal(keep_pm, export > 0), f"seed {seed}: {(keep_pm != (export > 0)).sum()} mask elements differ"
        share, sd = keep.mean(), np.sqrt(p * (1 - p) / keep.size)
        print(f"  p {p} seed {seed}: kept share {share:.5f}, {(share - (1 - p)) / sd:+.2f} standard deviations from {1 - p}")
        assert abs(share - (1 - p)) <= 5 * sd
        dz = pair_bwd(N, out, dout, B, S, p, seed)
        assert (dz[~keep_pm] == 0).all()
        out2 = pair_fwd(N, g.uniform(-1, 1, (T, 2)).astype(np.float32), B, S, p, seed)
        dz2 = pair_bwd(N, out2, dout, B, S, p, seed)
        assert np.array_equal(dz2 != 0, keep_pm), f"seed {seed}: {((dz2 != 0) != keep_pm).sum()} elements of dz off the mask"
        masks.append(keep_pm)
    differ = (masks[0] != masks[1]).mean()
    print(f"  p {p}: the two seeds' masks differ in {differ:.4f} of their elements (independent masks: {2 * p * (1 - p):.4f})")
    assert differ > 0


# ---------------------------------------------------------------------------------------------- BiCutLoss
ALPHA, RATIO = 0.65, 0.1


def check_bicut(N, t, name, out, labels, idx):
    B, S = labels.shape
    alpha, r = float(np.float32(ALPHA)), float(np.float32(RATIO))                          # what the ABI's float arguments hold
    np.testing.assert_array_equal(R.bicut_last_truncate(out), idx)
    od, yd = dev(out), dev(labels)
    for nci in (1, 0):
        per, loss, dout = padded(B, torch.float32), padded(1, torch.float32), padded(2 * B * S, torch.float32)
        N.call("rlt_bicut_loss", N.ptr(od), N.ptr(yd), B, S, nci, ALPHA, RATIO, N.ptr(per), N.ptr(loss), N.ptr(dout), N.stream())
        torch.cuda.synchronize()
        per, loss, dout = unpad(per, B, "per_list"), float(unpad(loss, 1, "loss")[0]), unpad(dout, 2 * B * S, "dout").reshape(B, S, 2)
        per_ref, loss_ref, dout_ref, mask, abs_terms = R.bicut_loss(out, labels, nci, alpha, r)
        case = f"{name} nci={nci}"
        nz = dout_ref != 0
        assert nz.any() and (abs_terms > 0).all()
        t.add("dout / ref", case, float((np.abs(dout[nz] - dout_ref[nz]) / np.abs(dout_ref[nz])).max()), 1e-6)
        t.add("dout where ref is 0", case, float((dout[~nz] != 0).sum()), 0)
        t.add("dout past the mask", case, float((dout[mask == 0] != 0).sum()), 0)
        t.add("per_list / sum |terms|", case, float((np.abs(per - per_ref) / abs_terms).max()), 1e-5)
        t.add("loss", case, abs(loss - loss_ref) / max(1.0, abs(loss_ref)), 1e-5)


# (B, S, offset into the places): every S in {1, 2, 63, 64, 65, 128, 129, 300, 1025} and B in {1, 3, 4, 5, 1027}; B = 1027 holds every
# place S has and every label fill many times over; the offsets give the small batches different places
BICUT_SHAPES = [(1, 1, 0), (3, 2, 5), (4, 63, 0), (5, 64, 1), (1027, 65, 0), (1, 128, 3), (3, 129, 2), (4, 300, 4), (5, 1025, 5),
                (1027, 129, 0), (1027, 1, 0), (3, 1025, 6), (1027, 300, 0), (1, 300, 6), (5, 129, 3)]


@pytest.mark.parametrize("B,S,offset", BICUT_SHAPES, ids=[f"bicut-B{B}-S{S}" for B, S, _ in BICUT_SHAPES])
def test_bicut_loss_shapes(N, B, S, offset):
    """rlt_bicut_loss on probabilities built directly (bicut_edge_lists): the B % 4 tail of the four-lists-per-workgroup grid,
    B > 256 in the sum kernel, S = 1, S around one and two wavefront rounds and S = 1025; rows with no class-0 position,
    with exact ties, labels all 0 / all 1 / a single 1; both reward forms"""
    out, labels, idx = R.bicut_edge_lists(B, S, offset=offset)
    t = Tally()
    check_bicut(N, t, f"bicut-B{B}-S{S}", out, labels, idx)
    t.done()


@pytest.mark.parametrize("place", [0, 63, 64, 127, 128, "end", "none", "ties"], ids=lambda v: f"bicut-last0-{v}")
def test_bicut_loss_last_class0_position(N, place):
    """every list of the batch with its last class-0 position at one place: a lane boundary of the wavefront-strided scan
    (63 | 64, 127 | 128), the first and the last position, nowhere (nothing masked), exact ties (class 0 wins)"""
    t = Tally()
    for B, S in ((5, 300), (4, 129)):
        out, labels, idx = R.bicut_edge_lists(B, S, only=place)
        want = {"end": S - 1, "none": S, "ties": S // 2}.get(place, place)
        assert (idx == want).all()
        check_bicut(N, t, f"bicut-last0-{place}-B{B}-S{S}", out, labels, idx)
    t.done()


# ---------------------------------------------------------------------------------------------- layout and embedding
def planted(g, shape):
    """N(0, 1) float32 with -0.0, a quiet and a signalling-range NaN payload planted"""
    x = g.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1).view(np.int32)
    n = flat.size
    flat[n // 2] = np.int32(-2 ** 31)                                                      # -0.0
    if n > 1:
        flat[n - 1] = np.int32(0x7FC12345)
    if n > 2:
        flat[0] = np.int32(0x7F812345 - 2 ** 32 + 2 ** 31)                                 # 0xFF812345
    return x


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_layout(N, B, S, F):
    x = planted(np.random.default_rng(B * 10007 + S * 101 + F), (B, S, F))
    n = B * S * F
    xd = dev(x)
    pm = padded(n, torch.float32)
    N.call("rlt_to_position_major", N.ptr(xd), B, S, F, N.ptr(pm), N.stream())
    torch.cuda.synchronize()
    got = unpad(pm, n, "x_sbf").reshape(S * B, F)
    assert np.array_equal(bits(got), bits(R.to_position_major(x)))
    pmd = dev(got)
    back = padded(n, torch.float32)
    N.call("rlt_from_position_major", N.ptr(pmd), B, S, F, N.ptr(back), N.stream())
    torch.cuda.synchronize()
    got_back = unpad(back, n, "x_bsf").reshape(B, S, F)
    assert np.array_equal(bits(got_back), bits(R.from_position_major(got, B, S)))
    assert np.array_equal(bits(got_back), bits(x))                                        # the round trip is the identity
    # from_position_major on its own input, not only on to_position_major's output
    y = planted(np.random.default_rng(n), (S * B, F))
    yd = dev(y)
    back = padded(n, torch.float32)
    N.call("rlt_from_position_major", N.ptr(yd), B, S, F, N.ptr(back), N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(unpad(back, n, "x_bsf").reshape(B, S, F)), bits(R.from_position_major(y, B, S)))


@pytest.mark.parametrize("F", [1, 3, 128], ids=lambda F: f"F{F}")
@pytest.mark.parametrize("B,S", [(1, 1), (3, 5), (65, 7)], ids=["pm-B1-S1", "pm-B3-S5", "pm-B65-S7"])
def test_position_major_maps(N, B, S, F):
    check_layout(N, B, S, F)


def test_position_major_maps_past_the_grid_cap(N):
    """pm-gridcap: (B, S, F) = (257, 129, 128), 4,243,584 elements: 4145 workgroups of 1024 elements wanted, 4096 launched"""
    check_layout(N, 257, 129, 128)


@pytest.mark.parametrize("E", [2, 128], ids=lambda E: f"choopy-E{E}")
@pytest.mark.parametrize("B,S", [(1, 1), (3, 5), (65, 7)], ids=["B1-S1", "B3-S5", "B65-S7"])
def test_choopy_embed(N, B, S, E):
    g = np.random.default_rng(B * 131 + S * 7 + E)
    score, pe = planted(g, (B, S)), planted(g, (S, E - 1))
    sd, ped = dev(score), dev(pe)
    out = padded(S * B * E, torch.float32)
    N.call("rlt_choopy_embed", N.ptr(sd), N.ptr(ped), B, S, E, N.ptr(out), N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(unpad(out, S * B * E, "out").reshape(S * B, E)), bits(R.choopy_embed(score, pe)))
