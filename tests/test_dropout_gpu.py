"""Every train-mode kernel through the raw C ABI against float64 references built from the RESTATED keep mask
(tests/dropout_restate.py, pinned to the header by tests/test_dropout_restate.py) - never from a mask the library exports.

  exporters   rlt_dropout_mask, rlt_attention_dropout_mask and _range equal the restatement bit for bit (this closes the chain for
              the GEMM and BiCut tests, which keep using the exporter).
  attention   rlt_list_attention_fwd / _bwd_prepare / _bwd_dkv / _bwd_dq at S = 2, H = 2 (pairs 1..3 matter), p = 0.3: one id per
              (precision, head dim, B); the kernel of every part is taken from tests/attn_plan_restate.plan and asserted on
              native.attention_plan before the launch.  No environment switch is read or set.  Relative max-norm error, the
              tolerances of tests/test_attention_dispatch_gpu.py: 1e-5 forward, 3e-5 gradients, 6x in bf16x3 mode.
  layer norm  rlt_add_layernorm_fwd / _bwd over every vector width and chunk count, T = 1, 5 and 8195 (the first row count at which
              the grid-stride loop of the 2048-workgroup cap wraps and leaves a partial workgroup), accumulate 0 and 1; 5e-6
              forward, 2e-5 gradients (tools/gpu_probe.py: dropout()); dr exactly 0 where the restated mask is 0.
  python      ops.AddLayerNormFn, FFNFn, ListAttentionFn and EncoderLayerKernelsFn with explicit seeds reproduce the float64
              reference of the restated masks of those seeds: the seed reaches the kernel unchanged, each site its own.

Tolerance fallback (shapes the project never ran before): where a train-mode error exceeds the project tolerance, the same call
is measured with drop_p = 0 against the same reference without a mask, and the bound is 2 / (1 - p) times that eval-mode error -
kept weights are scaled by 1 / (1 - p), the factor 2 allows for the different accumulation order.  A bound is never derived from
the train-mode kernel's own output.  Such ids print a line starting with FALLBACK.

NaN sentinels behind every output and workspace must stay untouched."""
import functools
import math

import numpy as np
import pytest
import torch

import attn_plan_restate as AP
import dropout_restate as D
from gemm_cases import CASES as GEMM_CASES

pytestmark = pytest.mark.gpu

GUARD = 256          # sentinel floats behind every buffer
P_DROP = 0.3
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


def rel(a, b, floor=0.0):
    return float((a.double() - b).abs().max() / (max(float(b.abs().max()), floor) + 1e-30))


def guarded(nbytes):
    """float buffer of at least nbytes, NaN behind it -> (buffer, sentinel view)"""
    n = (max(int(nbytes), 16) + 3) // 4
    full = torch.full((n + GUARD,), float("nan"), device=dev())
    full[:n] = 0.0
    return full[:n], full[n:]


def intact(*ends):
    return all(bool(torch.isnan(e).all()) for e in ends)


def within(name, errs, tols, drop_p, eval_errs):
    """errs <= tols key by key; where not, the fallback bound 2 / (1 - p) * (the eval-mode error of the same call)"""
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    over = [k for k in errs if not errs[k] <= tols[k]]
    if not over:
        return
    ev = eval_errs()
    for k in over:
        bound = 2.0 / (1.0 - drop_p) * ev[k]
        print(f"FALLBACK {name} {k}: train {errs[k]:.3e} eval {ev[k]:.3e} bound {bound:.3e} (project tolerance {tols[k]:.1e})")
        assert errs[k] <= bound, (name, k, errs[k], ev[k], bound)


# ------------------------------------------------------------------------------------------------ exporters
MASK_SHAPES = [(1, 1), (300, 1), (5, 2), (130, 515), (700, 256)] + sorted({(c["M"], c["N"]) for c in GEMM_CASES.values() if c.get("drop")})


@pytest.mark.parametrize("p", (0.0, 0.1, 0.5, BELOW_ONE), ids=("p0", "p0.1", "p0.5", "below1"))
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=[f"{r}x{c}" for r, c in MASK_SHAPES])
def test_dropout_mask_is_the_restatement(N, shape, p):
    rows, cols = shape
    assert (300, 96) in MASK_SHAPES and (256, 256) in MASK_SHAPES and (256, 512) in MASK_SHAPES          # the GEMM dropout ids
    for seed in (4242, 12345):          # 4242: the seed of tests/test_gemm_dispatch_gpu.py
        out, end = guarded(4 * rows * cols)
        N.call("rlt_dropout_mask", seed, rows, cols, p, N.ptr(out), N.stream())
        torch.cuda.synchronize()
        got = out[:rows * cols].cpu().numpy().reshape(rows, cols)
        assert np.array_equal(got, D.mask(seed, rows, cols, p)) and intact(end)


@pytest.mark.parametrize("S,B,H", ((2, 70, 3), (1, 1, 1)))
def test_attention_dropout_mask_is_the_restatement(N, S, B, H):
    seed, n = 4321, S * H * B * B
    want = D.attention_mask(seed, S, B, H, P_DROP)
    assert want.shape == (S * H, B, B)
    out, end = guarded(4 * n)
    N.call("rlt_attention_dropout_mask", seed, S, B, H, P_DROP, N.ptr(out), N.stream())
    torch.cuda.synchronize()
    got = out[:n].cpu().numpy().reshape(S * H, B, B)
    assert np.array_equal(got, want) and intact(end)
    if S * H > 1:
        assert not np.array_equal(got[0], got[1])          # every pair its own stream
    if S * H >= 5:
        part, pend = guarded(4 * 2 * B * B)
        N.call("rlt_attention_dropout_mask_range", seed, 3, 2, B, P_DROP, N.ptr(part), N.stream())
        torch.cuda.synchronize()
        sl = part[:2 * B * B].cpu().numpy().reshape(2, B, B)
        assert np.array_equal(sl, got[3:5]) and np.array_equal(sl, D.attention_mask(seed, S, B, H, P_DROP, pair0=3, npair=2))
        assert intact(pend)


# ------------------------------------------------------------------------------------------------ list attention
ATTN_SEED = 4321
ATTN_S = 2
HEAD_DIMS = {"fp32": (16, 32, 64, 128), "bf16x3": (16, 32, 64), "bf16x6": (16, 32, 64)}
ATTN_CASES = [(prec, HD, B, 2) for prec, hds in HEAD_DIMS.items() for HD in hds for B in (1, 63, 64, 65, 130)]
ATTN_CASES += [("bf16x6", 16, 512, 2), ("bf16x6", 16, 576, 2)]                                        # x6n_2w_seeded: train mode never takes the pipe
ATTN_CASES += [("bf16x6", 64, B, H) for B in (512, 576) for H in (1, 2)]                              # x6h_pipe and its x6_pp fix-up
ATTN_CASES += [("bf16x6", 64, 520, 2)]                                                                # x6_pp over nine tiles, the last ragged
# one id per kernel family, two tiles with a ragged second one: the flipped entry (last query, last key) lies in the ragged tile
SENSITIVITY = [("fp32", 16, 65, 2), ("fp32", 32, 65, 2), ("fp32", 64, 65, 2), ("fp32", 128, 65, 2), ("bf16x3", 32, 65, 2),
               ("bf16x6", 16, 65, 2), ("bf16x6", 32, 65, 2), ("bf16x6", 64, 65, 2)]
# what the grid must reach, by part
REACHED = {"fwd": {"f32_hd16", "f32", "f32_sb", "x3", "x6", "x6n_2w", "x6n_2w_seeded", "x6_pp", "x6h_pipe"},
           "dkv": {"f32_hd16", "f32", "f32_occ1", "x3", "x6", "x6n_2w", "x6n_2w_seeded", "x6_dkv1"},
           "dq": {"f32_hd16", "f32", "x3", "x6", "x6n_2w", "x6n_2w_seeded", "x6_dq1"}}


def attn_id(c):
    return f"{c[0]}-hd{c[1]}-B{c[2]}" + ("" if c[3] == 2 else f"-H{c[3]}")


def attn_tols(prec):
    scale = 6.0 if prec == "bf16x3" else 1.0
    return {"fwd": 1e-5 * scale, "dq": 3e-5 * scale, "dk": 3e-5 * scale, "dv": 3e-5 * scale}


def attn_reference(qkv, dout, S, B, H, HD, mask):
    """fp64 on the device; mask: (S * H, B, B) over (pair, query, key) or None.  Position-major in and out."""
    E = H * HD
    q = qkv.double().reshape(S, B, 3, H, HD).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)      # (3, S, H, B, HD)
    p = torch.softmax(q[0] @ q[1].transpose(-1, -2) / math.sqrt(HD), -1)
    if mask is not None:
        p = p * torch.as_tensor(mask, device=qkv.device).double().reshape(S, H, B, B)
    o = (p @ q[2]).permute(0, 2, 1, 3).reshape(S * B, E)
    o.backward(dout.double())
    return o.detach(), q.grad.permute(1, 3, 0, 2, 4).reshape(S * B, 3 * E)


def attn_errors(out, dqkv, ref, E, floors=(0.0, 0.0)):
    o_ref, g_ref = ref
    return {"fwd": rel(out, o_ref), "dq": rel(dqkv[:, :E], g_ref[:, :E], floors[0]), "dk": rel(dqkv[:, E:2 * E], g_ref[:, E:2 * E], floors[1]),
            "dv": rel(dqkv[:, 2 * E:], g_ref[:, 2 * E:])}


def single_list_floors(qkv, dout, H, HD, drop_p):
    """B = 1: the one softmax weight is 1 whatever the scores, so dQ and dK are exactly 0 and a relative error has no denominator.
    The kernels get that 0 as P (dP - delta), the difference of two equal terms each rounded on its own (dP = dO . V / (1 - p) from
    the tile, delta = dO . O from the prepare pass).  Their error is measured against the size of one of those terms carried to dQ
    and dK: max |dO . V| / (1 - p) * max |K| (or |Q|) / sqrt(HD)."""
    E = H * HD
    q, k, v = (qkv[:, i * E:(i + 1) * E].double().reshape(-1, H, HD) for i in range(3))
    dp = float((dout.double().reshape(-1, H, HD) * v).sum(-1).abs().max()) / (1.0 - drop_p)
    return dp * float(k.abs().max()) / math.sqrt(HD), dp * float(q.abs().max()) / math.sqrt(HD)


@functools.lru_cache(maxsize=2)
def attn_inputs(B, H, HD):
    g = torch.Generator().manual_seed(B * 131 + HD * 7 + H)
    E = H * HD
    return torch.randn(ATTN_S * B, 3 * E, generator=g).to(dev()), torch.randn(ATTN_S * B, E, generator=g).to(dev())


def attn_run(N, prec, HD, B, H, drop_p):
    """the four entry points on guarded buffers, the plan asserted first -> (out, dqkv)"""
    S, E, code, seed = ATTN_S, H * HD, N.precision_code(prec), ATTN_SEED
    want = AP.plan(S, B, H, HD, drop_p, 1, prec)
    plan = N.attention_plan(S, B, H, HD, drop_p, 1, code)
    for f in ("fwd", "fwd_fixup", "dkv", "dq", "images_bytes", "images_retained", "ws_bytes"):
        assert plan[f] == want[f], (f, plan[f], want[f])
    qkv, dout = attn_inputs(B, H, HD)
    ib, wb, ptr, st = plan["images_bytes"], plan["ws_bytes"], N.ptr, N.stream()
    assert ib == N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, drop_p, code)
    assert wb == N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, drop_p, code)
    out, out_end = guarded(4 * S * B * E)
    lse, lse_end = guarded(4 * S * H * B)
    images, images_end = guarded(ib)
    ws, ws_end = guarded(wb)
    dqkv, dqkv_end = guarded(4 * S * B * 3 * E)
    N.call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, drop_p, seed, ptr(out), ptr(lse), ptr(images) if ib else None, ib, code, st)
    img = ptr(images) if ib and plan["images_retained"] else None
    N.call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, drop_p, img, ptr(ws), wb, code, st)
    N.call("rlt_list_attention_bwd_dkv", ptr(qkv), ptr(dout), ptr(lse), img, ptr(ws), wb, S, B, H, HD, drop_p, seed, ptr(dqkv), code, st)
    N.call("rlt_list_attention_bwd_dq", ptr(qkv), ptr(dout), ptr(lse), img, ptr(ws), wb, S, B, H, HD, drop_p, seed, ptr(dqkv), code, st)
    torch.cuda.synchronize()
    assert intact(out_end, lse_end, images_end, ws_end, dqkv_end), "sentinel overwritten"
    return out[:S * B * E].reshape(S * B, E), dqkv[:S * B * 3 * E].reshape(S * B, 3 * E)


def test_attention_grid_reaches_every_train_mode_kernel():
    got = {"fwd": set(), "dkv": set(), "dq": set()}
    fixups = set()
    for prec, HD, B, H in ATTN_CASES:
        p = AP.plan(ATTN_S, B, H, HD, P_DROP, 1, prec)
        for part in got:
            got[part].add(p[part])
        fixups.add((p["fwd"], p["fwd_fixup"]))
    assert got == REACHED, got
    assert ("x6h_pipe", "x6_pp") in fixups
    assert all(c in ATTN_CASES for c in SENSITIVITY) and len(ATTN_CASES) == 57


@pytest.mark.parametrize("case", ATTN_CASES, ids=[attn_id(c) for c in ATTN_CASES])
def test_attention_train_mode(N, case):
    prec, HD, B, H = case
    S, E = ATTN_S, H * HD
    qkv, dout = attn_inputs(B, H, HD)
    mask = D.attention_mask(ATTN_SEED, S, B, H, P_DROP)
    out, dqkv = attn_run(N, prec, HD, B, H, P_DROP)
    floors = single_list_floors(qkv, dout, H, HD, P_DROP) if B == 1 else (0.0, 0.0)
    errs = attn_errors(out, dqkv, attn_reference(qkv, dout, S, B, H, HD, mask), E, floors)
    tols = attn_tols(prec)

    def eval_errs():
        o0, g0 = attn_run(N, prec, HD, B, H, 0.0)
        return attn_errors(o0, g0, attn_reference(qkv, dout, S, B, H, HD, None), E, floors)

    within(attn_id(case), errs, tols, P_DROP, eval_errs)
    if case in SENSITIVITY:
        # One wrong keep decision moves an output row by about softmax weight * v / (1 - p), here about 1 / 65 of the largest
        # output: the comparison must see it, at more than ten times its tolerance.
        flipped = mask.copy()
        flipped[-1, -1, -1] = D.keep_scale(P_DROP) - flipped[-1, -1, -1]
        wrong = attn_errors(out, dqkv, attn_reference(qkv, dout, S, B, H, HD, flipped), E)
        print("one flipped entry:", {k: f"{v:.2e}" for k, v in wrong.items()})
        assert wrong["fwd"] > 10 * tols["fwd"] and wrong["dv"] > 10 * tols["dv"], wrong


# ------------------------------------------------------------------------------------------------ residual + LayerNorm
LN_SEED = 12345
LN_EPS = 1e-5
LN_TOLS = {"y": 5e-6, "dz": 2e-5, "dr": 2e-5, "dgamma": 2e-5, "dbeta": 2e-5}
LN_E = (64, 192, 128, 384, 256, 1024)          # V = 1: one and three chunks per lane; V = 2: one and three; V = 4: one and four
LN_T = (1, 5, 8195)


@functools.lru_cache(maxsize=1)
def ln_problem(T, E):
    """inputs, the restated mask and the float64 references with and without it; shared by the accumulate ids, never modified"""
    g = torch.Generator().manual_seed(T * 31 + E)
    x, r, dy = (torch.randn(T, E, generator=g).to(dev()) for _ in range(3))
    gamma, beta, dg0, db0 = (torch.randn(E, generator=g).to(dev()) for _ in range(4))
    mask = torch.from_numpy(D.mask(LN_SEED, T, E, P_DROP)).to(dev())

    def ref(m):
        xr, rr, gr, br = (t.double().requires_grad_(True) for t in (x, r, gamma, beta))
        z = xr + (rr if m is None else rr * m.double())
        y = torch.nn.functional.layer_norm(z, (E,), gr, br, LN_EPS)
        y.backward(dy.double())
        return {"y": y.detach(), "dz": xr.grad, "dr": rr.grad, "dgamma": gr.grad, "dbeta": br.grad}

    return (x, r, dy, gamma, beta, dg0, db0, mask), ref(mask), ref(None)


def ln_run(N, T, E, drop_p, accumulate):
    (x, r, dy, gamma, beta, dg0, db0, _), _, _ = ln_problem(T, E)
    ptr, st = N.ptr, N.stream()
    y, y_end = guarded(4 * T * E)
    stats, stats_end = guarded(4 * T * 2)
    dz, dz_end = guarded(4 * T * E)
    dr, dr_end = guarded(4 * T * E)
    dgamma, dg_end = guarded(4 * E)
    dbeta, db_end = guarded(4 * E)
    wb = N.query("rlt_add_layernorm_bwd_workspace", T, E)
    assert wb == min((T + 3) // 4, 2048) * 2 * E * 4
    ws, ws_end = guarded(wb)
    if accumulate:
        dgamma[:E] = dg0
        dbeta[:E] = db0
    N.call("rlt_add_layernorm_fwd", ptr(x), ptr(r), ptr(gamma), ptr(beta), T, E, LN_EPS, drop_p, LN_SEED, ptr(y), ptr(stats), st)
    N.call("rlt_add_layernorm_bwd", ptr(x), ptr(r), ptr(gamma), ptr(stats), ptr(dy), T, E, drop_p, LN_SEED, ptr(dz),
           ptr(dr) if drop_p > 0 else None, ptr(dgamma), ptr(dbeta), accumulate, ptr(ws), wb, st)
    torch.cuda.synchronize()
    assert intact(y_end, stats_end, dz_end, dr_end, dg_end, db_end, ws_end), "sentinel overwritten"
    return {"y": y[:T * E].reshape(T, E), "dz": dz[:T * E].reshape(T, E), "dr": dr[:T * E].reshape(T, E), "dgamma": dgamma[:E],
            "dbeta": dbeta[:E]}


def ln_errors(got, ref, accumulate, dg0, db0, with_dr=True):
    want = dict(ref)
    if accumulate:
        want["dgamma"], want["dbeta"] = ref["dgamma"] + dg0.double(), ref["dbeta"] + db0.double()
    return {k: rel(got[k], want[k]) for k in LN_TOLS if with_dr or k != "dr"}


@pytest.mark.parametrize("accumulate", (0, 1), ids=("set", "acc"))
@pytest.mark.parametrize("T", LN_T)
@pytest.mark.parametrize("E", LN_E)
def test_add_layernorm_train_mode(N, E, T, accumulate):
    (x, r, dy, gamma, beta, dg0, db0, mask), ref, ref_eval = ln_problem(T, E)
    got = ln_run(N, T, E, P_DROP, accumulate)
    errs = ln_errors(got, ref, accumulate, dg0, db0)

    def eval_errs():
        ev = ln_errors(ln_run(N, T, E, 0.0, accumulate), ref_eval, accumulate, dg0, db0, with_dr=False)
        ev["dr"] = ev["dz"]          # without dropout the gradient of r is dz itself
        return ev

    within(f"add_ln E{E} T{T} acc{accumulate}", errs, LN_TOLS, P_DROP, eval_errs)
    dropped = mask == 0
    assert 0 < int(dropped.sum()) < T * E or T * E < 64
    assert bool((got["dr"][dropped] == 0).all()), "dr must be exactly 0 where the restated mask drops"
    assert bool((got["dr"][~dropped] == got["dz"][~dropped] * mask[~dropped]).all())          # and dz / (1 - p), one fp32 product, elsewhere


# ------------------------------------------------------------------------------------------------ the Python layer
def mode_scale(N):
    return 6.0 if N.get_precision() == "bf16x3" else 1.0


def test_add_layernorm_fn_passes_its_seed(N):
    from rlt_hip import ops
    T, E, seed = 37, 192, 987654321
    g = torch.Generator().manual_seed(1)
    x, r, dy = (torch.randn(T, E, generator=g) for _ in range(3))
    gamma, beta = torch.randn(E, generator=g), torch.randn(E, generator=g)
    mask = torch.from_numpy(D.mask(seed, T, E, P_DROP)).double()
    refs = [t.clone().double().requires_grad_(True) for t in (x, r, gamma, beta)]
    yr = torch.nn.functional.layer_norm(refs[0] + refs[1] * mask, (E,), refs[2], refs[3], LN_EPS)
    yr.backward(dy.double())
    devs = [t.clone().to(dev()).requires_grad_(True) for t in (x, r, gamma, beta)]
    yd = ops.AddLayerNormFn.apply(*devs, LN_EPS, P_DROP, seed)
    yd.backward(dy.to(dev()))
    errs = {"y": rel(yd.detach().cpu(), yr.detach())}
    errs.update({k: rel(a.grad.cpu(), b.grad) for k, a, b in zip(("dz", "dr", "dgamma", "dbeta"), devs, refs)})
    print(errs)
    assert all(errs[k] <= LN_TOLS[k] for k in errs), errs
    other = torch.from_numpy(D.mask(seed + 1, T, E, P_DROP)).double()
    assert rel(yd.detach().cpu(), torch.nn.functional.layer_norm(x.double() + r.double() * other, (E,), gamma.double(), beta.double(),
                                                                 LN_EPS)) > 1e-2          # and no other seed's


def test_ffn_fn_passes_its_seed(N):
    from rlt_hip import ops
    T, E, Fh, seed = 70, 64, 96, 3000000001
    g = torch.Generator().manual_seed(2)
    x, dy = torch.randn(T, E, generator=g), torch.randn(T, E, generator=g)
    w1, b1 = torch.randn(Fh, E, generator=g) / 8, torch.randn(Fh, generator=g) / 10
    w2, b2 = torch.randn(E, Fh, generator=g) / 10, torch.randn(E, generator=g) / 10
    mask = torch.from_numpy(D.mask(seed, T, Fh, P_DROP)).double()
    refs = [t.clone().double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    devs = [t.clone().to(dev()).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    # ReLU is discontinuous at 0: on a pre-activation within rounding distance of zero the reference follows the branch the device
    # took (tools/gpu_probe.py: dropout()); everywhere else it is the sign of the float64 value
    z = refs[0] @ refs[1].t() + refs[2]
    hd = torch.empty(T, Fh, device=dev())
    ops.gemm(0, 1, T, Fh, E, devs[0].detach(), E, devs[1].detach(), E, hd, Fh, bias=devs[2].detach(), flags=N.GEMM_RELU)
    gate = torch.where(z.detach().abs() < 1e-4, hd.cpu() > 0, z.detach() > 0).double()
    yr = (z * gate * mask) @ refs[3].t() + refs[4]
    yr.backward(dy.double())
    yd = ops.FFNFn.apply(*devs, P_DROP, seed)
    yd.backward(dy.to(dev()))
    s = mode_scale(N)
    errs = {"y": rel(yd.detach().cpu(), yr.detach())}
    errs.update({k: rel(a.grad.cpu(), b.grad) for k, a, b in zip(("dx", "dw1", "db1", "dw2", "db2"), devs, refs)})
    print(errs)
    assert errs["y"] <= 1e-5 * s and all(v <= 3e-5 * s for k, v in errs.items() if k != "y"), errs


def test_list_attention_fn_passes_its_seed(N):
    from rlt_hip import ops
    S, B, H, HD, seed = 2, 70, 2, 16, 0xFFFFFFFF
    E = H * HD
    g = torch.Generator().manual_seed(3)
    qkv, dout = torch.randn(S * B, 3 * E, generator=g).to(dev()), torch.randn(S * B, E, generator=g).to(dev())
    ref = attn_reference(qkv, dout, S, B, H, HD, D.attention_mask(seed, S, B, H, P_DROP))
    qd = qkv.clone().requires_grad_(True)
    od = ops.ListAttentionFn.apply(qd, S, B, H, P_DROP, seed)
    od.backward(dout)
    errs = attn_errors(od.detach(), qd.grad, ref, E)
    print(errs)
    s = mode_scale(N)
    assert errs["fwd"] <= 1e-5 * s and max(errs["dq"], errs["dk"], errs["dv"]) <= 3e-5 * s, errs


def test_encoder_layer_gives_each_site_its_own_seed(N):
    """One EncoderLayerKernelsFn forward with four distinct seeds (attention, LayerNorm 1, FFN hidden, LayerNorm 2) against the
    float64 layer built from the four restated masks.  Bound 1e-4 of the largest output - the bound of the layer-level checks
    (smoke()): six kernels, each within 1e-5 .. 3e-5 of float64 on its own, through two LayerNorms of gain O(1).  A seed that
    reached another site changes 30 % of that site's elements by O(1): the reference with two seeds swapped must be 100 x further."""
    from rlt_hip import ops
    S, B, H, E, FF = 2, 20, 2, 64, 96
    T, HD = S * B, E // H
    seeds = (11, 22, 33, 44)
    g = torch.Generator().manual_seed(4)
    rn = lambda *shape, div=1.0: (torch.randn(*shape, generator=g) / div).to(dev())
    x = rn(T, E)
    w = dict(in_w=rn(3 * E, E, div=8), in_b=rn(3 * E, div=10), out_w=rn(E, E, div=8), out_b=rn(E, div=10), n1_w=rn(E), n1_b=rn(E),
             w1=rn(FF, E, div=8), b1=rn(FF, div=10), w2=rn(E, FF, div=10), b2=rn(E, div=10), n2_w=rn(E), n2_b=rn(E))
    with torch.no_grad():
        y = ops.EncoderLayerKernelsFn.apply(x, *w.values(), S, B, H, LN_EPS, P_DROP, seeds)
    torch.cuda.synchronize()

    # the four sites draw masks that differ, exported and restated alike
    exported = []
    for s in seeds:
        m, end = guarded(4 * T * E)
        N.call("rlt_dropout_mask", s, T, E, P_DROP, N.ptr(m), N.stream())
        torch.cuda.synchronize()
        exported.append(m[:T * E].cpu().numpy().reshape(T, E))
        assert np.array_equal(exported[-1], D.mask(s, T, E, P_DROP)) and intact(end)
    assert all(not np.array_equal(exported[a], exported[b]) for a in range(4) for b in range(a + 1, 4))

    def layer(s_attn, s_ln1, s_ffn, s_ln2):
        d = {k: v.double() for k, v in w.items()}
        ln = torch.nn.functional.layer_norm
        mk = lambda s, rows, cols: torch.from_numpy(D.mask(s, rows, cols, P_DROP)).to(dev()).double()
        qkv = x.double() @ d["in_w"].t() + d["in_b"]
        q = qkv.reshape(S, B, 3, H, HD).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q[0] @ q[1].transpose(-1, -2) / math.sqrt(HD), -1)
        p = p * torch.from_numpy(D.attention_mask(s_attn, S, B, H, P_DROP)).to(dev()).double().reshape(S, H, B, B)
        att = (p @ q[2]).permute(0, 2, 1, 3).reshape(T, E)
        h1 = ln(x.double() + (att @ d["out_w"].t() + d["out_b"]) * mk(s_ln1, T, E), (E,), d["n1_w"], d["n1_b"], LN_EPS)
        hid = torch.relu(h1 @ d["w1"].t() + d["b1"]) * mk(s_ffn, T, FF)
        return ln(h1 + (hid @ d["w2"].t() + d["b2"]) * mk(s_ln2, T, E), (E,), d["n2_w"], d["n2_b"], LN_EPS)

    err = rel(y, layer(*seeds))
    swapped = {"ln1<->ln2": rel(y, layer(11, 44, 33, 22)), "attn<->ffn": rel(y, layer(33, 22, 11, 44)),
               "attn<->ln1": rel(y, layer(22, 11, 33, 44)), "ffn<->ln2": rel(y, layer(11, 22, 44, 33))}
    print(err, swapped)
    tol = 1e-4 * mode_scale(N)
    assert err <= tol, err
    assert all(v > 100 * tol for v in swapped.values()), swapped
