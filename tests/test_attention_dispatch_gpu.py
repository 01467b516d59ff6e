"""One test id per kernel the list-attention plan can name under the default switches, at the smallest shape of the plan grid
(tests/attn_plan_restate.py) that reaches it: the plan's kernel code is asserted first, then the forward and dQ / dK / dV are
compared with the fp64 reference of tools/gpu_probe.py (_attn_ref; the same relative max-norm error and tolerances: 1e-5
forward, 3e-5 gradients, 6x in bf16x3 mode).  NaN sentinels behind `images`, the workspace and dqkv must stay untouched.
No environment switch is read or set: RLT_ATTN_X6_IMG / _X6_PP_IMG need RLT_ATTN6_IMG=1 and are pinned by the plan test only.
One shape per kernel: the eval-mode kernels at their tile edges, lse, delta, the fix-up flag words and the order of the backward
parts are tests/test_attention_edges_gpu.py; the train-mode kernels at theirs, tests/test_dropout_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# id = the kernel; (part, precision, S, B, H, HD, drop_p)
CASES = {
    "f32": ("fwd", "fp32", 2, 130, 2, 32, 0.0),
    "f32_sb": ("fwd", "fp32", 1, 448, 1, 64, 0.0),
    "f32_occ1": ("dkv", "fp32", 1, 130, 1, 128, 0.0),
    "f32_hd16": ("fwd", "fp32", 2, 64, 1, 16, 0.0),
    "x3": ("fwd", "bf16x3", 2, 130, 2, 32, 0.0),
    "x6": ("fwd", "bf16x6", 2, 130, 2, 32, 0.0),
    "x6_pp": ("fwd", "bf16x6", 1, 448, 1, 64, 0.0),
    "x6_dkv1": ("dkv", "bf16x6", 1, 448, 1, 64, 0.0),
    "x6_dq1": ("dq", "bf16x6", 1, 448, 1, 64, 0.0),
    "x6_backward_beyond_24_bits": ("dkv", "bf16x6", 1, 4096, 22, 64, 0.0),      # x6 for dK+dV and dQ at head dim 64
    "x6n_2w": ("fwd", "bf16x6", 2, 64, 1, 16, 0.0),
    "x6n_2w_seeded": ("fwd", "bf16x6", 1, 576, 1, 16, 0.0),
    "x6n_2w_seeded_train": ("dkv", "bf16x6", 1, 576, 1, 16, 0.1),
    "x6n_pipe": ("fwd", "bf16x6", 1, 512, 1, 16, 0.0),
    "x6n_pipe_backward": ("dkv", "bf16x6", 1, 576, 1, 16, 0.0),
    "x6h_pipe": ("fwd", "bf16x6", 1, 512, 1, 64, 0.0),
    "x6h_pipe_train": ("fwd", "bf16x6", 1, 512, 1, 64, 0.1),
}
EXPECT = {"x6_backward_beyond_24_bits": "x6", "x6n_2w_seeded_train": "x6n_2w_seeded", "x6n_pipe_backward": "x6n_pipe",
          "x6h_pipe_train": "x6h_pipe"}
GUARD = 256          # sentinel floats behind every buffer


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


def guarded(nbytes, dev):
    """float buffer of at least nbytes, NaN behind it -> (buffer, sentinel view)"""
    n = (max(int(nbytes), 16) + 3) // 4
    full = torch.full((n + GUARD,), float("nan"), device=dev)
    full[:n] = 0.0
    return full[:n], full[n:]


def reference(N, qkv, dout, S, B, H, HD, drop_p, seed):
    """fp64 on the device, gpu_probe's _attn_ref (with the kernels' keep mask in train mode): position-major in and out"""
    E = H * HD
    q = qkv.double().reshape(S, B, 3, H, HD).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)      # (3, S, H, B, HD)
    p = torch.softmax(q[0] @ q[1].transpose(-1, -2) / math.sqrt(HD), -1)
    if drop_p > 0:
        mask = torch.empty(S, H, B, B, device=qkv.device)
        N.call("rlt_attention_dropout_mask", seed, S, B, H, drop_p, N.ptr(mask), N.stream())
        p = p * mask.double()
    o = (p @ q[2]).permute(0, 2, 1, 3).reshape(S * B, E)
    o.backward(dout.double())
    return o.detach(), q.grad.permute(1, 3, 0, 2, 4).reshape(S * B, 3 * E)


@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_kernel(N, name):
    part, prec, S, B, H, HD, drop_p = CASES[name]
    dev, code, seed, E = torch.device("cuda"), N.precision_code(prec), 4321, H * HD
    plan = N.attention_plan(S, B, H, HD, drop_p, 1, code)
    assert plan[part] == EXPECT.get(name, name), plan
    if name == "x6_backward_beyond_24_bits":
        assert plan["dq"] == "x6"
    g = torch.Generator().manual_seed(B * 131 + HD)
    qkv = torch.randn(S * B, 3 * E, generator=g).to(dev)
    dout = torch.randn(S * B, E, generator=g).to(dev)
    out, lse = torch.empty(S * B, E, device=dev), torch.empty(S, H, B, device=dev)
    assert plan["images_bytes"] == N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, drop_p, code)
    assert plan["ws_bytes"] == N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, drop_p, code)
    images, images_end = guarded(plan["images_bytes"], dev)
    ws, ws_end = guarded(plan["ws_bytes"], dev)
    dqkv, dqkv_end = guarded(4 * S * B * 3 * E, dev)
    ib, wb, ptr, st = plan["images_bytes"], plan["ws_bytes"], N.ptr, N.stream()
    N.call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, drop_p, seed, ptr(out), ptr(lse), ptr(images) if ib else None, ib, code, st)
    img = ptr(images) if ib and plan["images_retained"] else None
    N.call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, drop_p, img, ptr(ws), wb, code, st)
    N.call("rlt_list_attention_bwd_dkv", ptr(qkv), ptr(dout), ptr(lse), img, ptr(ws), wb, S, B, H, HD, drop_p, seed, ptr(dqkv), code, st)
    N.call("rlt_list_attention_bwd_dq", ptr(qkv), ptr(dout), ptr(lse), img, ptr(ws), wb, S, B, H, HD, drop_p, seed, ptr(dqkv), code, st)
    torch.cuda.synchronize()
    o_ref, g_ref = reference(N, qkv, dout, S, B, H, HD, drop_p, seed)
    scale = 6.0 if prec == "bf16x3" else 1.0
    got = dqkv[:S * B * 3 * E].reshape(S * B, 3 * E)
    errs = {"fwd": rel(out, o_ref), "dq": rel(got[:, :E], g_ref[:, :E]), "dk": rel(got[:, E:2 * E], g_ref[:, E:2 * E]),
            "dv": rel(got[:, 2 * E:], g_ref[:, 2 * E:])}
    print(name, errs)
    assert errs["fwd"] <= 1e-5 * scale, errs
    assert max(errs["dq"], errs["dk"], errs["dv"]) <= 3e-5 * scale, errs
    for end in (images_end, ws_end, dqkv_end):
        assert bool(torch.isnan(end).all()), "sentinel overwritten"
