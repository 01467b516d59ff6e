#!/usr/bin/env python3
"""Developer micro-benchmark (GPU box): time the MFMA kernels at the BASELINE configs[1] shapes
(AttnCut, 4096 lists x 300) with HIP events and print TFLOP/s.  Variants are selected with the
RLT_* environment variables the library reads at launch."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "ranked-list-truncation_amd"))

import torch

from rlt_hip import native as N
from rlt_hip import ops
from rlt_hip.native import call, ptr, stream

dev = torch.device("cuda")


def timeit(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def attention(B=4096, S=60, H=4, HD=64, drop=0.0):
    E = H * HD
    T = S * B
    qkv = torch.randn(T, 3 * E, device=dev)
    out = torch.empty(T, E, device=dev)
    lse = torch.empty(S, H, B, device=dev)
    dout = torch.randn(T, E, device=dev)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(S, H, B, device=dev)
    unit = B * B * HD * S * H / 1e9     # GFLOP per "2*B*B*HD" product /2
    ib = N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, drop, N.PRECISION_DEFAULT)
    images = torch.empty(max(ib, 16) // 4, device=dev) if ib else None
    wb = N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, drop, N.PRECISION_DEFAULT)
    ws = torch.empty(wb // 4 + 4, device=dev)
    ms = timeit(lambda: call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, drop, 7, ptr(out), ptr(lse), ptr(images), ib, N.PRECISION_DEFAULT, stream()))
    print(f"attn_fwd      B{B} S{S} HD{HD}: {ms:8.3f} ms  {4 * unit / ms:7.1f} TF/s", flush=True)
    ms = timeit(lambda: call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, drop, ptr(images), ptr(ws), wb, N.PRECISION_DEFAULT, stream()))
    print(f"attn_bwd_prep B{B} S{S} HD{HD}: {ms:8.3f} ms", flush=True)
    ms = timeit(lambda: call("rlt_list_attention_bwd_dkv", ptr(qkv), ptr(dout), ptr(lse), ptr(images), ptr(ws), wb, S, B, H, HD, drop, 7, ptr(dqkv), N.PRECISION_DEFAULT, stream()))
    print(f"attn_bwd_dkv  B{B} S{S} HD{HD}: {ms:8.3f} ms  {8 * unit / ms:7.1f} TF/s", flush=True)
    ms = timeit(lambda: call("rlt_list_attention_bwd_dq", ptr(qkv), ptr(dout), ptr(lse), ptr(images), ptr(ws), wb, S, B, H, HD, drop, 7, ptr(dqkv), N.PRECISION_DEFAULT, stream()))
    print(f"attn_bwd_dq   B{B} S{S} HD{HD}: {ms:8.3f} ms  {6 * unit / ms:7.1f} TF/s", flush=True)


def attention_fwd(B=4096, S=60, H=4, HD=64):
    """The forward launch alone (its prepare passes and fix-up launch included)."""
    E = H * HD
    T = S * B
    qkv = torch.randn(T, 3 * E, device=dev)
    out = torch.empty(T, E, device=dev)
    lse = torch.empty(S, H, B, device=dev)
    ib = N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, 0.0, N.PRECISION_DEFAULT)
    images = torch.empty(max(ib, 16) // 4, device=dev) if ib else None
    ms = timeit(lambda: call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, 0.0, 7, ptr(out), ptr(lse), ptr(images), ib, N.PRECISION_DEFAULT, stream()), reps=5, warm=2)
    print(f"attn_fwd      B{B} S{S} HD{HD}: {ms:8.3f} ms  {4 * B * B * HD * S * H / 1e9 / ms:7.1f} TF/s", flush=True)


def attention_drop():
    """AttnCut's conf dropout (0.4) and Choopy's (0.2)."""
    print("dropout 0.4:", flush=True)
    attention(drop=0.4)
    print("dropout 0.2, head dim 16:", flush=True)
    attention(B=8192, S=20, H=8, HD=16, drop=0.2)


def attention16():
    """Choopy's shape (BASELINE configs[2]): 8192 lists, 8 heads x 16."""
    attention(B=8192, S=20, H=8, HD=16)


def gemms(T=4096 * 300):
    shapes = [("in_proj fwd NT", 0, 1, T, 768, 256), ("ffn1 fwd NT", 0, 1, T, 2048, 256), ("ffn2 fwd NT", 0, 1, T, 256, 2048),
              ("ffn1 dX NN", 0, 0, T, 256, 2048), ("ffn2 dX NN", 0, 0, T, 2048, 256),
              ("ffn1 dW TN", 1, 0, 2048, 256, T), ("ffn2 dW TN", 1, 0, 256, 2048, T), ("in_proj dW TN", 1, 0, 768, 256, T),
              ("lstm dWhh TN", 1, 0, 512, 128, T)]
    for name, ta, tb, M, Nn, K in shapes:
        A = torch.randn((K, M) if ta else (M, K), device=dev)
        Bm = torch.randn((Nn, K) if tb else (K, Nn), device=dev)
        C = torch.empty(M, Nn, device=dev)
        bias = torch.randn(Nn, device=dev)
        ms = timeit(lambda: ops.gemm(ta, tb, M, Nn, K, A, A.shape[1], Bm, Bm.shape[1], C, Nn, bias=bias))
        print(f"gemm {name:16s} {M}x{Nn}x{K}: {ms:8.3f} ms  {2.0 * M * Nn * K / ms / 1e9:7.1f} TF/s", flush=True)
        del A, Bm, C


def gemm_bits(T=4096 * 300, E=256, Fh=2048):
    """The FFN pair with the 1-bit mask: linear1 + ReLU forward (writes hid + mask) and the masked dH backward."""
    x = torch.randn(T, E, device=dev)
    w1 = torch.randn(Fh, E, device=dev) / 16
    b1 = torch.randn(Fh, device=dev) / 10
    hid = torch.empty(T, Fh, device=dev)
    bits = ops.alloc_relu_bits(T, Fh, dev)
    ms = timeit(lambda: ops.gemm_bits(0, 1, T, Fh, E, x, E, w1, E, hid, Fh, bias=b1, flags=N.GEMM_RELU, bits_out=bits))
    print(f"gemm_bits ffn1 fwd NT  {T}x{Fh}x{E}: {ms:8.3f} ms  {2.0 * T * Fh * E / ms / 1e9:7.1f} TF/s", flush=True)
    dy = torch.randn(T, E, device=dev)
    w2 = torch.randn(E, Fh, device=dev) / 16
    ms = timeit(lambda: ops.gemm_bits(0, 0, T, Fh, E, dy, E, w2, Fh, hid, Fh, bits_in=bits))
    print(f"gemm_bits dhid bwd NN  {T}x{Fh}x{E}: {ms:8.3f} ms  {2.0 * T * Fh * E / ms / 1e9:7.1f} TF/s", flush=True)
    ms = timeit(lambda: ops.gemm(0, 1, T, Fh, E, x, E, w1, E, hid, Fh, bias=b1, flags=N.GEMM_RELU))
    print(f"gemm      ffn1 relu NT {T}x{Fh}x{E}: {ms:8.3f} ms  {2.0 * T * Fh * E / ms / 1e9:7.1f} TF/s", flush=True)
    ms = timeit(lambda: ops.gemm(0, 1, T, Fh, E, x, E, w1, E, hid, Fh))
    print(f"gemm      ffn1 plain NT {T}x{Fh}x{E}: {ms:8.3f} ms  {2.0 * T * Fh * E / ms / 1e9:7.1f} TF/s", flush=True)


def loss(S=300):
    """HBM-bound scan kernels: the fused reward-loss + cut-metrics pass (rlt_loss_metrics) against the separate kernels
    it replaces; algorithmic bytes per list = read p, labels 8S + write dL/dp 4S + 24 B of results.
    HIP-event times include the host's launch gaps at small batches: read the kernel durations from
    `rocprofv3 --kernel-trace --stats -- python tools/bench_kernels.py loss`."""
    for B in (4096, 65536, 262144):
        g = torch.Generator(device=dev).manual_seed(B)
        p = torch.softmax(torch.randn(B, S, device=dev, generator=g), 1).contiguous()
        y = (torch.rand(B, S, device=dev, generator=g) < 0.1).float()
        per_list, loss_out, dp = torch.empty(B, device=dev), torch.empty(1, device=dev), torch.empty(B, S, device=dev)
        k = torch.empty(B, dtype=torch.int32, device=dev)
        f1, dcg = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        wsb = N.query("rlt_loss_metrics_workspace", B)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=dev)
        nbytes = B * (12.0 * S + 24)

        def fused():
            call("rlt_loss_metrics", ptr(p), ptr(y), None, B, S, N.METRIC_F1, -1.0, N.LOSS_JS, 0.85, -1.0, ptr(per_list), ptr(loss_out),
                 ptr(dp), ptr(k), ptr(f1), ptr(dcg), ptr(sums), ptr(ops.dcg_table(dev)), ptr(ws), wsb, stream())

        def separate():
            call("rlt_reward_loss", ptr(p), ptr(y), None, B, S, N.METRIC_F1, N.LOSS_JS, 0.85, ptr(per_list), ptr(loss_out), ptr(dp), stream())
            call("rlt_cut_metrics", ptr(p), ptr(y), None, B, S, ptr(k), ptr(f1), ptr(dcg), ptr(sums), stream())
        ms = timeit(fused, reps=50, warm=5)
        print(f"loss+metrics fused (2 launches) B{B} S{S}: {ms * 1e3:9.1f} us  {nbytes / ms / 1e6:8.1f} GB/s algorithmic = {nbytes / ms / 1e6 / 8000:.3f} of 8 TB/s", flush=True)
        ms = timeit(separate, reps=50, warm=5)
        print(f"loss, then metrics (4 launches) B{B} S{S}: {ms * 1e3:9.1f} us  {(nbytes + B * 8.0 * S) / ms / 1e6:8.1f} GB/s of its own bytes (p, labels read twice)", flush=True)


def baselines(B=1048576, S=300):
    """rlt_truncation_curves (the Oracle / Fixed-k / Greedy-k curves): 1,048,576 lists x 300 labels, robust04-shaped labels.
    Algorithmic bytes: the labels, 4 S per list (the per-workgroup records and the curves are < 1 % of it).  Per-list outputs
    off, as the streaming accumulator (utils/baselines.py) runs it."""
    g = torch.Generator(device=dev).manual_seed(7)
    prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32, device=dev) / 45.0) + 0.02
    y = (torch.rand(B, S, device=dev, generator=g) < prob).float()
    curves = torch.zeros(3, S + 1, dtype=torch.float64, device=dev)
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    wsb = N.query("rlt_truncation_curves_workspace", B, S)
    ws = torch.empty(wsb // 8 + 2, dtype=torch.float64, device=dev)
    tab = ops.dcg_table(dev)
    nbytes = 4.0 * B * S

    def run():
        call("rlt_truncation_curves", ptr(y), B, S, -1.0, ptr(tab), 0, ptr(curves), None, None, None, None, ptr(sums), ptr(ws), wsb, stream())
    ms = timeit(run, reps=20, warm=3)
    print(f"truncation curves B{B} S{S}: {ms * 1e3:9.1f} us  {nbytes / ms / 1e6:8.1f} GB/s algorithmic = {nbytes / ms / 1e6 / 8000:.3f} of 8 TB/s "
          f"(records {wsb / 1e6:.1f} MB)", flush=True)


def report(B=1048576, S=300, reps=9):
    """rlt_cut_report (the fused per-query report + the --draw curves) against the composition it replaces on the same data:
    rlt_cut_metrics_ex + rlt_truncation_curves + rlt_reward_matrix_ex (r written) + torch softmax / sum over r / tau and over
    p / sharpen in float64.  1,048,576 lists x 300 positions, the shape of the `baselines` bench.  HIP events around single
    alternating launches, the median of `reps`; GB/s on the fused pass's algorithmic bytes, 8 S per list (p and the labels
    read once), for both."""
    g = torch.Generator(device=dev).manual_seed(7)
    prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32, device=dev) / 45.0) + 0.02
    y = (torch.rand(B, S, device=dev, generator=g) < prob).float()
    p = torch.softmax(torch.randn(B, S, device=dev, generator=g), 1).contiguous()
    tab, coef = ops.dcg_table(dev), ops.dcg_coef(S, dev)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    k, pk, mg, f1, dcg, bf, bfk, bd, bdk, better = i32(B), torch.zeros(B, device=dev), torch.zeros(B, device=dev), f64(B), f64(B), \
        f64(B), i32(B), f64(B), i32(B), i32(B)
    hist, pc, rc, sums = f64(S + 1), f64(S), f64(S), f64(5)
    wsb = N.query("rlt_cut_report_workspace", B, S)
    ws = N.workspace(wsb, dev)
    tau, sharpen = 0.9, 0.9e-3

    def fused():
        call("rlt_cut_report", ptr(p), N.CUT_ARGMAX, ptr(y), ptr(coef), B, S, N.METRIC_DCG, -1.0, -1.0, tau, sharpen, ptr(tab), 0,
             ptr(k), ptr(pk), ptr(mg), ptr(f1), ptr(dcg), ptr(bf), ptr(bfk), ptr(bd), ptr(bdk), ptr(better), ptr(hist), ptr(pc), ptr(rc),
             ptr(sums), ptr(ws), wsb, stream())
    curves, csums, s2 = f64(3, S + 1), f64(3), f64(2)
    cwsb = N.query("rlt_truncation_curves_workspace", B, S)
    cws = N.workspace(cwsb, dev)
    r = torch.empty(B, S, device=dev)

    def composed():
        call("rlt_cut_metrics_ex", ptr(p), ptr(y), None, B, S, -1.0, ptr(k), ptr(f1), ptr(dcg), ptr(s2), stream())
        call("rlt_truncation_curves", ptr(y), B, S, -1.0, ptr(tab), 0, ptr(curves), ptr(bf), ptr(bfk), ptr(bd), ptr(bdk), ptr(csums),
             ptr(cws), cwsb, stream())
        call("rlt_reward_matrix_ex", ptr(y), ptr(coef), B, S, N.METRIC_DCG, -1.0, tau, ptr(r), None, stream())
        rk = r.gather(1, (k.long() - 1).unsqueeze(1))
        (r > rk).sum(1)
        torch.softmax(r.double() / tau, 1).sum(0)
        torch.softmax(p.double() / sharpen, 1).sum(0)
        torch.bincount(k, minlength=S + 1)
    times = {"fused": [], "composed": []}
    for fn in (fused, composed):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in (("fused", fused), ("composed", composed)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    nbytes = 8.0 * B * S
    mf, mc = (sorted(times[n])[reps // 2] for n in ("fused", "composed"))
    print(f"cut report fused    B{B} S{S}: {mf * 1e3:9.1f} us  {nbytes / mf / 1e6:8.1f} GB/s algorithmic = {nbytes / mf / 1e6 / 8000:.3f} of 8 TB/s", flush=True)
    print(f"cut report composed B{B} S{S}: {mc * 1e3:9.1f} us  {nbytes / mc / 1e6:8.1f} GB/s on the same bytes", flush=True)
    print(f"cut report composed / fused: {mc / mf:.2f}x", flush=True)


def sweep(B=1048576, S=300, T=19, reps=9):
    """rlt_cut_sweep (T threshold cuts and their eight curve rows from one read of p and the labels) against two compositions of
    what exists without it, on the same data, QUANTILE rule: (a) one float64 cumsum of p, one batched searchsorted for the T
    targets and T launches of rlt_cut_metrics_ex at k[:, t] - k, F1 and DCG only, precision / recall / F_beta are not available
    that way; (b) torch alone: the cumsum and searchsorted, float64 cumsums of the relevant count and of the DCG terms, a gather
    at k and the eight rows as tensor arithmetic.  1,048,576 lists x 300 positions, T = 19 thresholds 0.05..0.95.  HIP events
    around single alternating launches, the median of `reps`; GB/s on the fused pass's algorithmic bytes, 8 S per list."""
    g = torch.Generator(device=dev).manual_seed(7)
    prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32, device=dev) / 45.0) + 0.02
    y = (torch.rand(B, S, device=dev, generator=g) < prob).float()
    p = torch.softmax(torch.randn(B, S, device=dev, generator=g), 1).contiguous()
    taus = torch.linspace(0.05, 0.95, T, dtype=torch.float64, device=dev)
    tab = ops.dcg_table(dev)
    k = torch.zeros(B, T, dtype=torch.int32, device=dev)
    curve = torch.zeros(N.SWEEP_COLS, T, dtype=torch.float64, device=dev)
    wsb = N.query("rlt_cut_sweep_workspace", B, S, T)
    ws = N.workspace(wsb, dev)

    def fused():
        call("rlt_cut_sweep", ptr(p), 1, N.SWEEP_QUANTILE, ptr(taus), T, ptr(y), B, S, -1.0, 1.0, ptr(tab), 0, ptr(k), ptr(curve),
             ptr(ws), wsb, stream())
    kb, f1, dcg, s2 = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.float64, device=dev), \
        torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    out_a = torch.zeros(3, T, dtype=torch.float64, device=dev)

    def cuts():
        C = torch.cumsum(p, 1, dtype=torch.float64)
        target = taus[None, :] * C[:, -1:]
        return (1 + torch.searchsorted(C[:, :-1].contiguous(), target)).to(torch.int32)

    def composed_metrics():
        kk = cuts().t().contiguous()
        for t in range(T):
            call("rlt_cut_metrics_ex", None, ptr(y), ptr(kk[t]), B, S, -1.0, ptr(kb), ptr(f1), ptr(dcg), ptr(s2), stream())
            out_a[1:, t] = s2
        out_a[0] = kk.sum(1, dtype=torch.float64)
    coef = tab[:S]

    def composed_torch():
        kk = cuts().long()
        rel = y == 1.0
        cnt = torch.cumsum(rel, 1, dtype=torch.float64)
        dpre = torch.cumsum(torch.where(rel, coef, -coef), 1)
        hits, d = cnt.gather(1, kk - 1), dpre.gather(1, kk - 1)
        n = cnt[:, -1:]
        prec, rec = hits / kk, torch.where(n != 0, hits / n, torch.zeros_like(hits))
        den = prec + rec
        f = torch.where(den != 0, 2.0 * prec * rec / den, torch.zeros_like(den))
        return torch.stack([kk.sum(0, dtype=torch.float64), f.sum(0), d.sum(0), prec.sum(0), rec.sum(0), f.sum(0),
                            (kk == S).sum(0, dtype=torch.float64), torch.full((T,), float(B), dtype=torch.float64, device=dev)])
    fns = (("fused", fused), ("cumsum + searchsorted + T x rlt_cut_metrics_ex", composed_metrics), ("torch alone", composed_torch))
    for _name, fn in fns:
        fn()
    torch.cuda.synchronize()
    # the three agree before anything is timed
    ref = composed_torch()
    # (a pair whose target sits within rounding of a prefix may be cut one position apart by another summation order)
    assert (curve[0] - ref[0]).abs().max() <= 4 and (curve[0] - out_a[0]).abs().max() <= 4 and (curve[6] - ref[6]).abs().max() <= 4
    for row in (1, 2, 3, 4):
        assert torch.allclose(curve[row], ref[row], rtol=1e-11, atol=0), row
    assert torch.allclose(curve[1:3], out_a[1:], rtol=1e-11, atol=0)
    times = {name: [] for name, _fn in fns}
    for _ in range(reps):
        for name, fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    nbytes = 8.0 * B * S
    med = {name: sorted(v)[reps // 2] for name, v in times.items()}
    for name, v in times.items():
        print(f"cut sweep B{B} S{S} T{T} {name:48s}: {med[name] * 1e3:10.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, {reps} calls)  "
              f"{nbytes / med[name] / 1e6:8.1f} GB/s on 8 S bytes per list", flush=True)
    best = min((n for n in med if n != "fused"), key=med.get)
    print(f"cut sweep best composition: {best}; composition / fused: {med[best] / med['fused']:.2f}x"
          + ("  (the fused pass is SLOWER than the composition here)" if med["fused"] > med[best] else ""), flush=True)


def probe(B=4096, S=300, E=256):
    """rlt_probe_heads (the probing study's fused probe pass) against the composed path on the same data: one BCE and one
    rerank head on frozen position-major features x (S*B, E) = 1.26 GB.  Fused: x read once, no dx.  Composed: rlt_heads_fwd
    (x read) + rlt_mt_terms + rlt_mt_terms_bwd + rlt_heads_bwd (x read again, a dx nobody uses written): >= 3 x 4 S B E bytes.
    GB/s counts each path's algorithmic bytes; the fraction is of 8 TB/s."""
    T = S * B
    x = torch.randn(T, E, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32, device=dev) / 45.0) + 0.02
    y = (torch.rand(B, S, device=dev, generator=g) < prob).float()
    w = torch.randn(2, E, device=dev) / E ** 0.5
    b = torch.zeros(2, device=dev)
    loss, dw, db, out = torch.empty(2, device=dev), torch.empty(2, E, device=dev), torch.empty(2, device=dev), torch.empty(2, B, S, device=dev)
    karr = (N.c_int * 2)(N.PROBE_BCE, N.PROBE_RERANK)
    wsb = N.query("rlt_probe_heads_workspace", 2, S, B, E)
    ws = N.workspace(wsb, dev)

    def fused():
        call("rlt_probe_heads", ptr(x), ptr(w), ptr(b), karr, 2, S, B, E, ptr(y), 5e-4, ptr(loss), ptr(dw), ptr(db), ptr(out),
             ptr(ws), wsb, stream())
    hk = (N.c_int * 2)(N.HEAD_SIGMOID, N.HEAD_SOFTMAX)
    terms = torch.empty(4, device=dev)
    tws_b = N.query("rlt_mt_terms_workspace", B, S)
    tws = N.workspace(tws_b, dev)
    dout = torch.empty(2, B, S, device=dev)
    dx = torch.empty(T, E, device=dev)
    hws_b = N.query("rlt_heads_bwd_workspace", 2, S, B, E)
    hws = N.workspace(hws_b, dev)
    dw2, db2 = torch.empty(2, E, device=dev), torch.empty(2, device=dev)

    def composed():
        call("rlt_heads_fwd", ptr(x), ptr(w), ptr(b), hk, 2, S, B, E, ptr(out), stream())
        call("rlt_mt_terms", ptr(out[1]), ptr(out[0]), ptr(y), B, S, 5e-4, ptr(terms), ptr(tws), tws_b, stream())
        call("rlt_mt_terms_bwd", ptr(out[0]), ptr(y), ptr(terms), B, S, 1.0, 1.0, None, ptr(dout[1]), ptr(dout[0]), stream())
        call("rlt_heads_bwd", ptr(x), ptr(w), hk, 2, ptr(out), ptr(dout), S, B, E, ptr(dx), 0, ptr(dw2), ptr(db2), ptr(hws),
             hws_b, stream())
    xb = 4.0 * T * E
    fb = xb + 4.0 * B * S * 3 + wsb
    cb = 3 * xb + 4.0 * B * S * 12
    mf = timeit(fused, reps=10, warm=2)
    mc = timeit(composed, reps=10, warm=2)
    print(f"probe fused    B{B} S{S} E{E} 2 heads: {mf * 1e3:9.1f} us  {fb / mf / 1e6:8.1f} GB/s = {fb / mf / 1e6 / 8000:.3f} of 8 TB/s", flush=True)
    print(f"probe composed B{B} S{S} E{E} 2 heads: {mc * 1e3:9.1f} us  {cb / mc / 1e6:8.1f} GB/s = {cb / mc / 1e6 / 8000:.3f} of 8 TB/s", flush=True)
    print(f"probe fused / composed speed-up: {mc / mf:.2f}x", flush=True)


def lstm(B=4096, S=300):
    T = S * B
    gates = torch.randn(T, 1024, device=dev) * 0.5
    w = torch.randn(2, 512, 128, device=dev) / 12
    h = torch.empty(T, 256, device=dev)
    c = torch.empty(T, 256, device=dev)
    dh = torch.randn(T, 256, device=dev)
    fl = 2.0 * 512 * 128 * T * 2 / 1e9
    ms = timeit(lambda: call("rlt_bilstm_rec_fwd", ptr(gates), ptr(w[0]), ptr(w[1]), S, B, ptr(h), ptr(c), N.PRECISION_DEFAULT, stream()), reps=2)
    print(f"bilstm_fwd B{B} S{S}: {ms:8.3f} ms  {fl / ms:7.1f} TF/s", flush=True)
    ms = timeit(lambda: call("rlt_bilstm_rec_bwd", ptr(gates), ptr(c), ptr(w[0]), ptr(w[1]), ptr(dh), S, B, N.PRECISION_DEFAULT, stream()), reps=2)
    print(f"bilstm_bwd B{B} S{S}: {ms:8.3f} ms  {fl / ms:7.1f} TF/s", flush=True)


def lstm_x(B=4096, S=300):
    """Layer 0: the recurrence with the fused input projection (I = 3)."""
    T = S * B
    x = torch.randn(T, 3, device=dev)
    gates = torch.empty(T, 1024, device=dev)
    w = torch.randn(2, 512, 128, device=dev) / 12
    wi = torch.randn(2, 512, 3, device=dev) / 2
    bi = torch.randn(2, 512, device=dev) / 4
    bh = torch.randn(2, 512, device=dev) / 4
    h = torch.empty(T, 256, device=dev)
    c = torch.empty(T, 256, device=dev)
    ms = timeit(lambda: call("rlt_bilstm_rec_fwd_x", ptr(x), 3, ptr(wi[0]), ptr(bi[0]), ptr(bh[0]), ptr(wi[1]), ptr(bi[1]), ptr(bh[1]),
                             ptr(w[0]), ptr(w[1]), S, B, ptr(gates), ptr(h), ptr(c), N.PRECISION_DEFAULT, stream()), reps=2)
    print(f"bilstm_fwd_x B{B} S{S}: {ms:8.3f} ms", flush=True)


def lstm_w():
    """Forward recurrences (layer 1 form and layer 0 with the fused input projection) over batch sizes."""
    for B in (32, 63, 512, 4096):
        S = 300
        T = S * B
        gates = torch.randn(T, 1024, device=dev) * 0.5
        w = torch.randn(2, 512, 128, device=dev) / 12
        h = torch.empty(T, 256, device=dev)
        c = torch.empty(T, 256, device=dev)
        ms = timeit(lambda: call("rlt_bilstm_rec_fwd", ptr(gates), ptr(w[0]), ptr(w[1]), S, B, ptr(h), ptr(c), N.PRECISION_DEFAULT, stream()), reps=3)
        print(f"bilstm_fwd   B{B} S{S}: {ms:8.3f} ms  {ms / S * 1e3:6.2f} us / step", flush=True)
        lstm_x(B, S)
        dh = torch.randn(T, 256, device=dev)
        ms = timeit(lambda: call("rlt_bilstm_rec_bwd", ptr(gates), ptr(c), ptr(w[0]), ptr(w[1]), ptr(dh), S, B, N.PRECISION_DEFAULT, stream()), reps=3)
        print(f"bilstm_bwd   B{B} S{S}: {ms:8.3f} ms  {ms / S * 1e3:6.2f} us / step", flush=True)


def lstm_small():
    for B in (32, 64, 256):
        lstm(B=B)


def overlap(B=4096, S=300):
    """Does a latency/HBM-bound persistent kernel (BiLSTM backward recurrence, 256 workgroups) share the chip with an
    MFMA-bound weight-gradient product (TN, M=2048 N=256 K=T, 256 workgroups) issued on a second stream?"""
    T = S * B
    gates = torch.randn(T, 1024, device=dev) * 0.5
    w = torch.randn(2, 512, 128, device=dev) / 12
    h = torch.empty(T, 256, device=dev)
    c = torch.empty(T, 256, device=dev)
    dh = torch.randn(T, 256, device=dev)
    call("rlt_bilstm_rec_fwd", ptr(gates), ptr(w[0]), ptr(w[1]), S, B, ptr(h), ptr(c), N.PRECISION_DEFAULT, stream())
    hid = torch.randn(T, 2048, device=dev)
    dy = torch.randn(T, 256, device=dev)
    dw = torch.empty(2048, 256, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def rec():
        call("rlt_bilstm_rec_bwd", ptr(gates), ptr(c), ptr(w[0]), ptr(w[1]), ptr(dh), S, B, N.PRECISION_DEFAULT, stream())

    def gemm_tn():
        ops.gemm(1, 0, 2048, 256, T, hid, 2048, dy, 256, dw, 256)

    def both():
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(s1):
            s1.wait_event(ev)
            rec()
            e1 = torch.cuda.Event(); e1.record()
        with torch.cuda.stream(s2):
            s2.wait_event(ev)
            gemm_tn()
            gemm_tn()
            e2 = torch.cuda.Event(); e2.record()
        torch.cuda.current_stream().wait_event(e1)
        torch.cuda.current_stream().wait_event(e2)

    print(f"bilstm_bwd alone      : {timeit(rec, reps=3):8.3f} ms", flush=True)
    print(f"2 x dW (TN) alone     : {timeit(lambda: (gemm_tn(), gemm_tn()), reps=3):8.3f} ms", flush=True)
    print(f"both, two streams     : {timeit(both, reps=3):8.3f} ms", flush=True)


def stamps():
    """Timeline of one dK+dV workgroup (library built with -DRLT_STAMPS): per wavefront and tile, cycles spent computing
    (tile start -> before the barrier) and the start offsets relative to wavefront 0."""
    import ctypes
    attention()
    buf = (ctypes.c_ulonglong * 256)()
    fn = N.load().rlt_debug_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    rc = fn(buf, 256)
    assert rc == 0, rc
    v = list(buf)
    t00 = v[0]
    print("wave: per tile (start - wave0 tile0 start, compute cycles)")
    for w in range(8):
        row = []
        for t in range(2, 10):
            a, b = v[(w * 16 + t) * 2], v[(w * 16 + t) * 2 + 1]
            row.append(f"{a - t00:7d}+{b - a:5d}")
        print(f"  w{w}: " + "  ".join(row))


def gemm_stamps(T=4096 * 300):
    """Timeline of one gemm3b workgroup (library built with -DRLT_STAMPS): prologue / K loop / epilogue cycles per wavefront."""
    import ctypes
    fn = N.load().rlt_debug_gemm_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    for name, ta, tb, M, Nn, K in [("ffn1 fwd NT", 0, 1, T, 2048, 256), ("ffn2 fwd NT", 0, 1, T, 256, 2048), ("ffn2 dX NN", 0, 0, T, 2048, 256)]:
        A = torch.randn((K, M) if ta else (M, K), device=dev)
        Bm = torch.randn((Nn, K) if tb else (K, Nn), device=dev)
        C = torch.empty(M, Nn, device=dev)
        ms = timeit(lambda: ops.gemm(ta, tb, M, Nn, K, A, A.shape[1], Bm, Bm.shape[1], C, Nn))
        buf = (ctypes.c_ulonglong * 32)()
        assert fn(buf, 32) == 0
        v = list(buf)
        print(f"gemm {name} {M}x{Nn}x{K}: {ms:.3f} ms; per wavefront (prologue, K loop, epilogue) cycles:")
        for w in range(8):
            s0, s1, s2, s3 = v[4 * w:4 * w + 4]
            print(f"   w{w}: {s1 - s0:6d} {s2 - s1:7d} {s3 - s2:6d}")
        del A, Bm, C


def g6c_stamps(T=4096 * 300):
    """Slot timeline of one gemm6c workgroup (bf16x6 mode, library built with -DRLT_STAMPS): per wavefront and slot the cycles
    from slot start to its last MFMA issue, and the wait at the barrier behind it; even slots only multiply, odd slots also
    split the next register tile."""
    import ctypes
    fn = N.load().rlt_debug_g6c_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    N.set_precision("bf16x6")
    for name, ta, tb, M, Nn, K in [("ffn1 fwd NT", 0, 1, T, 2048, 256), ("ffn2 fwd NT", 0, 1, T, 256, 2048), ("ffn1 dW TN", 1, 0, 2048, 256, T)]:
        A = torch.randn((K, M) if ta else (M, K), device=dev)
        Bm = torch.randn((Nn, K) if tb else (K, Nn), device=dev)
        C = torch.empty(M, Nn, device=dev)
        ms = timeit(lambda: ops.gemm(ta, tb, M, Nn, K, A, A.shape[1], Bm, Bm.shape[1], C, Nn))
        buf = (ctypes.c_ulonglong * (8 * 40 * 3))()
        assert fn(buf, 8 * 40 * 3) == 0
        v = list(buf)
        print(f"gemm6c {name} {M}x{Nn}x{K}: {ms:.3f} ms; slots 2..33 of one workgroup: cycles [start->last MFMA issued | barrier wait], slot period")
        for w in range(8):
            row = []
            for sl in range(2, 34):
                t0, t1, t2 = v[(w * 40 + sl) * 3:(w * 40 + sl) * 3 + 3]
                nxt = v[(w * 40 + sl + 1) * 3]
                row.append(f"{t1 - t0:5d}|{t2 - t1:4d}|{nxt - t0:5d}")
            print(f"   w{w}: " + " ".join(row))
        ev = [v[(0 * 40 + sl + 1) * 3] - v[(0 * 40 + sl) * 3] for sl in range(2, 34, 2)]
        od = [v[(0 * 40 + sl + 1) * 3] - v[(0 * 40 + sl) * 3] for sl in range(3, 35, 2)]
        print(f"   wave 0 mean slot period: even {sum(ev) / len(ev):.0f}, odd {sum(od) / len(od):.0f} cycles (48 MFMAs per wavefront and slot = 3,072 matrix cycles per SIMD)")
        del A, Bm, C


def dkv1_stamps(B=4096, S=60, H=4, HD=64, which="dkv"):
    """Phase timeline of the one-wavefront-per-SIMD dK+dV kernel: needs a -DRLT_DKV1_STAMPS library (RLT_HIP_LIB)."""
    import ctypes
    E = H * HD
    T = S * B
    qkv = torch.randn(T, 3 * E, device=dev); out = torch.randn(T, E, device=dev); lse = torch.randn(S, H, B, device=dev).abs() + 20
    dout = torch.randn(T, E, device=dev); dqkv = torch.empty_like(qkv)
    ib = N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, 0.0, N.PRECISION_DEFAULT)
    images = torch.empty(max(ib, 16) // 4, device=dev) if ib else None
    wb = N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, 0.0, N.PRECISION_DEFAULT)
    ws = torch.empty(wb // 4 + 4, device=dev)
    call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, ptr(images), ptr(ws), wb, N.PRECISION_DEFAULT, stream())
    f = lambda: call("rlt_list_attention_bwd_" + which, ptr(qkv), ptr(dout), ptr(lse), ptr(images), ptr(ws), wb, S, B, H, HD, 0.0, 7, ptr(dqkv), N.PRECISION_DEFAULT, stream())
    ms = timeit(f)
    fn = N.load().rlt_debug_dkv1_stamps
    fn.restype = ctypes.c_int
    buf = (ctypes.c_ulonglong * (4 * 4 * 66))()
    assert fn(buf) == 0
    v = list(buf)
    nstep = 64 if which == "dkv" else 48
    print(f"{which}1 {ms:.3f} ms; cycles per step (six MFMAs = 192 matrix cycles) of tiles 9, 10 of wavefronts 0 and 3, then barrier wait and tile period")
    for w in (0, 3):
        for tl in (1, 2):
            st = v[(w * 4 + tl) * 66:(w * 4 + tl) * 66 + 66]
            nx = v[(w * 4 + tl + 1) * 66]
            d = [st[k + 1] - st[k] for k in range(nstep - 1)] + [st[64] - st[nstep - 1]]
            print(f"  w{w} t{8 + tl}: " + " ".join(f"{x:4d}" for x in d) + f" | {st[65] - st[64]:5d} | {nx - st[0]:6d}")


def a6n_stamps(which="dkv", B=8192, S=20, H=8, HD=16):
    """Slot timeline of the pipelined head-dim-16 backward kernels: needs a -DRLT_A6N_STAMPS library (RLT_HIP_LIB)."""
    import ctypes
    E = H * HD
    T = S * B
    qkv = torch.randn(T, 3 * E, device=dev); out = torch.randn(T, E, device=dev); lse = torch.randn(S, H, B, device=dev).abs() + 20
    dout = torch.randn(T, E, device=dev); dqkv = torch.empty_like(qkv)
    wb = N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, 0.0, N.PRECISION_DEFAULT)
    ws = torch.empty(wb // 4 + 4, device=dev)
    call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, None, ptr(ws), wb, N.PRECISION_DEFAULT, stream())
    f = lambda: call("rlt_list_attention_bwd_" + which, ptr(qkv), ptr(dout), ptr(lse), None, ptr(ws), wb, S, B, H, HD, 0.0, 7, ptr(dqkv), N.PRECISION_DEFAULT, stream())
    ms = timeit(f)
    fn = N.load().rlt_debug_a6n_stamps
    fn.restype = ctypes.c_int
    buf = (ctypes.c_ulonglong * (4 * 4 * 18))()
    assert fn(buf) == 0
    v = list(buf)
    gs = 32 if which == "dkv" else 22
    print(f"{which} {ms:.3f} ms; cycles per slot ({gs} MFMAs = {16 * gs} matrix cycles) of tiles 9, 10 of wavefronts 0 and 3, then barrier wait and tile period")
    for w in (0, 3):
        for tl in (1, 2):
            st = v[(w * 4 + tl) * 18:(w * 4 + tl) * 18 + 18]
            nx = v[(w * 4 + tl + 1) * 18]
            d = [st[k + 1] - st[k] for k in range(16)]
            print(f"  w{w} t{8 + tl}: " + " ".join(f"{x:4d}" for x in d) + f" | {st[17] - st[16]:5d} | {nx - st[0]:6d}")


def a6h_stamps(which="fwd", B=4096, S=60, H=4, HD=64):
    """Slot timeline of the pipelined head-dim-64 kernels: needs a -DRLT_A6H_STAMPS library (RLT_HIP_LIB)."""
    import ctypes
    E = H * HD
    T = S * B
    qkv = torch.randn(T, 3 * E, device=dev); out = torch.randn(T, E, device=dev); lse = torch.randn(S, H, B, device=dev).abs() + 20
    dout = torch.randn(T, E, device=dev); dqkv = torch.empty_like(qkv)
    ib = N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, 0.0, N.PRECISION_DEFAULT)
    images = torch.empty(max(ib, 16) // 4, device=dev) if ib else None
    wb = N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, 0.0, N.PRECISION_DEFAULT)
    ws = torch.empty(wb // 4 + 4, device=dev)
    if which == "fwd":
        f = lambda: call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, 0.0, 7, ptr(out), ptr(lse), ptr(images), ib, N.PRECISION_DEFAULT, stream())
    else:
        call("rlt_list_attention_bwd_prepare", ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, ptr(images), ptr(ws), wb, N.PRECISION_DEFAULT, stream())
        f = lambda: call("rlt_list_attention_bwd_" + which, ptr(qkv), ptr(dout), ptr(lse), ptr(images), ptr(ws), wb, S, B, H, HD, 0.0, 7, ptr(dqkv), N.PRECISION_DEFAULT, stream())
    ms = timeit(f)
    fn = N.load().rlt_debug_a6h_stamps
    fn.restype = ctypes.c_int
    buf = (ctypes.c_ulonglong * (4 * 4 * 18))()
    assert fn(buf) == 0
    v = list(buf)
    gs, ns = {"fwd": (52, 8), "dq": (76, 4), "dkv": (104, 4)}[which]
    print(f"{which} {ms:.3f} ms; cycles per slot ({gs} MFMAs = {16 * gs} matrix cycles) of tiles 9, 10 of wavefronts 0 and 3, then the last slot up to the barrier, the barrier wait and the tile period")
    for w in (0, 3):
        for tl in (1, 2):
            st = v[(w * 4 + tl) * 18:(w * 4 + tl) * 18 + 18]
            nx = v[(w * 4 + tl + 1) * 18]
            d = [st[k + 1] - st[k] for k in range(ns - 1)] + [st[16] - st[ns - 1]]
            print(f"  w{w} t{8 + tl}: " + " ".join(f"{x:4d}" for x in d) + f" | {st[17] - st[16]:5d} | {nx - st[0]:6d}")


def a6h_stamps_dq():
    a6h_stamps(which="dq")


def a6h_stamps_dkv():
    a6h_stamps(which="dkv")


def a6n_stamps_dq():
    a6n_stamps(which="dq")


def dq1_stamps():
    dkv1_stamps(which="dq")


def features(B=4096, S=300, n_docs=131072, D=200, n_terms=231448, rounds=25):
    """rlt_neighbor_features (AttnCut's neighbour-similarity statistics, both columns written into the packed model input) over
    4096 lists x 300 from a table of 131,072 documents: doc2vec rows of 200 float32, tf-idf rows drawn from the robust-like
    profile of tools/make_feature_golden.py.  Beside it, alternating in the same process, a torch composition of the doc2vec
    column ALONE (index_select of the rows, product, sum, norms, divide): what the library offered before this kernel.
    HIP-event time per launch, median over `rounds` launches of each after warm-up.  Algorithmic bytes per position: 4 (id)
    + 4 D (dense row) + 12 nnz (sparse row) + 8 (two outputs)."""
    import types
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from make_feature_golden import robust_like_table
    rs = np.random.RandomState(20261016)
    indptr, indices, values = robust_like_table(rs, n_docs, n_terms)
    d2v_h = (rs.standard_normal((n_docs, D)) * 0.3).astype(np.float32)
    ids_h = rs.randint(0, n_docs, (B, S)).astype(np.int32)
    table = types.SimpleNamespace(n_docs=n_docs, indptr=torch.from_numpy(indptr).to(dev), indices=torch.from_numpy(indices).to(dev),
                                  values=torch.from_numpy(values).to(dev), d2v=torch.from_numpy(d2v_h).to(dev))
    ids = torch.from_numpy(ids_h).to(dev)
    X = torch.zeros(B, S, 3, device=dev)
    nnz = int(np.diff(indptr)[ids_h].sum())
    nbytes = float(B * S * (4 + 4 * D + 8) + 12 * nnz)

    def fused():
        ops.neighbor_features(ids, table, out=X, col=1, validate=False)

    flat = ids.reshape(-1).long()
    first = (torch.arange(B * S, device=dev) % S) == 0
    last = (torch.arange(B * S, device=dev) % S) == S - 1

    def composed():
        x = table.d2v.index_select(0, flat)                     # (B*S, D): the gathered copy
        nrm = torch.linalg.vector_norm(x, dim=1)
        num = (x[:-1] * x[1:]).sum(1)
        den = nrm[:-1] * nrm[1:]
        sim = torch.nan_to_num(torch.where(den != 0, num / den, torch.zeros_like(num)), nan=0.0)
        right = torch.cat([sim, sim[-1:]])                      # sim(i, i+1) at i
        left = torch.cat([sim[:1], sim])                        # sim(i-1, i) at i
        out = torch.where(first, right, (left + right) / 2)
        return torch.where(last, left, out).view(B, S)

    for _ in range(3):
        fused()
        ref = composed()
    torch.cuda.synchronize()
    diff = float((X[:, :, 2] - ref).abs().max())
    t = {"fused": [], "composed": []}
    for _ in range(rounds):
        for name, fn in (("fused", fused), ("composed", composed)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(b) * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"neighbor features B{B} S{S} D{D} docs{n_docs} mean nnz {nnz / (B * S):.1f}: fused two columns {med['fused']:9.1f} us "
          f"(min {min(t['fused']):.1f}, max {max(t['fused']):.1f}; {nbytes / med['fused'] / 1e3:8.1f} GB/s algorithmic = "
          f"{nbytes / med['fused'] / 1e3 / 8000:.3f} of 8 TB/s; {B / med['fused'] * 1e6:.3e} lists/s)", flush=True)
    print(f"    torch composition, doc2vec column alone      {med['composed']:9.1f} us (min {min(t['composed']):.1f}, max "
          f"{max(t['composed']):.1f}); ratio composed / fused = {med['composed'] / med['fused']:.2f}; max |fused - composed| on "
          f"that column {diff:.2e}; median over {rounds} alternating launches", flush=True)


def bicut_sparse(B=20, S=300, V=231448, n_docs=60000, draws=200, rounds=15):
    """BiCut's layer-0 input projection and its weight gradient on the sparse kernels (rlt_sparse_inproj_fwd / _bwd) at the
    reference loader's batch of 20 lists x 300 and the published dictionary of 231,448 terms, against the same two products on
    the dense path (rlt_gemm forward and dW, default precision) on the densified (6000, 231451) input, alternating in one process.
    The table's profile is ASSUMED (the reference publishes neither figure): 60,000 documents, `draws` term draws per document
    from a rank^-1 (Zipf) distribution over the dictionary, duplicates merged - about 150 distinct terms per document, the most
    frequent term in nearly every document -, counts 1..5.  HIP-event time per call, median over `rounds` after warm-up.  Bytes
    moved, by the header's count: forward 4 KB per nonzero of the batch + the (T, 1024) gates; backward 4 KB per nonzero + the
    4 KB x I gradient written once; rate against the 6.0 TB/s indexed-row HBM rate.  Then the whole BiCut step (forward,
    BiCutLoss, backward, FusedAdam over all parameters)."""
    import numpy as np
    from dataloader.bicut_data import BowTable
    from models import BiCut
    from rlt_hip.parallel import FlatModel, FusedAdam
    from utils import losses as hl
    rs = np.random.RandomState(20261016)
    p = 1.0 / np.arange(1, V + 1)
    p /= p.sum()
    key = np.unique(np.repeat(np.arange(n_docs, dtype=np.int64), draws) * V + rs.choice(V, size=n_docs * draws, p=p))
    rows, indices = key // V, (key % V).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_docs))]).astype(np.int64)
    table = BowTable.from_csr(indptr, indices, rs.randint(1, 6, size=indices.size).astype(np.float32), V).to(dev)
    ids_h = rs.randint(0, n_docs, (B, S)).astype(np.int32)
    nnz = int(np.diff(indptr)[ids_h].sum())
    T, I, Dn = S * B, 3 + V, 3
    dense = torch.from_numpy(rs.uniform(0, 4, (B, S, Dn)).astype(np.float32)).to(dev)
    batch = ops.SparseBatch(dense, torch.from_numpy(ids_h).to(dev), table)
    perm = torch.sort(batch.ids.t().reshape(-1), stable=True)[1].to(torch.int32)
    sb, _keep = batch.struct(perm)
    wt = [torch.randn(I, 512, device=dev) * 0.01 for _ in range(2)]
    dwt = [torch.empty(I, 512, device=dev) for _ in range(2)]
    bias = [torch.randn(512, device=dev) * 0.1 for _ in range(4)]
    db = [torch.empty(512, device=dev) for _ in range(4)]
    gates = torch.empty(T, 1024, device=dev)
    dg = torch.randn(T, 1024, device=dev)
    ws_b = N.query("rlt_sparse_inproj_workspace", S, B, Dn, table.n_docs, V, table.n_chunks)
    ws = N.byte_buffer(ws_b, dev)
    import ctypes
    fwd = lambda: call("rlt_sparse_inproj_fwd", ctypes.byref(sb), S, B, ptr(wt[0]), ptr(wt[1]), ptr(bias[0]), ptr(bias[1]), ptr(bias[2]),
                       ptr(bias[3]), ptr(gates), stream())
    bwd = lambda: call("rlt_sparse_inproj_bwd", ctypes.byref(sb), S, B, ptr(dg), ptr(dwt[0]), ptr(dwt[1]), ptr(db[0]), ptr(db[1]),
                       ptr(db[2]), ptr(db[3]), ptr(ws), ws_b, stream())
    # the dense path of the same two products: x (T, I) densified, both directions' weights packed (1024, I) as csrc/path.hip does
    x = batch.to_dense().transpose(0, 1).contiguous().view(T, I)          # position-major rows t = s*B + b
    wcat = torch.cat([w.t() for w in wt], 0).contiguous()
    dwcat = torch.empty(1024, I, device=dev)
    gates_d = torch.empty(T, 1024, device=dev)
    d_fwd = lambda: ops.gemm(0, 1, T, 1024, I, x, I, wcat, I, gates_d, 1024)
    d_bwd = lambda: ops.gemm(1, 0, 1024, I, T, dg, 1024, x, I, dwcat, I)
    t = {"fwd": [], "bwd": [], "dense_fwd": [], "dense_dw": []}
    fns = (("fwd", fwd), ("bwd", bwd), ("dense_fwd", d_fwd), ("dense_dw", d_bwd))
    for _ in range(2):
        for _n, fn in fns:
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(b) * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    by_f, by_b = 4096.0 * nnz + 4096.0 * T, 4096.0 * nnz + 4096.0 * I
    print(f"bicut_sparse B{B} S{S} V{V} docs{n_docs}: {nnz / T:.1f} terms per ranked document, {nnz} nonzeros in the batch, "
          f"{table.n_chunks - V} extra chunks over {table.n_multi} terms", flush=True)
    print(f"    (a) sparse projection forward  {med['fwd']:10.1f} us (min {min(t['fwd']):.1f}, max {max(t['fwd']):.1f}); "
          f"{by_f / 1e9:.2f} GB -> {by_f / med['fwd'] / 1e6:.2f} TB/s = {by_f / med['fwd'] / 1e6 / 6.0:.2f} of 6.0 TB/s", flush=True)
    print(f"    (b) sparse weight gradient     {med['bwd']:10.1f} us (min {min(t['bwd']):.1f}, max {max(t['bwd']):.1f}); "
          f"{by_b / 1e9:.2f} GB -> {by_b / med['bwd'] / 1e6:.2f} TB/s = {by_b / med['bwd'] / 1e6 / 6.0:.2f} of 6.0 TB/s", flush=True)
    print(f"    (c) dense rlt_gemm forward     {med['dense_fwd']:10.1f} us, dW {med['dense_dw']:10.1f} us "
          f"({2.0 * T * 1024 * I / med['dense_fwd'] / 1e6:.1f} / {2.0 * T * 1024 * I / med['dense_dw'] / 1e6:.1f} TFLOP/s); "
          f"(c) / ((a) + (b)) = {(med['dense_fwd'] + med['dense_dw']) / (med['fwd'] + med['bwd']):.1f}; median of {rounds} alternating calls",
          flush=True)
    # both paths against float64 products of torch on 64 token rows / 64 weight columns
    brow = torch.cat([bias[0] + bias[1], bias[2] + bias[3]])[None, :].double()
    ref_g = x[:64].double() @ wcat.double().t()
    cols = torch.cat([torch.arange(0, 35, device=dev), torch.randint(0, I, (29,), device=dev)])
    ref_w = dg.double().t() @ x[:, cols].double()
    got_w = torch.cat([w.t() for w in dwt], 0)[:, cols].double()
    print(f"    against float64 on 64 rows / 64 columns: gates sparse {float((gates[:64].double() - brow - ref_g).abs().max()):.2e}, dense "
          f"{float((gates_d[:64].double() - ref_g).abs().max()):.2e} (max |gate| {float(ref_g.abs().max()):.2f}); dW sparse "
          f"{float((got_w - ref_w).abs().max()):.2e}, dense {float((dwcat[:, cols].double() - ref_w).abs().max()):.2e} "
          f"(max |dW| {float(ref_w.abs().max()):.1f})", flush=True)
    del x, wcat, dwcat, gates_d
    # the whole step
    model = BiCut(input_size=I, dropout=0.0, sparse_input=True).to(dev)
    opt = FusedAdam(FlatModel(model), lr=3e-5, weight_decay=0.005)
    crit = hl.BiCutLoss(metric="nci")
    y = (torch.rand(B, S, device=dev) < 0.1).float()
    model.train()

    def step():
        opt.zero_grad()
        crit(model(batch), y).backward()
        opt.step()

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    print(f"    whole BiCut step (forward, BiCutLoss, backward, FusedAdam over {opt.flat.numel / 1e6:.1f} M parameters): "
          f"{float(np.median(ts)):10.1f} us (min {min(ts):.1f}, max {max(ts):.1f})", flush=True)


def optim(reps=15):
    """The optimizer step at AttnCut's 1,846,785 parameters (rounded up to its 4-float slots) and at BiCut's 237.6 M: (a)
    rlt_adam_step alone, (b) rlt_grad_norm + rlt_adam_step_guarded (and each of the two on its own), (c) the torch composition
    the guarded step replaces - vector_norm of the float64-cast bucket, isfinite().all(), mul_ by the clamped coefficient, then
    rlt_adam_step - with no host read either.  HIP events around single alternating launches, the median of `reps`; GB/s on each
    pass's algorithmic bytes (Adam 28 n: p, g, m, v read, p, m, v written; the norm 4 n)."""
    lr, b1, b2, eps, wd, max_norm = 3e-5, 0.9, 0.999, 1e-8, 0.005, 1e9
    for label, n in (("AttnCut", (1846785 + 3) // 4 * 4), ("BiCut", 237600000)):
        gen = torch.Generator(device=dev).manual_seed(3)
        p, g = torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device=dev)
        wsb = N.query("rlt_grad_norm_workspace", n, 0)
        ws = N.byte_buffer(wsb, dev)
        t = [0]

        def adam():
            t[0] += 1
            call("rlt_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), n, t[0], lr, b1, b2, eps, wd, stream())

        def norm():
            call("rlt_grad_norm", ptr(g), n, None, 0, max_norm, ptr(ws), wsb, None, ptr(state), stream())

        def guarded():
            call("rlt_adam_step_guarded", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(state), lr, b1, b2, eps, wd, 1, stream())

        def both():
            norm()
            guarded()

        def composed():
            nrm = torch.linalg.vector_norm(g.double())
            torch.isfinite(g).all()
            g.mul_((max_norm / (nrm + 1e-6)).clamp(max=1.0).float())
            adam()
        fns = (("adam_step", adam, 28), ("grad_norm", norm, 4), ("adam_step_guarded", guarded, 28), ("norm+guarded", both, 32),
               ("torch composition", composed, 32))
        times = {name: [] for name, _, _ in fns}
        for _, fn, _ in fns:
            fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, fn, _ in fns:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b))
        med = {name: sorted(ts)[reps // 2] for name, ts in times.items()}
        for name, _, per in fns:
            ms = med[name]
            print(f"optim {label:8s} n={n:10d} {name:18s}: {ms * 1e3:9.1f} us  {per * n / ms / 1e6:8.1f} GB/s on {per} n bytes", flush=True)
        print(f"optim {label:8s} norm+guarded / adam_step: {med['norm+guarded'] / med['adam_step']:.2f}x;  torch composition / norm+guarded: "
              f"{med['torch composition'] / med['norm+guarded']:.2f}x"
              + ("  (the guarded step is SLOWER than the torch composition here)" if med['norm+guarded'] > med['torch composition'] else ""),
              flush=True)
        del p, g, m, v
        torch.cuda.empty_cache()


def recipe(reps=9):
    """The recipe step (csrc/recipe.hip) at AttnCut's 1,846,785 parameters (padded as FlatModel pads its slots) and at BiCut's
    237.6 M.  (a) rlt_adam_step_guarded alone against the recipe step without EMA and with one group: equal bytes, 28 n.  (b) the
    recipe step with EMA and AttnCut's real group table (no decay on biases and norms, the cut head at half the rate; at BiCut's
    size the same 30 slots scaled up) against the composition it replaces: rlt_adam_step_guarded + ema.lerp_(p, 1 - d) + a
    host-computed lr - the common, non-skipped step.  HIP events around single alternating launches, the median of `reps`; GB/s on
    each pass's algorithmic bytes (recipe with EMA 36 n, the composition 40 n)."""
    import ctypes
    import math
    import models
    from rlt_hip.parallel import FlatModel, resolve_param_groups
    lr, b1, b2, eps, wd, d = 3e-5, 0.9, 0.999, 1e-8, 0.005, 0.999
    flat = FlatModel(models.AttnCut(input_size=3))
    groups = resolve_param_groups(flat.names, [("*bias*", {"weight_decay": 0.0}), ("*norm*", {"weight_decay": 0.0}),
                                               ("decison_layer.*", {"lr_scale": 0.5})], wd)
    sizes = [int(b - a) for a, b in zip(flat.offsets.tolist(), flat.offsets.tolist()[1:])]
    for label, n in (("AttnCut", flat.numel), ("BiCut", 237600000)):
        k = n // flat.numel                                      # BiCut's size: the same table with every slot k times as long
        offs = [0]
        for sz in sizes:
            offs.append(offs[-1] + sz * k)
        offs[-1] = n
        off_t = torch.tensor(offs, dtype=torch.int64, device=dev)
        grp_t = torch.tensor(groups, dtype=torch.float32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(3)
        p, g = torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen) * 1e-3
        m, v, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
        state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device=dev)
        rstate = torch.zeros(N.RECIPE_STATE_WORDS, dtype=torch.int64, device=dev)
        sched = dict(sched_kind="cosine", warmup_steps=100, total_steps=100000, min_lr_ratio=0.1)
        r_plain = N.recipe_struct(base_lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, **sched)
        r_full = N.recipe_struct(base_lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, decoupled=True, ema_decay=d, **sched)
        t = [0]

        def guarded():
            call("rlt_adam_step_guarded", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(state), lr, b1, b2, eps, wd, 0, stream())

        def recipe_plain():
            call("rlt_adam_step_recipe", ptr(p), ptr(g), ptr(m), ptr(v), None, n, None, None, 0, ptr(state), ptr(rstate),
                 ctypes.byref(r_plain), stream())

        def recipe_full():
            call("rlt_adam_step_recipe", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, ptr(off_t), ptr(grp_t), len(groups), ptr(state),
                 ptr(rstate), ctypes.byref(r_full), stream())

        def composed():
            t[0] += 1
            lr_t = lr * 0.5 * (1.0 + math.cos(math.pi * min(t[0], 100000) / 100000))       # the host advances the schedule
            call("rlt_adam_step_guarded", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(state), lr_t, b1, b2, eps, wd, 0, stream())
            ema.lerp_(p, 1.0 - d)
        fns = (("adam_step_guarded", guarded, 28), ("recipe, no ema, 1 group", recipe_plain, 28), ("recipe, ema, 30 groups", recipe_full, 36),
               ("guarded + lerp_ + host lr", composed, 40))
        times = {name: [] for name, _, _ in fns}
        call("rlt_grad_norm", ptr(g), n, None, 0, 0.0, ptr(N.byte_buffer(N.query("rlt_grad_norm_workspace", n, 0), dev)),
             N.query("rlt_grad_norm_workspace", n, 0), None, ptr(state), stream())          # coef = 1, nonfinite = 0 in the state
        for _ in range(2):
            for _, fn, _ in fns:
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, fn, _ in fns:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b))
        med = {name: sorted(ts)[reps // 2] for name, ts in times.items()}
        for name, _, per in fns:
            ms, ts = med[name], times[name]
            print(f"recipe {label:8s} n={n:10d} {name:26s}: {ms * 1e3:9.1f} us (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f})  "
                  f"{per * n / ms / 1e6:8.1f} GB/s on {per} n bytes = {per * n / ms / 1e6 / 8000 * 100:4.1f} % of 8 TB/s", flush=True)
        names = [nm for nm, _, _ in fns]
        print(f"recipe {label:8s} recipe (no ema) / guarded: {med[names[1]] / med[names[0]]:.2f}x;  composition / recipe (ema, groups): "
              f"{med[names[3]] / med[names[2]]:.2f}x"
              + ("  (the fused pass is SLOWER than the composition here)" if med[names[2]] > med[names[3]] else ""), flush=True)
        del p, g, m, v, ema
        torch.cuda.empty_cache()


def compare():
    """The paired comparison pass (rlt_paired_compare: R sign-flip replicates and R bootstrap replicates of M systems over Q
    queries) against the best torch composition of the same two statistics, tiled over replicates so that its tensors fit.
    The composition is searched, each half on its own: the randomization sums over {int8 randint bits, bits unpacked from int32
    random words} x {signs @ d, 2 (bits @ d) - sum d, d @ signs.T, where(bit, -d, d).sum per system}; the bootstrap sums over
    d[:, idx].sum with int64 and int32 indices, dT[idx].sum and dT.index_select(int32).sum.  Every form is timed at tiles that
    grow by 4 until its per-replicate time stops falling (or the tile's tensors pass TILE_BYTES, or a gather 2^31 elements), on up to two tiles' worth
    after a warm-up tile; the fastest (form, tile) of each half makes the composition that is timed over all R.  HIP events
    around single alternating calls, the median of `reps` (15 at the small shape, 7 at the large ones, where a composition
    pass takes seconds), with the minimum and maximum; draws = 2 R Q (one sign and one index per replicate and query)."""
    TILE_BYTES = 96e9
    shifts = torch.arange(32, dtype=torch.int32, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for Q, M, R, first_tile, reps in ((1 << 20, 1, 10000, 64, 7), (1 << 20, 4, 10000, 64, 7), (250, 4, 100000, 1024, 15)):
        gen = torch.Generator(device=dev).manual_seed(5)
        base = torch.rand(Q, device=dev, generator=gen)
        sys_ = base[None, :] + 0.05 * torch.randn(M, Q, device=dev, generator=gen)
        plan = N.paired_compare_plan(Q, M, R)
        wsb = N.query("rlt_paired_compare_workspace", Q, M, R)
        ws = N.byte_buffer(wsb, dev)
        rec = torch.zeros(M, N.CMP_WORDS, dtype=torch.int64, device=dev)
        rs, bs = torch.empty(M, R, dtype=torch.float64, device=dev), torch.empty(M, R, dtype=torch.float64, device=dev)
        d = sys_.double() - base.double()[None, :]
        dT = d.t().contiguous()
        t_obs = d.sum(1)

        def kernel():
            call("rlt_paired_compare", ptr(base), ptr(sys_), Q, Q, M, R, 7, ptr(ws), wsb, ptr(rec), ptr(rs), ptr(bs), stream())

        def bits_int8(t):
            return torch.randint(0, 2, (t, Q), device=dev, dtype=torch.int8)

        def bits_words(t):
            w = torch.randint(-2 ** 31, 2 ** 31, (t, (Q + 31) // 32), device=dev, dtype=torch.int32)
            return ((w[:, :, None] >> shifts) & 1).reshape(t, -1)[:, :Q]

        def s_matmul(b):
            return (b.double() * 2 - 1) @ dT                                    # (t, M)

        def s_matmul01(b):
            return 2 * (b.double() @ dT) - t_obs[None, :]

        def s_dmatmul(b):
            return (d @ (b.double() * 2 - 1).t()).t()

        def s_where(b):
            nz = b.bool()
            return torch.stack([torch.where(nz, -d[m], d[m]).sum(1) for m in range(M)], 1)

        def g_adv64(t):
            return d[:, torch.randint(0, Q, (t, Q), device=dev)].sum(-1)        # (M, t)

        def g_adv32(t):
            return d[:, torch.randint(0, Q, (t, Q), device=dev, dtype=torch.int32)].sum(-1)

        def g_rows64(t):
            return dT[torch.randint(0, Q, (t, Q), device=dev)].sum(1).t()

        def g_select32(t):
            idx = torch.randint(0, Q, (t * Q,), device=dev, dtype=torch.int32)
            return dT.index_select(0, idx).view(t, Q, M).sum(1).t()

        sign_forms = {f"{bn}+{sn}": (lambda t, bf=bf, sf=sf: sf(bf(t)))
                      for bn, bf in (("int8", bits_int8), ("words", bits_words))
                      for sn, sf in (("signs@d", s_matmul), ("2(bits@d)-sum", s_matmul01), ("d@signs.T", s_dmatmul), ("where", s_where))}
        boot_forms = {"d[:,idx64]": g_adv64, "d[:,idx32]": g_adv32}
        if M == 1:          # at M = 4 torch refused a launch of the row forms ("invalid configuration argument"); cause not looked into
            boot_forms.update({"dT[idx64]": g_rows64, "dT.index_select(idx32)": g_select32})
        # bytes of a tile's largest tensors: float64 signs and bits / int64 indices and the M gathered float64 planes
        sign_bytes, boot_bytes = (lambda t: t * Q * 20.0), (lambda t: t * Q * (8.0 + 8.0 * M))

        def search(forms, tile_bytes, count):
            """{form: {tile: us per replicate}} and the fastest (us, form, tile)"""
            table, best = {}, None
            for name, fn in forms.items():
                table[name], tile, last = {}, min(first_tile, R), None
                while True:
                    n = min(R, 2 * tile)

                    def run(n=n, tile=tile):
                        acc = torch.zeros(M, device=dev)
                        for r0 in range(0, n, tile):
                            acc += count(fn(min(tile, n - r0)))
                    fn(tile)
                    torch.cuda.synchronize()
                    us = timed(run) / n * 1e3
                    table[name][tile] = us
                    if best is None or us < best[0]:
                        best = (us, name, tile)
                    # a gather is kept below 2^31 gathered elements: beyond it torch's index kernels refuse the launch
                    if tile >= R or tile_bytes(4 * tile) > TILE_BYTES or (last is not None and us > 0.97 * last) \
                            or (forms is boot_forms and 4 * tile * Q * M >= 2 ** 31):
                        break
                    last, tile = us, min(4 * tile, R)
                torch.cuda.empty_cache()
            return table, best
        s_table, s_best = search(sign_forms, sign_bytes, lambda sg: (sg.abs() >= t_obs.abs()[None, :]).sum(0))
        b_table, b_best = search(boot_forms, boot_bytes, lambda bt: (bt <= 0).sum(1))

        def composed():
            ge, le = torch.zeros(M, device=dev), torch.zeros(M, device=dev)
            for r0 in range(0, R, s_best[2]):
                ge += (sign_forms[s_best[1]](min(s_best[2], R - r0)).abs() >= t_obs.abs()[None, :]).sum(0)
            for r0 in range(0, R, b_best[2]):
                le += (boot_forms[b_best[1]](min(b_best[2], R - r0)) <= 0).sum(1)
            return ge, le
        kernel()
        composed()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(reps):
            tk.append(timed(kernel))
            tc.append(timed(composed))
        mk, mc = sorted(tk)[reps // 2], sorted(tc)[reps // 2]
        draws = 2.0 * R * Q
        print(f"compare Q={Q} M={M} R={R} form={plan['form']} chunks={plan['chunks']} workspace={wsb / 1e6:.1f} MB", flush=True)
        for title, table, best in (("randomization", s_table, s_best), ("bootstrap", b_table, b_best)):
            for name, row in table.items():
                print(f"compare   torch {title:13s} {name:24s} us per replicate at tile " + ", ".join(f"{t}: {v:.3f}" for t, v in row.items()), flush=True)
            print(f"compare   torch {title:13s} best: {best[1]} at tile {best[2]}, {best[0]:.3f} us per replicate", flush=True)
        print(f"compare   rlt_paired_compare: {mk:10.3f} ms (min {min(tk):.3f}, max {max(tk):.3f}, {reps} calls)  {draws / mk / 1e6:8.2f} G draws/s", flush=True)
        print(f"compare   torch composition : {mc:10.3f} ms (min {min(tc):.3f}, max {max(tc):.3f}, {reps} calls)  {draws / mc / 1e6:8.2f} G draws/s"
              f"   composition / kernel: {mc / mk:.2f}x"
              + ("  (the kernel is SLOWER than the torch composition here)" if mk > mc else ""), flush=True)
        del base, sys_, ws, rs, bs, d, dT
        torch.cuda.empty_cache()


def reward_any(shapes=((4096, 300), (1048576, 300)), reps=9):
    """rlt_reward_any_loss (JS, tau 0.85) with the reward built from the labels (F_2) and with a supplied reward matrix, against the
    torch composition it replaces - float32 softmax of r / tau, logs, the per-list sums, argmax of p and r and the gathers at them, dp
    by the closed form, on a reward matrix that already exists - and beside rlt_loss_metrics (F1, JS) at the same shape: the pass
    of equal algorithmic bytes, 12 S per list (8 S read, 4 S of dp written).  HIP events around single alternating launches, the
    median of `reps`."""
    from utils.rewards import RewardSpec
    spec = RewardSpec.fbeta(2.0)
    tau = 0.85
    for B, S in shapes:
        g = torch.Generator(device=dev).manual_seed(11)
        prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32, device=dev) / 45.0) + 0.02
        y = (torch.rand(B, S, device=dev, generator=g) < prob).float()
        p = torch.softmax(torch.randn(B, S, device=dev, generator=g), 1).contiguous()
        r = ops.reward_spec_matrix(y, spec)
        struct, _keep = spec.native(S, dev)
        tab = ops.dcg_table(dev)
        per, loss, dp = torch.empty(B, device=dev), torch.empty(1, device=dev), torch.empty(B, S, device=dev)
        k, bk = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        rk, rb, sums = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
        wsb = N.query("rlt_reward_any_workspace", B)
        ws = N.workspace(wsb, dev)
        f1, dcg, s2 = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev), \
            torch.empty(2, dtype=torch.float64, device=dev)
        lwsb = N.query("rlt_loss_metrics_workspace", B)
        lws = N.workspace(lwsb, dev)

        def from_spec():
            call("rlt_reward_any_loss", ptr(p), ptr(y), N.ctypes.byref(struct), None, B, S, N.LOSS_JS, tau, ptr(per), ptr(loss), ptr(dp),
                 ptr(k), ptr(rk), ptr(rb), ptr(bk), ptr(sums), None, ptr(ws), wsb, stream())

        def from_matrix():
            call("rlt_reward_any_loss", ptr(p), None, None, ptr(r), B, S, N.LOSS_JS, tau, ptr(per), ptr(loss), ptr(dp),
                 ptr(k), ptr(rk), ptr(rb), ptr(bk), ptr(sums), None, ptr(ws), wsb, stream())

        def f1_yardstick():
            call("rlt_loss_metrics", ptr(p), ptr(y), None, B, S, N.METRIC_F1, -1.0, N.LOSS_JS, tau, -1.0, ptr(per), ptr(loss), ptr(dp),
                 ptr(k), ptr(f1), ptr(dcg), ptr(s2), ptr(tab), ptr(lws), lwsb, stream())

        def composed_torch():
            q = torch.softmax(r / tau, 1)
            lm = torch.log((p + q) * 0.5)
            lp = torch.log(p)
            per_t = 0.5 * ((torch.xlogy(q, q) - q * lm).sum(1) + (p * lp - p * lm).sum(1))
            dp_t = (0.5 / B) * (lp - lm)
            kk = p.argmax(1, keepdim=True)
            bb = r.argmax(1, keepdim=True)
            r_k, r_b = r.gather(1, kk), r.gather(1, bb)
            return per_t.sum(dtype=torch.float64) / B, dp_t, kk, r_k.sum(dtype=torch.float64), r_b.sum(dtype=torch.float64), (r_k == r_b).sum()
        fns = (("rlt_reward_any_loss, spec (F_2 from the labels)", from_spec), ("rlt_reward_any_loss, supplied matrix", from_matrix),
               ("rlt_loss_metrics, F1 (equal bytes)", f1_yardstick), ("torch composition on the matrix", composed_torch))
        for _name, fn in fns:
            fn()
        torch.cuda.synchronize()
        # the three forms of the new loss agree before anything is timed
        from_spec()
        l_spec = loss.clone()
        from_matrix()
        ref = composed_torch()
        assert torch.allclose(l_spec, loss, rtol=1e-6) and abs(float(ref[0]) - float(loss)) <= 1e-4 * abs(float(loss)), (l_spec, loss, ref[0])
        assert torch.allclose(dp, ref[1], rtol=1e-3, atol=1e-9) and int(ref[5]) == int(sums[2])
        times = {name: [] for name, _fn in fns}
        for _ in range(reps):
            for name, fn in fns:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b))
        nbytes = 12.0 * B * S
        med = {name: sorted(v)[reps // 2] for name, v in times.items()}
        for name, v in times.items():
            print(f"reward_any B{B} S{S} {name:48s}: {med[name] * 1e3:10.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, {reps} calls)  "
                  f"{nbytes / med[name] / 1e6:8.1f} GB/s on 12 S bytes per list", flush=True)
        names = [n for n, _ in fns]
        print(f"reward_any B{B} S{S} spec / rlt_loss_metrics: {med[names[0]] / med[names[2]]:.2f}x   matrix / rlt_loss_metrics: "
              f"{med[names[1]] / med[names[2]]:.2f}x   torch composition / matrix: {med[names[3]] / med[names[1]]:.2f}x"
              + ("  (the kernel is SLOWER than the torch composition here)" if med[names[1]] > med[names[3]] else ""), flush=True)
        del y, p, r, dp, ref
        torch.cuda.empty_cache()


def reward_eval(shapes=((1048576, 300),), cuts=(1, 19), reps=9):
    """rlt_reward_eval (nDCG built from the labels, every output on) against the best composition of what existed before it:
    rlt_reward_spec_matrix for the (B,S) reward, then torch - sum(0) in float64 for the curve, max(1) for the best cut, gather at
    the cuts, compare-and-count for `better`, bincount for the histogram.  HIP events around single alternating launches, the
    median of `reps`; GB/s on the pass's algorithmic bytes, 4 S + 4 T per list."""
    from utils.rewards import RewardSpec
    spec = RewardSpec.ndcg()
    for B, S in shapes:
        g = torch.Generator(device=dev).manual_seed(11)
        prob = 0.55 * torch.exp(-torch.arange(S, dtype=torch.float32, device=dev) / 45.0) + 0.02
        y = (torch.rand(B, S, device=dev, generator=g) < prob).float()
        for T in cuts:
            k = torch.randint(0, S + 1, (B, T), device=dev, generator=g, dtype=torch.int32)
            k64 = k.long()
            res = {}

            def fused():
                res["fused"] = ops.reward_eval(y, spec, k=k, allow_empty=True)

            def composed():
                r = ops.reward_spec_matrix(y, spec)
                full = torch.cat([torch.zeros(B, 1, device=dev), r], 1)
                curve = full.sum(0, dtype=torch.float64)
                best, best_k = full.max(1)
                r_at = full.gather(1, k64)
                better = torch.stack([(full > r_at[:, t:t + 1]).sum(1, dtype=torch.int32) for t in range(T)], 1)
                hist = torch.bincount(best_k, minlength=S + 1)
                sums = (best.sum(dtype=torch.float64), r_at.sum(0, dtype=torch.float64), (r_at == best[:, None]).sum(0),
                        better.sum(0, dtype=torch.float64))
                res["composed"] = (curve, best, best_k, r_at, better, hist, sums)
            fns = (("rlt_reward_eval, every output", fused), ("rlt_reward_spec_matrix + torch composition", composed))
            for _name, fn in fns:
                fn()
            torch.cuda.synchronize()
            out, acc = res["fused"]
            curve, best, best_k, r_at, better, hist, _sums = res["composed"]
            assert torch.equal(out["r_at"], r_at) and torch.equal(out["best"], best) and torch.equal(out["better"], better)
            assert torch.equal(acc["best_hist"], hist.double()) and torch.allclose(acc["curve"], curve, rtol=1e-12)
            times = {name: [] for name, _fn in fns}
            for _ in range(reps):
                for name, fn in fns:
                    res.clear()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    times[name].append(a.elapsed_time(b))
            nbytes = (4.0 * S + 4.0 * T) * B
            med = {name: sorted(v)[reps // 2] for name, v in times.items()}
            for name, v in times.items():
                print(f"reward_eval B{B} S{S} T{T} {name:44s}: {med[name] * 1e3:10.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, "
                      f"{reps} calls)  {nbytes / med[name] / 1e6:8.1f} GB/s on 4 S + 4 T bytes per list", flush=True)
            names = [n for n, _ in fns]
            print(f"reward_eval B{B} S{S} T{T} composition / fused: {med[names[1]] / med[names[0]]:.2f}x"
                  + ("  (the fused pass is SLOWER than the composition here)" if med[names[0]] > med[names[1]] else ""), flush=True)
            res.clear()
            del k, k64, out, acc, curve, best, best_k, r_at, better, hist
            torch.cuda.empty_cache()


def seq_attention(shapes=((4096, 300, 4, 64), (8192, 300, 8, 16)), reps=7, runs=2, layer=True):
    """Within-list attention (rlt_seq_attention_fwd / _bwd) at (B, S, H, HD): the median of `reps` HIP-event timings in each of `runs`
    separate runs, TFLOP/s of the algorithm's flops (4*B*H*S*S*HD forward, 2.5 x that backward: five products) against the 157.3
    TFLOP/s f32-MFMA peak; against the composition a user would otherwise write in torch (permute to (B, H, S, HD), fp32
    scaled_dot_product_attention - matmul / softmax / matmul if it refuses fp32 - and permute back, autograd backward; the permutes
    counted); the list-axis launches at the same shape for context; and the encoder-layer step (forward + backward) per axis."""
    import statistics
    PEAK = 157.3

    def median_ms(fn):
        fn()                                                     # warm-up: code objects, allocator
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    for B, S, H, HD in shapes:
        E, T = H * HD, S * B
        gf = 4.0 * B * H * S * S * HD / 1e9
        qkv = torch.randn(T, 3 * E, device=dev)
        dout = torch.randn(T, E, device=dev)
        out, lse, dqkv = torch.empty(T, E, device=dev), torch.empty(B, H, S, device=dev), torch.empty_like(qkv)
        D = N.PRECISION_DEFAULT
        fwd = lambda: call("rlt_seq_attention_fwd", ptr(qkv), S, B, H, HD, 0.0, 0, ptr(out), ptr(lse), D, stream())
        bwd = lambda: call("rlt_seq_attention_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, 0, ptr(dqkv), None, 0, D, stream())

        x = qkv.detach().clone().requires_grad_(True)

        def torch_fwd():
            q, k, v = x.view(S, B, 3, H, HD).permute(2, 1, 3, 0, 4)
            try:
                o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
            except RuntimeError:
                o = torch.softmax(q @ k.transpose(-1, -2) / HD ** 0.5, -1) @ v
            return o.permute(2, 0, 1, 3).reshape(T, E)

        def torch_both():
            x.grad = None
            torch_fwd().backward(dout)

        def torch_fwd_only():
            with torch.no_grad():
                torch_fwd()

        o_t = torch_fwd().detach()
        fwd()
        torch.cuda.synchronize()
        print(f"seq_attention B{B} S{S} H{H} HD{HD}: max |out - torch| = {float((out - o_t).abs().max()):.2e}", flush=True)
        for r in range(runs):
            f, b = median_ms(fwd), median_ms(bwd)
            tf, tb = median_ms(torch_fwd_only), median_ms(torch_both)
            print(f"  run {r}: rlt fwd {f:8.3f} ms {gf / f:6.1f} TF/s ({100 * gf / f / PEAK:4.1f} % of peak) | bwd {b:8.3f} ms "
                  f"{2.5 * gf / b:6.1f} TF/s ({100 * 2.5 * gf / b / PEAK:4.1f} %) | fwd+bwd {f + b:8.3f} ms", flush=True)
            print(f"  run {r}: torch composition fwd {tf:8.3f} ms | fwd+bwd {tb:8.3f} ms | rlt / torch: fwd {f / tf:5.2f}, fwd+bwd {(f + b) / tb:5.2f}"
                  + ("  (SLOWER than the torch composition here)" if f + b > tb else ""), flush=True)
        del x, o_t
        torch.cuda.empty_cache()
        # context: the list-axis launches at the same shape (4*S*H*B*B*HD flops per product pass: B / S times the work)
        lse_l = torch.empty(S, H, B, device=dev)
        ib = N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, 0.0, D)
        images = torch.empty(max(ib, 16) // 4, device=dev) if ib else None
        wb = N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, 0.0, D)
        ws = torch.empty(wb // 4 + 4, device=dev)
        lf = median_ms(lambda: call("rlt_list_attention_fwd", ptr(qkv), S, B, H, HD, 0.0, 0, ptr(out), ptr(lse_l), ptr(images), ib, D, stream()))
        lb = median_ms(lambda: call("rlt_list_attention_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse_l), S, B, H, HD, 0.0, 0, ptr(images),
                                    ptr(dqkv), ptr(ws), wb, D, stream()))
        print(f"  context: list-axis launches at the same shape: fwd {lf:8.3f} ms | bwd {lb:8.3f} ms", flush=True)
        del images, ws, qkv, dout, out, dqkv
        torch.cuda.empty_cache()
        if layer:
            from models._common import ParamTree
            lay = ParamTree(torch.nn.TransformerEncoderLayer(E, H, dropout=0.0)).to(dev)
            h = torch.randn(T, E, device=dev, requires_grad=True)
            g = torch.randn(T, E, device=dev)
            for axis in ("list", "position"):
                def step():
                    h.grad = None
                    for p in lay.parameters():
                        p.grad = None
                    ops.encoder_layer(h, lay, S, B, H, axis=axis).backward(g)
                print(f"  encoder layer step (fwd + bwd), axis={axis}: {median_ms(step):8.3f} ms", flush=True)
            del lay, h, g
            torch.cuda.empty_cache()


SEQ_SHAPES = ((4096, 300, 4, 64), (8192, 300, 8, 16))


def _seq_median_ms(fn, reps):
    import statistics
    fn()                                                         # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def seq_attention_causal(shapes=SEQ_SHAPES, reps=7, runs=2, layer=True):
    """Causal within-list attention (rlt_seq_attention_fwd_ex / _bwd_ex, RLT_SEQ_MASK_CAUSAL) at (B, S, H, HD): the median of `reps`
    HIP-event timings in each of `runs` runs, forward and backward, of
      the causal kernels; the non-causal kernels in the same process (the calls without _ex); the composition a user would otherwise
      write in torch (permute to (B, H, S, HD), fp32 scaled_dot_product_attention(is_causal=True), permute back, autograd backward;
      the permutes counted); one encoder-layer step (forward + backward) on the position axis with and without the mask.
    The causal / non-causal share is printed beside what the tile count expects (the 32 x 32 products on and below the diagonal over
    all of them: 55 / 100 at S = 300) - nothing here fixes a ratio in advance.
    RLT_PARENT_LIB=<a library built from the parent commit>: it is loaded beside the product library and its rlt_seq_attention_fwd /
    _bwd are timed in the same runs on the same buffers; this build's non-causal medians are compared with them, the margin being
    the parent's own spread between its two runs."""
    import ctypes
    D = N.PRECISION_DEFAULT
    mine, theirs = {}, {}
    parent = os.environ.get("RLT_PARENT_LIB")
    plib = ctypes.CDLL(os.path.abspath(parent)) if parent else None
    for name in ("rlt_seq_attention_fwd", "rlt_seq_attention_bwd") if plib else ():
        getattr(plib, name).restype, getattr(plib, name).argtypes = N._SIGNATURES[name]
    for B, S, H, HD in shapes:
        E, T = H * HD, S * B
        nb = (S + 31) // 32
        share = nb * (nb + 1) / 2 / (nb * nb)
        qkv, dout = torch.randn(T, 3 * E, device=dev), torch.randn(T, E, device=dev)
        out, lse, dqkv = torch.empty(T, E, device=dev), torch.empty(B, H, S, device=dev), torch.empty_like(qkv)
        fwd = lambda: call("rlt_seq_attention_fwd", ptr(qkv), S, B, H, HD, 0.0, 0, ptr(out), ptr(lse), D, stream())
        bwd = lambda: call("rlt_seq_attention_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, 0, ptr(dqkv), None, 0, D, stream())
        cfwd = lambda: call("rlt_seq_attention_fwd_ex", ptr(qkv), S, B, H, HD, 0.0, 0, N.SEQ_MASK_CAUSAL, ptr(out), ptr(lse), D, stream())
        cbwd = lambda: call("rlt_seq_attention_bwd_ex", ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, 0, N.SEQ_MASK_CAUSAL,
                            ptr(dqkv), None, 0, D, stream())


        def pfwd():
            assert plib.rlt_seq_attention_fwd(ptr(qkv), S, B, H, HD, 0.0, 0, ptr(out), ptr(lse), D, stream()) == 0

        def pbwd():
            assert plib.rlt_seq_attention_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), S, B, H, HD, 0.0, 0, ptr(dqkv), None, 0, D, stream()) == 0
        x = qkv.detach().clone().requires_grad_(True)

        def torch_fwd():
            q, k, v = x.view(S, B, 3, H, HD).permute(2, 1, 3, 0, 4)
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
            return o.permute(2, 0, 1, 3).reshape(T, E)

        def torch_both():
            x.grad = None
            torch_fwd().backward(dout)

        def torch_fwd_only():
            with torch.no_grad():
                torch_fwd()

        o_t = torch_fwd().detach()
        cfwd()
        torch.cuda.synchronize()
        tag = f"B{B} S{S} H{H} HD{HD}"
        print(f"seq_attention_causal {tag}: max |out - torch| = {float((out - o_t).abs().max()):.2e}; expected share of the 32 x 32 "
              f"products {nb * (nb + 1) // 2} / {nb * nb} = {share:.3f}", flush=True)
        del o_t
        for r in range(runs):
            f, b, cf, cb = (_seq_median_ms(fn, reps) for fn in (fwd, bwd, cfwd, cbwd))
            tf, tb = _seq_median_ms(torch_fwd_only, reps), _seq_median_ms(torch_both, reps)
            mine[(tag, r)] = (f, b)
            print(f"seq_noncausal {tag} run {r} fwd {f:.4f} ms bwd {b:.4f} ms", flush=True)
            if plib:
                theirs[(tag, r)] = (_seq_median_ms(pfwd, reps), _seq_median_ms(pbwd, reps))
                print(f"seq_parent    {tag} run {r} fwd {theirs[(tag, r)][0]:.4f} ms bwd {theirs[(tag, r)][1]:.4f} ms (the parent commit's "
                      "library, non-causal)", flush=True)
            print(f"seq_causal    {tag} run {r} fwd {cf:.4f} ms bwd {cb:.4f} ms | causal / non-causal: fwd {cf / f:.3f} bwd {cb / b:.3f} "
                  f"fwd+bwd {(cf + cb) / (f + b):.3f} (tile count: {share:.3f})"
                  + ("  (causal is SLOWER than non-causal here)" if cf + cb > f + b else ""), flush=True)
            print(f"seq_torch     {tag} run {r} sdpa(is_causal) fwd {tf:.4f} ms fwd+bwd {tb:.4f} ms | rlt causal / torch: fwd {cf / tf:.3f} "
                  f"fwd+bwd {(cf + cb) / tb:.3f}" + ("  (SLOWER than the torch composition here)" if cf + cb > tb or cf > tf else ""), flush=True)
        del x, qkv, dout, out, lse, dqkv
        torch.cuda.empty_cache()
        if layer:
            from models._common import ParamTree
            lay = ParamTree(torch.nn.TransformerEncoderLayer(E, H, dropout=0.0)).to(dev)
            h = torch.randn(T, E, device=dev, requires_grad=True)
            g = torch.randn(T, E, device=dev)
            for r in range(runs):
                ms = {}
                for causal in (False, True):
                    def step():
                        h.grad = None
                        for p in lay.parameters():
                            p.grad = None
                        ops.encoder_layer(h, lay, S, B, H, axis="position", causal=causal).backward(g)
                    ms[causal] = _seq_median_ms(step, reps)
                print(f"seq_layer     {tag} run {r} encoder layer step (fwd + bwd), position axis: mask none {ms[False]:.3f} ms, causal "
                      f"{ms[True]:.3f} ms, causal / none {ms[True] / ms[False]:.3f}", flush=True)
            del lay, h, g
            torch.cuda.empty_cache()
    if not plib:
        print("seq_parent: RLT_PARENT_LIB not set - no comparison with the parent commit's non-causal kernels", flush=True)
        return
    for tag in sorted({t for t, _ in mine}):
        for i, what in enumerate(("fwd", "bwd")):
            p, c = [theirs[(tag, r)][i] for r in range(runs)], [mine[(tag, r)][i] for r in range(runs)]
            spread = max(p) - min(p)
            diff = sum(c) / len(c) - sum(p) / len(p)
            print(f"seq_parent    {tag} {what}: parent {p[0]:.4f} / {p[1]:.4f} ms (spread {spread:.4f}), this build non-causal {c[0]:.4f} / {c[1]:.4f} ms, mean difference "
                  f"{diff:+.4f} ms -> " + ("within the parent's spread" if abs(diff) <= spread else
                                           ("FASTER than the parent beyond its spread" if diff < 0 else "SLOWER than the parent beyond its spread")),
                  flush=True)


def rerank(shapes=((4096, 300), (1048576, 300)), companions=(1, 3), reps=7, runs=2):
    """rlt_rerank_lists (perm, rank, sorted values and n companion arrays: every output on) against the torch compositions a user
    would otherwise write: torch.sort(-pred, stable=True) + a gather per array (+ a scatter for rank), and argsort +
    take_along_dim.  The median of `reps` HIP-event timings in each of `runs` separate runs; GB/s on the pass's algorithmic bytes,
    4 S (1 + n) read + 4 S (3 + n) written per list, against the 8 TB/s of HBM.  (torch's descending order differs on NaNs; the
    inputs here hold none.)"""
    import statistics
    HBM = 8000.0

    def median_ms(fn):
        fn()                                                     # warm-up: code objects, allocator
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    for B, S in shapes:
        g = torch.Generator(device=dev).manual_seed(5)
        pred = torch.randn(B, S, device=dev, generator=g)
        pred[:, ::7] = torch.round(pred[:, ::7])                 # some ties: the order must be the stable one
        for n in companions:
            arrays = [torch.rand(B, S, device=dev, generator=g) for _ in range(n)]
            res = {}

            def fused():
                res["fused"] = ops.rerank_lists(pred, *arrays, want_perm=True, want_rank=True, want_sorted=True)

            def sort_gather():
                neg, idx = torch.sort(-pred, dim=1, stable=True)
                rank = torch.empty_like(idx).scatter_(1, idx, torch.arange(S, device=dev).expand(B, S))
                res["sort"] = (idx, rank, -neg, [a.gather(1, idx) for a in arrays])

            def argsort_take():
                idx = torch.argsort(pred, dim=1, descending=True, stable=True)
                rank = torch.argsort(idx, dim=1)
                res["argsort"] = (idx, rank, torch.take_along_dim(pred, idx, 1), [torch.take_along_dim(a, idx, 1) for a in arrays])
            fns = (("rlt_rerank_lists, every output", fused), ("torch.sort(stable) + gather + scatter", sort_gather),
                   ("torch.argsort x2 + take_along_dim", argsort_take))
            for _name, fn in fns:
                fn()
            torch.cuda.synchronize()
            perm, rank, srt, moved = res["fused"]
            for key in ("sort", "argsort"):
                idx, rk, sv, mv = res[key]
                assert torch.equal(perm.long(), idx) and torch.equal(rank.long(), rk) and torch.equal(srt, sv)
                assert all(torch.equal(a, b) for a, b in zip(moved, mv))
            res.clear()
            del perm, rank, srt, moved, idx, rk, sv, mv
            torch.cuda.empty_cache()
            nbytes = (4.0 * S * (1 + n) + 4.0 * S * (3 + n)) * B
            for r in range(runs):
                med = {}
                for name, fn in fns:
                    med[name] = median_ms(fn)
                    res.clear()
                    torch.cuda.empty_cache()
                for name, _fn in fns:
                    gbs = nbytes / med[name] / 1e6
                    print(f"rerank B{B} S{S} n{n} run {r} {name:40s}: {med[name] * 1e3:10.1f} us  {gbs:8.1f} GB/s on the algorithmic "
                          f"bytes ({100 * gbs / HBM:4.1f} % of 8 TB/s)", flush=True)
                best = min(med[name] for name, _fn in fns[1:])
                print(f"rerank B{B} S{S} n{n} run {r} best torch composition / rlt_rerank_lists: {best / med[fns[0][0]]:.2f}x"
                      + ("  (SLOWER than the torch composition here)" if med[fns[0][0]] > best else ""), flush=True)
            del arrays
            torch.cuda.empty_cache()


def pair_rank(shapes=((4096, 300), (1048576, 40)), reps=7, runs=2):
    """rlt_pair_rank_loss (loss + dscore in one call, ops.PairRankLossFn's forward) against a tiled torch composition of the same
    loss (s[:, :, None] - s[:, None, :], softplus, masks, autograd; tiles of lists so that the (b,S,S) temporaries stay near
    0.5 GB) and against the hinge it replaces (rlt_mt_terms + rlt_mt_terms_bwd).  0/1 labels at about 5 % relevant and 4 grades;
    RankNet and LambdaRank.  The median of `reps` HIP-event timings in each of `runs` separate runs; pair visits per second on
    the S^2 ordered pairs of every list."""
    import statistics
    from rlt_hip import native as N

    def median_ms(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    ops.dcg_table(dev)
    for B, S in shapes:
        g = torch.Generator(device=dev).manual_seed(5)
        score = torch.randn(B, S, device=dev, generator=g)
        tile = max(1, min(B, (1 << 27) // (S * S)))
        disc = 1.0 / torch.log2(torch.arange(S, device=dev, dtype=torch.float32) + 2.0)
        for label_name, n_grades in (("binary 5%", 2), ("4 grades", 4)):
            if n_grades == 2:
                labels = (torch.rand(B, S, device=dev, generator=g) < 0.05).float()
            else:
                labels = torch.randint(0, 4, (B, S), device=dev, generator=g).float()
            gains = (2.0 ** labels) - 1.0
            for kind in ("ranknet", "lambdarank"):
                def fused():
                    s = score.clone().requires_grad_(True)
                    ops.PairRankLossFn.apply(s, labels, kind, 1.0, None, n_grades, False).backward()
                    return s.grad

                def composed():
                    grad = torch.empty_like(score)
                    for lo in range(0, B, tile):
                        s = score[lo:lo + tile].clone().requires_grad_(True)
                        y, G = labels[lo:lo + tile], gains[lo:lo + tile]
                        pair = y[:, :, None] > y[:, None, :]
                        l = torch.nn.functional.softplus(-(s[:, :, None] - s[:, None, :]))
                        if kind == "lambdarank":
                            rank = torch.argsort(torch.argsort(s.detach(), dim=1, descending=True, stable=True), dim=1)
                            D = disc[rank]
                            w = (G[:, :, None] - G[:, None, :]).abs() * (D[:, :, None] - D[:, None, :]).abs()
                            per = (l * w * pair).sum(dim=(1, 2))
                        else:
                            per = (l * pair).sum(dim=(1, 2)) / pair.sum(dim=(1, 2)).clamp(min=1)
                        (per.sum() / B).backward()
                        grad[lo:lo + tile] = s.grad
                    return grad

                def hinge():
                    s = score.clone().requires_grad_(True)
                    ops.RerankLossFn.apply(s, labels.clamp(max=1.0), 5e-4).backward()
                    return s.grad
                a, b = fused(), composed()
                err = float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
                del a, b
                torch.cuda.empty_cache()
                for r in range(runs):
                    med = {name: median_ms(fn) for name, fn in (("rlt_pair_rank_loss", fused), ("tiled torch composition", composed),
                                                                 ("rlt_mt_terms + _bwd (hinge)", hinge))}
                    for name, ms in med.items():
                        print(f"pair_rank B{B} S{S} {label_name:10s} {kind:10s} run {r} {name:30s}: {ms * 1e3:10.1f} us  "
                              f"{B * S * S / ms / 1e6:8.2f} G pair visits/s", flush=True)
                    print(f"pair_rank B{B} S{S} {label_name:10s} {kind:10s} run {r} torch / kernel {med['tiled torch composition'] / med['rlt_pair_rank_loss']:.1f}x, "
                          f"kernel / hinge {med['rlt_pair_rank_loss'] / med['rlt_mt_terms + _bwd (hinge)']:.1f}x, "
                          f"max |kernel - torch| / max |torch| = {err:.1e}", flush=True)
                    torch.cuda.empty_cache()


def hazard(shapes=((4096, 300, 256), (8192, 300, 128)), reps=7, runs=2):
    """rlt_hazard_head_fwd / _bwd at (B, S, E) against their yardstick - rlt_heads_fwd / _bwd with ONE softmax head at the same
    shape, in the same job: both passes read x once (forward) or read x and write dx once (backward), equal algorithmic bytes -
    and against a torch composition of the same head (linear, logsigmoid, cumsum, exp, autograd).  The median of `reps` HIP-event
    timings in each of `runs` separate runs; GB/s on the algorithmic bytes 4 S B E (forward) and 8 S B E (backward)."""
    for B, S, E in shapes:
        g = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn(S * B, E, device=dev, generator=g)
        w = torch.randn(1, E, device=dev, generator=g) / E ** 0.5
        b = torch.randn(1, device=dev, generator=g)
        off = ops.hazard_prior_offset(S, dev)
        dp, dstop = torch.randn(B, S, device=dev, generator=g), torch.randn(B, S, device=dev, generator=g)
        p, stop, z, out = (torch.empty(B, S, device=dev) for _ in range(4))
        dx, dw, db = torch.empty(S * B, E, device=dev), torch.empty(1, E, device=dev), torch.empty(1, device=dev)
        kinds = (N.c_int * 1)(N.HEAD_SOFTMAX)
        hz_bytes = N.query("rlt_hazard_head_bwd_workspace", S, B, E)
        hd_bytes = N.query("rlt_heads_bwd_workspace", 1, S, B, E)
        hz_ws, hd_ws = N.workspace(hz_bytes, dev), N.workspace(hd_bytes, dev)

        def hz_fwd():
            call("rlt_hazard_head_fwd", ptr(x), ptr(w), ptr(b), ptr(off), S, B, E, ptr(p), ptr(stop), ptr(z), stream())

        def hz_bwd():
            call("rlt_hazard_head_bwd", ptr(x), ptr(w), ptr(z), ptr(dp), ptr(dstop), S, B, E, ptr(dx), 0, ptr(dw), ptr(db),
                 ptr(hz_ws), hz_bytes, stream())

        def hd_fwd():
            call("rlt_heads_fwd", ptr(x), ptr(w), ptr(b), kinds, 1, S, B, E, ptr(out), stream())

        def hd_bwd():
            call("rlt_heads_bwd", ptr(x), ptr(w), kinds, 1, ptr(out), ptr(dp), S, B, E, ptr(dx), 0, ptr(dw), ptr(db),
                 ptr(hd_ws), hd_bytes, stream())

        F = torch.nn.functional
        xt, wt, bt = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)

        def composed(backward):
            zz = (F.linear(xt, wt, bt).view(S, B).t() + off)[:, :S - 1]
            L = torch.cat([zz.new_zeros(B, 1), torch.cumsum(F.logsigmoid(-zz), 1)], 1)
            pp = torch.exp(torch.cat([F.logsigmoid(zz), zz.new_zeros(B, 1)], 1) + L)
            ss = torch.cat([torch.sigmoid(zz), zz.new_ones(B, 1)], 1)
            if backward:
                xt.grad = wt.grad = bt.grad = None
                torch.autograd.backward([pp, ss], [dp, dstop])
            return pp

        hz_fwd()
        err = float((p - composed(False).detach()).abs().max())
        for r in range(runs):
            med = {"rlt_hazard_head_fwd": _seq_median_ms(hz_fwd, reps), "rlt_heads_fwd (1 softmax head)": _seq_median_ms(hd_fwd, reps),
                   "torch composition fwd": _seq_median_ms(lambda: composed(False), reps),
                   "rlt_hazard_head_bwd": _seq_median_ms(hz_bwd, reps), "rlt_heads_bwd (1 softmax head)": _seq_median_ms(hd_bwd, reps),
                   "torch composition fwd+bwd": _seq_median_ms(lambda: composed(True), reps)}
            for name, ms in med.items():
                nbytes = (8 if "bwd" in name else 4) * S * B * E
                print(f"hazard B{B} S{S} E{E} run {r} {name:32s}: {ms * 1e3:9.1f} us  {nbytes / ms / 1e6:8.1f} GB/s", flush=True)
            print(f"hazard B{B} S{S} E{E} run {r} hazard / heads: fwd {med['rlt_hazard_head_fwd'] / med['rlt_heads_fwd (1 softmax head)']:.3f}x, "
                  f"bwd {med['rlt_hazard_head_bwd'] / med['rlt_heads_bwd (1 softmax head)']:.3f}x; torch / hazard: fwd "
                  f"{med['torch composition fwd'] / med['rlt_hazard_head_fwd']:.1f}x, fwd+bwd "
                  f"{med['torch composition fwd+bwd'] / (med['rlt_hazard_head_fwd'] + med['rlt_hazard_head_bwd']):.1f}x; "
                  f"max |p - torch fp32| = {err:.1e}", flush=True)
        del x, dx, xt
        torch.cuda.empty_cache()


def _once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stream_bench(reps=7, runs=2, S=300, pages=(1, 10, 32)):
    """Streaming truncation (rlt_seq_attention_append, rlt_hazard_head_append, utils/stream.py): the total time to stream S = 300 ranks
    in pages of 1, 10 and 32, the median of `reps` HIP-event timings in each of `runs` runs, against two yardsticks measured in the
    same job with the one-shot kernels:
      (a) ONE one-shot causal forward of the whole list - the floor: streaming does the same arithmetic in more launches;
      (b) one one-shot causal forward PER PAGE - what a caller has to do without the streaming calls (at page 1 that is 300
          forwards: the model-level figure is one timing per run, not a median).
    Two configurations: the whole model (Choopy, 8192 lists, E 128, 8 heads, 3 layers: model.stream against
    model.stop_probabilities) and the attention alone (4096 lists, 4 heads of 64).  At page 10 a second line retires every other
    list at rank 30.  Last, the append kernel alone at C = 1, t0 = 299, as GB/s on its 8 t B E bytes of cache."""
    import models as hm
    D = N.PRECISION_DEFAULT
    npages = lambda c: (S + c - 1) // c
    # ---- the attention alone
    B, H, HD = 4096, 4, 64
    E = H * HD
    qkv = torch.randn(S * B, 3 * E, device=dev)
    out, lse = torch.empty(S * B, E, device=dev), torch.empty(B, H, S, device=dev)
    cache = torch.empty(S * B, 2 * E, device=dev)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    half = ones.clone()
    half[::2] = 0
    upper = ones.clone()
    upper[B // 2:] = 0
    one_shot = lambda: call("rlt_seq_attention_fwd_ex", ptr(qkv), S, B, H, HD, 0.0, 0, N.SEQ_MASK_CAUSAL, ptr(out), ptr(lse), D, stream())

    def append(t0, c, active=None):
        call("rlt_seq_attention_append", N.c_void_p(qkv.data_ptr() + 4 * t0 * B * 3 * E), ptr(cache), t0, c, S, B, H, HD, ptr(active),
             N.c_void_p(out.data_ptr() + 4 * t0 * B * E), ptr(lse), D, stream())

    def attn_stream(c, retire_at=None):
        for t0 in range(0, S, c):
            append(t0, min(c, S - t0), None if retire_at is None else (ones if t0 < retire_at else half))

    def per_page(fn, c):
        for _ in range(npages(c)):
            fn()

    for r in range(runs):
        a = _seq_median_ms(one_shot, reps)
        print(f"stream attention B{B} S{S} H{H} HD{HD} run {r} (a) one-shot causal forward: {a:9.3f} ms", flush=True)
        for c in pages:
            s, b = _seq_median_ms(lambda: attn_stream(c), reps), _seq_median_ms(lambda: per_page(one_shot, c), reps)
            print(f"stream attention B{B} S{S} H{H} HD{HD} run {r} page {c:2d}: streamed {s:9.3f} ms = {s / a:6.2f} x (a) | (b) {npages(c)} one-shot "
                  f"forwards {b:9.3f} ms | (b) / streamed {b / s:6.2f} x", flush=True)
        s = _seq_median_ms(lambda: attn_stream(10, 30), reps)
        print(f"stream attention B{B} S{S} H{H} HD{HD} run {r} page 10, every other list retired at rank 30: {s:9.3f} ms", flush=True)
        t = _seq_median_ms(lambda: append(S - 1, 1), reps)
        print(f"stream attention B{B} S{S} H{H} HD{HD} run {r} append alone C 1 t0 {S - 1}: {t * 1e3:9.1f} us  "
              f"{8 * (S - 1) * B * E / t / 1e6:8.1f} GB/s on 8 t B E", flush=True)
        for what, act in (("every other list retired", half), ("the second half of the lists retired", upper)):
            t = _seq_median_ms(lambda: append(S - 1, 1, act), reps)
            print(f"stream attention B{B} S{S} H{H} HD{HD} run {r} append alone C 1 t0 {S - 1}, {what}: {t * 1e3:9.1f} us  "
                  f"{8 * (S - 1) * (B // 2) * E / t / 1e6:8.1f} GB/s on 8 t (B/2) E", flush=True)
    # the append kernel alone at head dim 16 (Choopy's heads)
    del qkv, out, cache
    B, H, HD = 8192, 8, 16
    E = H * HD
    qkv, out, cache = torch.randn(B, 3 * E, device=dev), torch.empty(B, E, device=dev), torch.randn(S * B, 2 * E, device=dev)
    for r in range(runs):
        t = _seq_median_ms(lambda: call("rlt_seq_attention_append", ptr(qkv), ptr(cache), S - 1, 1, S, B, H, HD, None, ptr(out), None, D, stream()), reps)
        print(f"stream attention B{B} S{S} H{H} HD{HD} run {r} append alone C 1 t0 {S - 1}: {t * 1e3:9.1f} us  "
              f"{8 * (S - 1) * B * E / t / 1e6:8.1f} GB/s on 8 t B E", flush=True)
    del qkv, out, cache
    torch.cuda.empty_cache()
    # ---- the whole model
    torch.manual_seed(3)
    m = hm.Choopy(seq_len=S, d_model=128, n_head=8, num_layers=3, dropout=0.0, attention_axis="position", attention_mask="causal",
                  cut_head="hazard").to(dev).eval()
    x = torch.randn(B, S, 1, device=dev)
    st = m.stream(2.0, B)                                           # tau = 2: nothing stops before the end
    chunks = {c: [x[:, t0:t0 + c].contiguous() for t0 in range(0, S, c)] for c in pages}
    forward = lambda: m.stop_probabilities(x)

    def model_stream(c, retire_at=None):
        st.reset()
        for page in chunks[c]:
            if retire_at is not None and st.position == retire_at:
                st.active[::2] = 0
            st.push(page)

    for r in range(runs):
        a = _seq_median_ms(forward, reps)
        print(f"stream choopy B{B} S{S} E128 H8 L3 run {r} (a) one-shot forward (stop_probabilities): {a:9.3f} ms", flush=True)
        for c in pages:
            s = _seq_median_ms(lambda: model_stream(c), reps)
            b = _seq_median_ms(lambda: per_page(forward, c), reps) if c > 1 else _once_ms(lambda: per_page(forward, c))
            print(f"stream choopy B{B} S{S} E128 H8 L3 run {r} page {c:2d}: streamed {s:9.3f} ms = {s / a:6.2f} x (a) | (b) {npages(c)} one-shot "
                  f"forwards {b:9.3f} ms{' (one timing)' if c == 1 else ''} | (b) / streamed {b / s:6.2f} x", flush=True)
        s = _seq_median_ms(lambda: model_stream(10, 30), reps)
        print(f"stream choopy B{B} S{S} E128 H8 L3 run {r} page 10, every other list retired at rank 30: {s:9.3f} ms", flush=True)


def stream_compact_bench(reps=7, runs=2, S=300, pages=(10, 32)):
    """Streaming truncation with batch compaction (rlt_stream_compact_plan, rlt_kv_cache_compact, StreamingTruncator.compact): the
    shapes and the method of `stream` - medians of `reps` HIP-event timings in each of `runs` runs.
      1. the whole model (Choopy, 8192 lists, E 128, 8 heads, 3 layers): the time to stream 300 ranks with compact_every None, 1, and
         3 with compact_below 0.5, under four retirement schedules forced through `active`: none; every other list at rank 30; the
         second half of the lists at rank 30; geometric - half of the live lists every 30 ranks.  Beside each time the rows the GEMMs
         ran over, as a fraction of 300 * 8192.
      2. the attention alone (4096 lists, 4 heads of 64): the append kernel at C = 1, t0 = 299 on the full batch, on the batch with
         lists retired through `active`, and on the compacted cache; and the streamed attention at page 10.
      3. the gather kernel alone, as GB/s on its 2 * 4 * t0 * B_dst * W bytes (the float4-copy yardstick is tools/micro/membw, run in
         the same job), and the plan launch at B = 8192 and 1,048,576."""
    import models as hm
    from rlt_hip import ops
    D = N.PRECISION_DEFAULT
    i32 = lambda *a, **k: torch.zeros(*a, dtype=torch.int32, device=dev, **k)

    def retire(active, how):
        """clear entries of a slot array on the device, no host read: 'alternate' every second LIVE slot, 'upper' the second half of them"""
        live = active != 0
        cs = torch.cumsum(live.int(), 0)
        gone = (cs % 2 == 0) if how == "alternate" else (2 * cs > cs[-1])
        active[gone & live] = 0

    # ---- 3. the two kernels alone
    for B, Bd, W, t0s in ((8192, 4096, 256, (150, 299)), (4096, 2048, 512, (150, 299))):
        src, dst = torch.randn(S * B, W, device=dev), torch.empty(S * Bd, W, device=dev)
        for what in ("alternate", "upper"):
            act = torch.ones(B, dtype=torch.int32, device=dev)
            retire(act, what)
            plan = ops.stream_compact_plan(act)
            assert int(plan["n_live"].item()) == Bd
            for t0 in t0s:
                for r in range(runs):
                    t = _seq_median_ms(lambda: call("rlt_kv_cache_compact", ptr(src), ptr(dst), ptr(plan["slot_src"]), t0, B, Bd, W, stream()), reps)
                    print(f"stream_compact gather {B} -> {Bd} lists ({'every other list' if what == 'alternate' else 'the first half'} live) W{W} "
                          f"t0 {t0} run {r}: {t * 1e3:9.1f} us  {2 * 4 * t0 * Bd * W / t / 1e6:8.1f} GB/s on 2*4*t0*B_dst*W", flush=True)
        del src, dst
    torch.cuda.empty_cache()
    for B in (8192, 1 << 20):
        act = (torch.arange(B, device=dev) % 3 != 0).int()
        org, car, k, kf = torch.arange(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.float64, device=dev), i32(B), i32(B)
        outs = [i32(B), i32(B), torch.empty(B, dtype=torch.float64, device=dev), i32(1)]
        f = lambda: call("rlt_stream_compact_plan", ptr(act), ptr(org), ptr(car), ptr(k), B, B, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(kf),
                         ptr(outs[3]), stream())
        for r in range(runs):
            print(f"stream_compact plan B {B} (origin, carry and k given) run {r}: {_seq_median_ms(f, reps) * 1e3:9.1f} us", flush=True)
    # ---- 2. the attention alone
    B, H, HD = 4096, 4, 64
    E = H * HD
    qkv = torch.randn(S * B, 3 * E, device=dev)
    out = torch.empty(S * B, E, device=dev)
    cache, cache2 = torch.randn(S * B, 2 * E, device=dev), torch.empty(S * B, 2 * E, device=dev)

    def append(t0, c, cch, Bs, active=None):
        call("rlt_seq_attention_append", N.c_void_p(qkv.data_ptr() + 4 * t0 * Bs * 3 * E), ptr(cch), t0, c, S, Bs, H, HD, ptr(active),
             N.c_void_p(out.data_ptr() + 4 * t0 * Bs * E), None, D, stream())

    def attn_stream(c, how, compact):
        act, cch, oth, Bs = torch.ones(B, dtype=torch.int32, device=dev), cache, cache2, B
        for t0 in range(0, S, c):
            if how and t0 and t0 % 30 == 0 and (how == "geometric" or t0 == 30):
                retire(act, "alternate" if how != "upper" else "upper")
                if compact:
                    plan = ops.stream_compact_plan(act)
                    n = int(plan["n_live"].item())
                    if n:
                        call("rlt_kv_cache_compact", ptr(cch), ptr(oth), ptr(plan["slot_src"]), t0, Bs, n, 2 * E, stream())
                    cch, oth, Bs, act = oth, cch, n, torch.ones(n, dtype=torch.int32, device=dev)
            if Bs:
                append(t0, min(c, S - t0), cch, Bs, act)

    for r in range(runs):
        t = _seq_median_ms(lambda: append(S - 1, 1, cache, B), reps)
        print(f"stream_compact attention B{B} S{S} H{H} HD{HD} run {r} append alone C 1 t0 {S - 1}, full batch: {t * 1e3:9.1f} us", flush=True)
        for how, label in (("alternate", "every other list retired"), ("upper", "the second half of the lists retired")):
            act = torch.ones(B, dtype=torch.int32, device=dev)
            retire(act, how)
            plan = ops.stream_compact_plan(act)
            n = int(plan["n_live"].item())
            call("rlt_kv_cache_compact", ptr(cache), ptr(cache2), ptr(plan["slot_src"]), S - 1, B, n, 2 * E, stream())
            t_act = _seq_median_ms(lambda: append(S - 1, 1, cache, B, act), reps)
            t_cmp = _seq_median_ms(lambda: append(S - 1, 1, cache2, n), reps)
            print(f"stream_compact attention B{B} S{S} H{H} HD{HD} run {r} append alone C 1 t0 {S - 1}, {label}: through `active` {t_act * 1e3:9.1f} us | "
                  f"compacted to {n} lists {t_cmp * 1e3:9.1f} us  {8 * (S - 1) * n * E / t_cmp / 1e6:8.1f} GB/s on 8 t B_live E", flush=True)
        for how in ("alternate", "upper", "geometric"):
            a, b = _seq_median_ms(lambda: attn_stream(10, how, False), reps), _seq_median_ms(lambda: attn_stream(10, how, True), reps)
            print(f"stream_compact attention B{B} S{S} H{H} HD{HD} run {r} page 10, {how} from rank 30: through `active` {a:9.3f} ms | compacted {b:9.3f} ms "
                  f"(plan, read and gather included) = {b / a:5.3f} x" + ("  (compaction is SLOWER here)" if b > a else ""), flush=True)
    del qkv, out, cache, cache2
    torch.cuda.empty_cache()
    # ---- 1. the whole model
    B = 8192
    torch.manual_seed(3)
    m = hm.Choopy(seq_len=S, d_model=128, n_head=8, num_layers=3, dropout=0.0, attention_axis="position", attention_mask="causal",
                  cut_head="hazard").to(dev).eval()
    x = torch.randn(B, S, 1, device=dev)
    chunks = {c: [x[:, t0:t0 + c].contiguous() for t0 in range(0, S, c)] for c in pages}
    modes = (("compact_every None", {}), ("compact_every 1", {"compact_every": 1}), ("compact_every 3, compact_below 0.5", {"compact_every": 3, "compact_below": 0.5}))
    trunc = {name: m.stream(2.0, B, **kw) for name, kw in modes}          # tau = 2: nothing stops by itself

    def model_stream(st, c, how):
        st.reset()
        nxt = 30
        for page in chunks[c]:
            if how and st.position >= nxt and st.slots:                    # the first page boundary at or behind rank 30, 60, ..
                retire(st.active, "upper" if how == "upper" else "alternate")
                nxt = nxt + 30 if how == "geometric" else S + 1
            st.push(page)

    for r in range(runs):
        for c in pages:
            for how, label in ((None, "no list retired"), ("alternate", "every other list retired at rank 30"),
                               ("upper", "the second half of the lists retired at rank 30"), ("geometric", "half of the live lists retired every 30 ranks")):
                base = None
                for name, _ in modes:
                    st = trunc[name]
                    t = _seq_median_ms(lambda: model_stream(st, c, how), reps)
                    base = t if base is None else base
                    extra = f" = {t / base:5.3f} x compact_every None" + ("  (compaction is SLOWER here)" if t > base else "") if name != modes[0][0] else ""
                    if how is None and name != modes[0][0]:
                        extra += f", {(t - base) * 1e3 / len(chunks[c]):7.1f} us per push"
                    print(f"stream_compact choopy B{B} S{S} E128 H8 L3 run {r} page {c:2d}, {label}, {name}: {t:9.3f} ms, GEMM rows "
                          f"{st.rows_computed() / (S * B):5.3f} of S*B{extra}", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["attention", "gemms", "lstm"]
    print("env:", {k: v for k, v in os.environ.items() if k.startswith("RLT_")}, flush=True)
    for w in which:
        ({"stream": stream_bench, "stream_compact": stream_compact_bench}.get(w) or globals()[w])()          # (`stream` itself is the library's stream getter)
