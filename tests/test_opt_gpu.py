"""The guarded optimizer step on the device (csrc/optim.hip) through the raw C ABI and through FusedAdam, against the float64
restatement of tests/opt_restate.py (pinned to torch in tests/test_opt_restate.py).

C = elements one workgroup takes per trip and G = the grid cap of the norm pass are read from the library.  Sizes and segment
tables sit on the chunk edges: n in {4, C-4, C, C+4, 2C+8, G*C+4} (the last one forces the second grid-stride trip), slots of
{4, 8, C-4, C+4, 3C+12} elements in two orders (a boundary exactly on a chunk edge, a segment straddling one, one spanning
several chunks, a 4-element segment alone in a chunk's tail).

Tolerances.  Exact operands (integers in [-8, 8] times 2^-6: every square and every partial sum is exact in float64): zero.
Random operands: a float64 sum of n non-negative terms is within n * 2^-53 relative of the exact sum in any order (the squares
of float32 values are exact in float64), asserted against numpy's float64 sum with n = the elements of that sum.  The update:
twice the distance of rlt_adam_step itself (coefficient folded into g on the host) from the restatement, measured in the same
test per array - the allowance for the one extra multiply and the device pow.  Measured on an MI355X (distance / largest
magnitude of the array, after 5 steps at n = 2C + 8 = 8200; guarded / rlt_adam_step): p 1.00e-7 / 1.00e-7, exp_avg 2.22e-7 /
2.13e-7, exp_avg_sq 1.284e-5 / 1.284e-5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opt_restate as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ranked-list-truncation_amd")
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.999, 1e-8, 0.005
U = 2.0 ** -53


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


@pytest.fixture(scope="module")
def CG(N):
    return N.query("rlt_grad_norm_chunk"), N.load().rlt_grad_norm_grid()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _exact(n, seed):
    """integers in [-8, 8] times 2^-6, float32"""
    return (np.random.RandomState(seed).randint(-8, 9, size=n).astype(np.float32) / 64.0).astype(np.float32)


def _new_state(N):
    return torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device="cuda")


def _read_state(N, state):
    w = state.cpu()
    f64, f32 = w.view(torch.float64), w.view(torch.float32)
    out = {k: int(w[i]) for k, i in (("step", N.OPT_STEP), ("skipped", N.OPT_SKIPPED), ("clipped", N.OPT_CLIPPED),
                                     ("nonfinite", N.OPT_NONFINITE), ("nan_count", N.OPT_NAN), ("norm_steps", N.OPT_NORM_STEPS))}
    out.update({k: float(f64[i]) for k, i in (("sumsq", N.OPT_SUMSQ), ("norm", N.OPT_NORM), ("max_abs", N.OPT_MAX_ABS),
                                              ("norm_sum", N.OPT_NORM_SUM), ("norm_max", N.OPT_NORM_MAX))})
    out["coef"] = f32[N.OPT_COEF_F32].numpy().copy()
    out["words"] = w.numpy().copy()
    return out


def _grad_norm(N, g, offsets=None, max_norm=0.0, state=None):
    """The raw entry point on device tensors -> (state dict read back, per-segment (sumsq, nonfinite, max_abs) arrays or None)."""
    n, n_seg = g.numel(), 0 if offsets is None else offsets.numel() - 1
    state = _new_state(N) if state is None else state
    ws_bytes = N.query("rlt_grad_norm_workspace", n, n_seg)
    ws = N.byte_buffer(ws_bytes, g.device)
    seg = torch.full((max(n_seg, 1), N.GRAD_SEG_WORDS), -1, dtype=torch.int64, device=g.device)
    N.call("rlt_grad_norm", N.ptr(g), n, N.ptr(offsets), n_seg, float(max_norm), N.ptr(ws), ws_bytes,
           N.ptr(seg) if n_seg else None, N.ptr(state), N.stream())
    torch.cuda.synchronize()
    segs = None
    if n_seg:
        s = seg.cpu()
        s64 = s.view(torch.float64)
        segs = (s64[:, 0].numpy().copy(), s[:, 1].numpy().copy(), s64[:, 2].numpy().copy())
    return _read_state(N, state), segs


def _guarded(N, p, g, m, v, state, skip, wd=WD):
    N.call("rlt_adam_step_guarded", N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), p.numel(), N.ptr(state), LR, B1, B2, EPS, wd, int(skip),
           N.stream())


def _plain(N, p, g, m, v, t, wd=WD):
    N.call("rlt_adam_step", N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), p.numel(), int(t), LR, B1, B2, EPS, wd, N.stream())


def _tables(C):
    """Two orders of the slot sizes {4, 8, C-4, C+4, 3C+12}.  A: offsets 0, C-4, C, C+8, 2C+12, 5C+24 - the 4-element slot is the
    tail of chunk 0 and ends exactly on the edge C, the (C+4)-slot straddles the edge 2C, the (3C+12)-slot spans chunks 2..5.
    B: offsets 0, 3C+12, 4C+16, 4C+20, 5C+16, 5C+24 - every boundary off the edges, the large slot first."""
    return {"A": np.cumsum([0, C - 4, 4, 8, C + 4, 3 * C + 12]), "B": np.cumsum([0, 3 * C + 12, C + 4, 4, C - 4, 8])}


def _check_against_restatement(N, g_np, offs_np, max_norm, tol_of):
    """One norm call vs the restatement; tol_of(n_elements) = the relative tolerance of a sum over n elements."""
    got, segs = _grad_norm(N, _dev(g_np), None if offs_np is None else _dev(offs_np, torch.int64), max_norm)
    want, wsegs = R.grad_norm(g_np, offs_np, max_norm)
    n = g_np.size
    assert got["nonfinite"] == want.nonfinite and got["nan_count"] == want.nan_count
    assert abs(got["sumsq"] - want.sumsq) <= tol_of(n) * want.sumsq
    assert got["max_abs"] == want.max_abs
    if want.nonfinite == 0:
        assert abs(got["norm"] - want.norm) <= (tol_of(n) + 2 * U) * want.norm
        assert got["norm_steps"] == 1 and got["norm_sum"] == got["norm"] == got["norm_max"]
    else:
        assert (np.isnan(got["norm"]) and np.isnan(want.norm)) or got["norm"] == want.norm == np.inf
        assert got["norm_steps"] == 0 and got["norm_sum"] == 0.0
    if wsegs is not None:
        for s, (ss, nf, mx) in enumerate(wsegs):
            cnt = int(offs_np[s + 1] - offs_np[s])
            assert abs(segs[0][s] - ss) <= tol_of(cnt) * ss, s
            assert segs[1][s] == nf and segs[2][s] == mx, s
    return got, want, segs


# ---------------------------------------------------------------------------------------------------------------- the norm
@pytest.mark.parametrize("size", ["4", "C-4", "C", "C+4", "2C+8", "GC+4"])
def test_norm_sizes_exact_operands(N, CG, size):
    C, G = CG
    n = {"4": 4, "C-4": C - 4, "C": C, "C+4": C + 4, "2C+8": 2 * C + 8, "GC+4": G * C + 4}[size]
    g = _exact(n, 11 + n % 97)
    for max_norm in (1e-3, 0.0, float("inf"), 1e9):         # clipping; off; off; on but above the norm
        got, want, _ = _check_against_restatement(N, g, None, max_norm, lambda k: 0.0)
        assert got["coef"].tobytes() == np.float32(want.coef).tobytes(), (max_norm, got["coef"], want.coef)
        if max_norm != 1e-3:
            assert got["coef"].tobytes() == np.float32(1.0).tobytes()
    assert float(want.coef) == 1.0 and R.grad_norm(g, None, 1e-3)[0].coef < 1.0


@pytest.mark.parametrize("order", ["A", "B"])
def test_norm_segment_tables_exact_operands(N, CG, order):
    C, _ = CG
    offs = _tables(C)[order]
    g = _exact(int(offs[-1]), 23)
    got, want, segs = _check_against_restatement(N, g, offs, 1e-3, lambda k: 0.0)
    assert got["coef"].tobytes() == np.float32(want.coef).tobytes()
    assert float(np.sum(segs[0])) == got["sumsq"] and segs[2].max() == got["max_abs"]      # exact operands: any order of the segments
    # the same bucket without a table: the same figures
    alone, _ = _grad_norm(N, _dev(g), None, 1e-3)
    assert alone["sumsq"] == got["sumsq"] and alone["coef"].tobytes() == got["coef"].tobytes()


@pytest.mark.parametrize("scale", [1.0, 1e4])
@pytest.mark.parametrize("shape", ["2C+8", "A", "B", "GC+4"])
def test_norm_random_operands_and_bitwise_repeat(N, CG, shape, scale):
    C, G = CG
    offs = _tables(C).get(shape)
    n = int(offs[-1]) if offs is not None else {"2C+8": 2 * C + 8, "GC+4": G * C + 4}[shape]
    g = (np.random.RandomState(31).standard_normal(n) * scale).astype(np.float32)
    got, want, segs = _check_against_restatement(N, g, offs, 1.0, lambda k: k * U)
    assert abs(float(got["coef"]) - float(want.coef)) <= (n * U + 2.0 ** -23) * float(want.coef) and got["coef"] < 1.0
    again, segs2 = _grad_norm(N, _dev(g), None if offs is None else _dev(offs, torch.int64), 1.0)
    assert again["words"].tobytes() == got["words"].tobytes()
    if offs is not None:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(segs, segs2))


def _nonfinite_cases(C, offs):
    big_lo, big_hi = [(int(a), int(b)) for a, b in zip(offs, offs[1:]) if b - a == 3 * C + 12][0]
    n = int(offs[-1])
    return {"nan_first": {0: np.nan}, "nan_last": {n - 1: np.nan}, "inf_chunk_end": {2 * C - 1: np.inf},
            "neg_inf_mid_segment": {(big_lo + big_hi) // 2 + 1: -np.inf},
            "two_segments": {C - 2: np.nan, n - 3: np.inf, n - 2: -np.inf}}     # A: the 4-slot and the large one; B: the large and the 8-slot


@pytest.mark.parametrize("order", ["A", "B"])
@pytest.mark.parametrize("case", ["nan_first", "nan_last", "inf_chunk_end", "neg_inf_mid_segment", "two_segments"])
def test_norm_nonfinite_elements(N, CG, case, order):
    C, _ = CG
    offs = _tables(C)[order]
    g = _exact(int(offs[-1]), 41)
    g[:] = np.where(g == 0, np.float32(1 / 64), g)            # no zeros: a dropped element always changes the sum
    for i, val in _nonfinite_cases(C, offs)[case].items():
        g[i] = val
    got, want, segs = _check_against_restatement(N, g, offs, 1e-3, lambda k: 0.0)
    assert got["nonfinite"] == len(_nonfinite_cases(C, offs)[case]) == int(segs[1].sum())
    assert (np.isnan(got["coef"]) and np.isnan(want.coef)) or got["coef"].tobytes() == np.float32(want.coef).tobytes()
    # without a bound the coefficient stays exactly 1 whatever the gradient holds
    off, _ = _grad_norm(N, _dev(g), _dev(offs, torch.int64), 0.0)
    assert off["coef"].tobytes() == np.float32(1.0).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the update
def _dist(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())


def _trajectory(N, n, scales, max_norm, skip, nan_step=None, check_unclipped=False):
    """`len(scales)` steps of (a) rlt_grad_norm + rlt_adam_step_guarded, (b) rlt_adam_step with the coefficient folded into g on
    the host and the host keeping the step count, (c) the float64 restatement, all from the same float32 inputs.  Returns per
    step the device state and the arrays of the three."""
    rs = np.random.RandomState(77)
    p0 = rs.standard_normal(n).astype(np.float32)
    grads = [(s * rs.standard_normal(n)).astype(np.float32) for s in scales]
    if nan_step is not None:
        grads[nan_step][n // 3] = np.nan
    pg, mg, vg = _dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pb, mb, vb = _dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pr, mr, vr = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    state, rst, t_host, steps = _new_state(N), R.OptState(), 0, []
    for i, g_np in enumerate(grads):
        g = _dev(g_np)
        before = [x.clone() for x in (pg, mg, vg)]
        state_before = state.clone()
        st, _ = _grad_norm(N, g, None, max_norm, state)
        _guarded(N, pg, g, mg, vg, state, skip)
        torch.cuda.synchronize()
        assert torch.equal(g.cpu().view(torch.int32), torch.from_numpy(g_np).view(torch.int32))          # g is not modified
        rst, _ = R.grad_norm(g_np, None, max_norm, rst)
        applied = R.adam_step_guarded(pr, g_np, mr, vr, rst, LR, B1, B2, EPS, WD, skip)
        if applied:
            t_host += 1
            with np.errstate(all="ignore"):
                _plain(N, pb, _dev(g_np * np.float32(rst.coef)), mb, vb, t_host)
        else:
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, (pg, mg, vg)))   # byte for byte
        if check_unclipped and not rst.coef < 1.0:
            # a step that does not clip: coef is exactly 1.0f, and the update is the one of the same kernel without a bound
            assert st["coef"].tobytes() == np.float32(1.0).tobytes()
            alt, alt_state = [x.clone() for x in before], state_before.clone()
            _grad_norm(N, g, None, float("inf"), alt_state)
            _guarded(N, alt[0], g, alt[1], alt[2], alt_state, skip)
            torch.cuda.synchronize()
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(alt, (pg, mg, vg)))
        steps.append({"state": _read_state(N, state), "coef_restated": rst.coef, "applied": applied,
                      "guarded": [x.cpu().numpy() for x in (pg, mg, vg)], "plain": [x.cpu().numpy() for x in (pb, mb, vb)],
                      "restated": [x.copy() for x in (pr, mr, vr)]})
    return steps, rst


def _assert_within_twice_the_plain_kernel(step, label):
    for name, a, b, ref in zip(("p", "exp_avg", "exp_avg_sq"), step["guarded"], step["plain"], step["restated"]):
        d_guarded, d_plain = _dist(a, ref), _dist(b, ref)
        print(f"{label} {name}: guarded {d_guarded:.3e}  rlt_adam_step {d_plain:.3e}  (of the largest magnitude)")
        assert d_plain > 0 and d_guarded <= 2 * d_plain, (label, name, d_guarded, d_plain)


def test_guarded_step_against_the_restatement(N, CG):
    C, _ = CG
    n = 2 * C + 8
    # |g| ~ scale * sqrt(n): 0.09 and 9 at n = 8200 against max_norm = 1 - steps 2 and 4 clip, steps 1, 3 and 5 do not
    steps, rst = _trajectory(N, n, (1e-3, 1e-1, 1e-3, 1e-1, 1e-3), 1.0, skip=0, check_unclipped=True)
    assert [float(s["coef_restated"]) < 1.0 for s in steps] == [False, True, False, True, False]
    for i, s in enumerate(steps):
        assert s["state"]["coef"].tobytes() == np.float32(s["coef_restated"]).tobytes() or \
            abs(float(s["state"]["coef"]) - float(s["coef_restated"])) <= (n * U + 2.0 ** -23) * float(s["coef_restated"])
        _assert_within_twice_the_plain_kernel(s, f"step {i + 1}")
    last = steps[-1]["state"]
    assert (last["step"], last["clipped"], last["skipped"], last["norm_steps"]) == (5, 2, 0, 5) == (rst.step, rst.clipped, rst.skipped, rst.norm_steps)
    assert abs(last["norm_sum"] - rst.norm_sum) <= 1e-12 * rst.norm_sum and abs(last["norm_max"] - rst.norm_max) <= 1e-12 * rst.norm_max


def test_nonfinite_step_is_skipped_and_later_steps_use_the_applied_count(N, CG):
    C, _ = CG
    steps, rst = _trajectory(N, 2 * C + 8, (1e-3, 1e-1, 1e-3, 1e-1, 1e-3), 1.0, skip=1, nan_step=2)
    assert [s["applied"] for s in steps] == [True, True, False, True, True]
    assert [s["state"]["step"] for s in steps] == [1, 2, 2, 3, 4] and [s["state"]["skipped"] for s in steps] == [0, 0, 1, 1, 1]
    assert steps[2]["state"]["nonfinite"] == 1 and np.isnan(steps[2]["state"]["norm"])
    last = steps[-1]["state"]
    assert (last["step"], last["skipped"], last["clipped"], last["norm_steps"]) == (4, 1, 2, 4) == (rst.step, rst.skipped, rst.clipped, rst.norm_steps)
    for i in (3, 4):                                           # the restatement's bias corrections there use t = 3 and t = 4
        _assert_within_twice_the_plain_kernel(steps[i], f"step {i + 1} after the skip")


def test_without_the_skip_a_nan_propagates_as_in_torch(N, CG):
    C, _ = CG
    steps, rst = _trajectory(N, 2 * C + 8, (1e-3, 1e-1, 1e-3, 1e-1, 1e-3), 1.0, skip=0, nan_step=2)
    assert all(s["applied"] for s in steps) and steps[-1]["state"]["step"] == 5 and steps[-1]["state"]["skipped"] == 0
    for i in (2, 3, 4):
        for a, ref in zip(steps[i]["guarded"], steps[i]["restated"]):
            assert np.isnan(ref).all() and np.isnan(a).all()   # the NaN coefficient reaches every element, as clip_grad_norm_'s does


# ---------------------------------------------------------------------------------------------------------------- FusedAdam
def _two_linears(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)).cuda()


def test_fused_adam_options_reproduce_the_c_abi(N):
    from rlt_hip.parallel import FlatModel, FusedAdam
    flat = FlatModel(_two_linears(3))
    assert flat.names == ["0.weight", "0.bias", "1.weight", "1.bias"]
    offs = [0, 16, 20, 28, 32]                                 # 15, 3, 6, 2 elements in 4-float slots
    assert flat.offsets.tolist() == offs and flat.offsets.is_cuda and flat.offsets.dtype == torch.int64 and flat.numel == 32
    opt = FusedAdam(flat, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.5, skip_nonfinite=True, segment_norms=True)
    p, m, v = flat.flat_param.clone(), torch.zeros(32, device="cuda"), torch.zeros(32, device="cuda")
    state = _new_state(N)
    grads = [_exact(32, 5) * 4, _exact(32, 6) / 8, _exact(32, 7), _exact(32, 8) * 2]       # norms about 2, 0.06, 0.5, 1
    grads[2][17] = np.inf
    norms, clipped, seg_last = [], 0, None
    for g_np in grads:
        for a, b in zip(offs, offs[1:]):                        # the padding of a slot stays zero, as autograd leaves it
            sz = flat.params[offs.index(a)].numel()
            g_np[a + sz:b] = 0
        flat.flat_grad.copy_(_dev(g_np))
        opt.step()
        st, segs = _grad_norm(N, flat.flat_grad, flat.offsets, 0.5, state)
        _guarded(N, p, flat.flat_grad, m, v, state, 1)
        torch.cuda.synchronize()
        for a, b in ((p, flat.flat_param), (m, opt.exp_avg), (v, opt.exp_avg_sq)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        gs = opt.grad_stats()
        assert all(t.is_cuda for t in gs.values())
        assert gs["sumsq"].item() == st["sumsq"] and gs["nonfinite"].item() == st["nonfinite"] and gs["max_abs"].item() == st["max_abs"]
        assert gs["coef"].cpu().numpy().tobytes() == st["coef"].tobytes()
        assert gs["seg_sumsq"].cpu().numpy().tobytes() == segs[0].tobytes() and gs["seg_nonfinite"].cpu().tolist() == segs[1].tolist()
        assert gs["seg_max_abs"].cpu().numpy().tobytes() == segs[2].tobytes()
        want, wsegs = R.grad_norm(g_np, offs, 0.5)
        assert st["sumsq"] == want.sumsq and [s[0] for s in wsegs] == segs[0].tolist()     # exact operands
        if want.nonfinite == 0:
            norms.append(want.norm)
            clipped += int(want.coef < 1.0)
        seg_last = wsegs
    assert clipped == 2 and len(norms) == 3
    sd = opt.state_dict()
    assert (sd["steps"], sd["clipped_steps"], sd["skipped_steps"]) == (3, 2, 1) and opt.steps == 0
    es = opt.epoch_stats(reset=True)
    assert (es["finite_steps"], es["clipped_steps"], es["skipped_steps"]) == (3, 2, 1)
    assert abs(es["grad_norm_mean"] - sum(norms) / 3) <= 1e-14 * es["grad_norm_mean"]      # three square roots and two additions
    assert abs(es["grad_norm_max"] - max(norms)) <= 1e-14 * max(norms)
    assert list(es["segment_norms"]) == flat.names
    for name, (ss, _, _) in zip(flat.names, seg_last):
        assert abs(es["segment_norms"][name] - np.sqrt(ss)) <= 1e-14 * np.sqrt(ss)
    again = opt.epoch_stats(reset=False)                        # the running figures and the two counters start over, the totals stay
    assert (again["finite_steps"], again["clipped_steps"], again["skipped_steps"]) == (0, 0, 0) and np.isnan(again["grad_norm_mean"])
    sd = opt.state_dict()
    assert (sd["steps"], sd["clipped_steps"], sd["skipped_steps"]) == (3, 2, 1)
    with pytest.raises(RuntimeError):
        FusedAdam(FlatModel(_two_linears(4)), lr=LR).epoch_stats()


def test_ops_grad_norm_wrapper(N, CG):
    from rlt_hip import ops
    C, _ = CG
    offs = _tables(C)["A"]
    g = _exact(int(offs[-1]), 51)
    out = ops.grad_norm(_dev(g), _dev(offs, torch.int64), max_norm=1e-3)
    want, wsegs = R.grad_norm(g, offs, 1e-3)
    assert out["sumsq"].item() == want.sumsq and out["nonfinite"].item() == 0 and out["max_abs"].item() == want.max_abs
    assert out["coef"].cpu().numpy().tobytes() == np.float32(want.coef).tobytes()
    assert out["seg_sumsq"].cpu().tolist() == [s[0] for s in wsegs]
    assert ops.grad_norm(_dev(g))["coef"].item() == 1.0 and "seg_sumsq" not in ops.grad_norm(_dev(g))


def test_fused_adam_with_the_options_off_is_the_plain_step(N):
    """Passes with and without the guarded step: the default FusedAdam is the one rlt_adam_step launch per step it always was."""
    from rlt_hip.parallel import FlatModel, FusedAdam
    flat = FlatModel(_two_linears(9))
    opt = FusedAdam(flat, lr=LR, weight_decay=WD)
    p, m, v = flat.flat_param.clone(), torch.zeros(flat.numel, device="cuda"), torch.zeros(flat.numel, device="cuda")
    for t in (1, 2, 3):
        g = _dev(_exact(flat.numel, 60 + t))
        flat.flat_grad.copy_(g)
        opt.step()
        N.call("rlt_adam_step", N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), flat.numel, t, LR, 0.9, 0.999, 1e-8, WD, N.stream())
    torch.cuda.synchronize()
    assert opt.steps == 3 and opt.state_dict()["steps"] == 3
    for a, b in ((p, flat.flat_param), (m, opt.exp_avg), (v, opt.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- the trainer
TAGS = ("train/grad_norm_epoch", "train/grad_norm_max_epoch", "train/clipped_steps", "train/skipped_steps")


def _run_trainer(tmp_path, name, extra):
    """run.py on the smallest synthetic set the suite writes (tests/test_parallel_gloo.py: 11 + 5 lists of 40 documents)."""
    from dataloader.synth import write_synthetic_robust04
    base = tmp_path / "data"
    if not base.exists():
        write_synthetic_robust04(str(base), "robust04", "drmm_tks", n_train=11, n_test=5, seq_len=40, seed=3)
    out = tmp_path / name
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO, os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, os.path.join(PKG, "run.py"), "--dataset-base", str(base), "--model-name", "attncut",
                          "--epochs", "2", "--batch-size", "4", "--use-conf", "0", "--seed", "3", "--history-json",
                          str(out / "history.json"), "--tensorboard-dir", str(out / "tb"), "--save-path", str(out / "best")] + extra,
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = [json.loads(line) for line in open(out / "tb" / "scalars.jsonl")]
    return rows, json.load(open(out / "history.json"))


def test_trainer_flags_log_the_four_scalars(tmp_path):
    rows, hist = _run_trainer(tmp_path, "guarded", ["--clip-grad-norm", "1e-3", "--skip-nonfinite", "1"])
    by_tag = {t: [r["value"] for r in rows if r["tag"] == t] for t in TAGS}
    steps_per_epoch = len([r for r in rows if r["tag"] == "train/loss_step"]) // 2
    assert steps_per_epoch == 3 and all(len(v) == 2 for v in by_tag.values())
    assert by_tag["train/clipped_steps"] == [steps_per_epoch] * 2 and by_tag["train/skipped_steps"] == [0, 0]
    assert all(np.isfinite(v) and v > 1e-3 for v in by_tag["train/grad_norm_epoch"])
    assert all(a >= b for a, b in zip(by_tag["train/grad_norm_max_epoch"], by_tag["train/grad_norm_epoch"]))
    assert all(np.isfinite(r["value"]) for r in rows if r["tag"] in ("train/loss_step", "train/loss_epoch", "test/loss_epoch"))
    for e, h in enumerate(hist["history"]):
        assert h["grad"] == {t.split("/", 1)[1]: by_tag[t][e] for t in TAGS}


def test_trainer_without_the_flags_logs_none_of_them(tmp_path):
    rows, hist = _run_trainer(tmp_path, "plain", [])
    assert not [r for r in rows if r["tag"] in TAGS] and all("grad" not in h for h in hist["history"])
    assert len([r for r in rows if r["tag"] == "train/loss_step"]) == 6
