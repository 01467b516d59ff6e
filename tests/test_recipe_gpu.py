"""The recipe step on the device (csrc/recipe.hip) through the raw C ABI, through FusedAdam and through run.py, against the float64
restatement of tests/recipe_restate.py (pinned to torch in tests/test_recipe_restate.py).

C = elements one workgroup takes per trip and G = the grid cap are read from the library.  Sizes sit on the chunk edges: n in {4,
C-4, C, C+4, 2C+8, G*C+4} (the last one forces the second grid-stride trip); the segment tables are the two orders of the slots
{4, 8, C-4, C+4, 3C+12} (A: offsets 0, C-4, C, C+8, 2C+12, 5C+24 - a boundary exactly on a chunk edge, a slot straddling one, one
spanning several chunks, a 4-element slot alone in a chunk's tail; B: 0, 3C+12, 4C+16, 4C+20, 5C+16, 5C+24 - every boundary off the
edges).  Every array sits between 64 sentinel floats that must not change.

Tolerances.  Exact operands (the group tags, the EMA of integers / 64 at decay 0.5, the schedule words): zero, or one float32 ulp
where the device's cos enters.  Random operands, 5 steps: rlt_adam_step_guarded runs on the same operands (coupled, one group,
constant lr, the same clip coefficient) and its distance from the restatement is measured per array; the recipe step must stay
within twice that - the project's allowance for one extra multiply (tests/test_opt_gpu.py), here the group's and the decay's.  The
run with table A's groups has the table's n = 5C+24, so the yardstick is measured there too, on the same operands (the n = 2C+8
runs take the first 2C+8 elements of the same arrays).  EMA: the p allowance plus steps * 2^-22 * max|p|, one rounding of each of
its two products per step.

Measured on an MI355X (distance / largest magnitude of the array after 5 steps; recipe / rlt_adam_step_guarded): coupled, one
group, n = 8200: p 9.113e-8 / 9.113e-8, exp_avg 2.109e-7 / 2.109e-7, exp_avg_sq 1.275e-5 / 1.275e-5; decoupled, table A, n = 20504:
p 1.143e-7 / 1.106e-7, exp_avg 2.643e-7 / 2.578e-7, exp_avg_sq 1.274e-5 / 1.286e-5; EMA |error| 4.86e-7 / 5.05e-7 against allowances
of 5.53e-6 / 5.69e-6; through FusedAdam: p 1.032e-7, exp_avg 2.639e-7, exp_avg_sq 1.278e-5."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opt_restate as R
import recipe_restate as RR

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ranked-list-truncation_amd")
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.999, 1e-8, 0.005
SENTINEL = -7.25
SCALES = (1.0, 0.5, 0.25, 0.0, 2.0)
TAG_WD = (2.0 ** -2, 2.0 ** -4, 2.0 ** -1, 2.0 ** -3, 2.0 ** -5)
RAND_WD = (0.005, 0.0, 0.01, 0.005, 0.02)


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


@pytest.fixture(scope="module")
def CG(N):
    return N.query("rlt_recipe_chunk"), N.load().rlt_recipe_grid()


def _tables(C):
    return {"A": np.cumsum([0, C - 4, 4, 8, C + 4, 3 * C + 12]), "B": np.cumsum([0, 3 * C + 12, C + 4, 4, C - 4, 8])}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Guarded:
    """n floats between two runs of 64 sentinels (256 bytes: the array keeps its 16-byte alignment)."""

    def __init__(self, init):
        init = torch.as_tensor(init, dtype=torch.float32)
        self.buf = torch.full((init.numel() + 128,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[64:64 + init.numel()]
        self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:64] == SENTINEL).all() and (self.buf[-64:] == SENTINEL).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


class Run:
    """One bucket's p, m, v (and ema) on the device with the two state records, stepped through the raw entry points."""

    def __init__(self, N, p0, offs=None, groups=None, ema0=None, m0=None, v0=None, **fields):
        self.N, self.n = N, len(p0)
        zeros = np.zeros(self.n, dtype=np.float32)
        self.p, self.m, self.v = Guarded(p0), Guarded(zeros if m0 is None else m0), Guarded(zeros if v0 is None else v0)
        self.ema = None if ema0 is None else Guarded(ema0)
        self.offs = None if offs is None else _dev(offs, torch.int64)
        self.groups = None if groups is None else _dev(np.asarray(groups, dtype=np.float32))
        self.n_seg = 0 if offs is None else len(offs) - 1
        self.state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device="cuda")
        self.rstate = torch.zeros(N.RECIPE_STATE_WORDS, dtype=torch.int64, device="cuda")
        self.recipe = N.recipe_struct(**fields)
        self.max_norm = 0.0
        if self.recipe.use_norm:
            self.ws_bytes = N.query("rlt_grad_norm_workspace", self.n, 0)
            self.ws = N.byte_buffer(self.ws_bytes, "cuda")

    def arrays(self):
        return [x.t for x in (self.p, self.m, self.v)] + ([self.ema.t] if self.ema else [])

    def intact(self):
        return all(x.intact() for x in (self.p, self.m, self.v) + ((self.ema,) if self.ema else ()))

    def step(self, g):
        import ctypes
        N = self.N
        if self.recipe.use_norm:
            N.call("rlt_grad_norm", N.ptr(g), self.n, None, 0, self.max_norm, N.ptr(self.ws), self.ws_bytes, None, N.ptr(self.state), N.stream())
        N.call("rlt_adam_step_recipe", N.ptr(self.p.t), N.ptr(g), N.ptr(self.m.t), N.ptr(self.v.t), N.ptr(self.ema.t) if self.ema else None,
               self.n, N.ptr(self.offs), N.ptr(self.groups), self.n_seg, N.ptr(self.state), N.ptr(self.rstate), ctypes.byref(self.recipe),
               N.stream())
        torch.cuda.synchronize()

    def words(self):
        N, w, r = self.N, self.state.cpu(), self.rstate.cpu()
        return {"step": int(w[N.OPT_STEP]), "skipped": int(w[N.OPT_SKIPPED]), "clipped": int(w[N.OPT_CLIPPED]),
                "lr": r.view(torch.float32)[N.RECIPE_LR_F32].numpy().copy(), "lr64": float(r.view(torch.float64)[N.RECIPE_LR64]),
                "ema_decay": r.view(torch.float32)[N.RECIPE_EMA_DECAY_F32].numpy().copy(), "ema_updates": int(r[N.RECIPE_EMA_UPDATES]),
                "rstate": r.numpy().copy()}


# ---------------------------------------------------------------------------------------------------------------- exact operands
@pytest.mark.parametrize("size", ["4", "C-4", "C", "C+4", "2C+8", "GC+4"])
def test_sizes_one_group_tag_and_guard_elements(N, CG, size):
    C, G = CG
    n = {"4": 4, "C-4": C - 4, "C": C, "C+4": C + 4, "2C+8": 2 * C + 8, "GC+4": G * C + 4}[size]
    one = torch.ones(n)
    run = Run(N, one, ema0=one, base_lr=2.0 ** -3, weight_decay=2.0 ** -2, decoupled=True, ema_decay=0.5, ema_warmup=False)
    g = torch.zeros(n, device="cuda")
    run.step(g)
    assert run.intact()
    p_new = np.float32(1 - 2.0 ** -5)
    assert bool((run.p.t == float(p_new)).all()) and bool((run.ema.t == float(np.float32(0.5 + 0.5 * p_new))).all())
    assert not bool(run.m.t.any()) and not bool(run.v.t.any()) and not bool(g.any())
    w = run.words()
    assert (w["step"], w["skipped"], w["ema_updates"]) == (1, 0, 1) and float(w["lr"]) == 2.0 ** -3 == w["lr64"]


@pytest.mark.parametrize("order", ["A", "B"])
def test_group_tags_name_every_elements_segment(N, CG, order):
    C, _ = CG
    offs = _tables(C)[order]
    n = int(offs[-1])
    groups = list(zip(SCALES, TAG_WD))
    frozen = [(int(a), int(b)) for (a, b), s in zip(zip(offs, offs[1:]), SCALES) if s == 0.0]
    rs = np.random.RandomState(3)
    init = [np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)]
    for a, b in frozen:                                        # arbitrary bits where nothing may be written
        for arr in init:
            arr[a:b] = rs.standard_normal(b - a).astype(np.float32)
    run = Run(N, init[0], offs, groups, ema0=init[3], m0=init[1], v0=init[2], base_lr=2.0 ** -3, decoupled=True, ema_decay=0.5,
              ema_warmup=False, weight_decay=0.75)             # the recipe's own weight decay is not read with a table
    run.step(torch.zeros(n, device="cuda"))
    assert run.intact()
    scale, wd = RR.expand_groups(n, offs, groups)
    want_p = np.where(scale == 0, init[0], 1.0 - 2.0 ** -3 * scale * wd).astype(np.float32)
    want_e = np.where(scale == 0, init[3], 0.5 + 0.5 * want_p.astype(np.float64)).astype(np.float32)
    assert len(np.unique(want_p[scale != 0])) == 4             # every live group has its own tag
    got = [_bits(t) for t in run.arrays()]
    assert np.array_equal(got[0], want_p.view(np.int32)) and np.array_equal(got[3], want_e.view(np.int32))
    assert np.array_equal(got[1], init[1].view(np.int32)) and np.array_equal(got[2], init[2].view(np.int32))
    for a, b in frozen:                                        # byte-identical in all four
        assert all(np.array_equal(x[a:b], y[a:b].view(np.int32)) for x, y in zip(got, init))


@pytest.mark.parametrize("warmup", [False, True])
def test_ema_exact_and_its_warmup_decay(N, CG, warmup):
    C, _ = CG
    n = 2 * C + 8
    rs = np.random.RandomState(4)
    p0 = (rs.randint(-64, 65, size=n) / 64.0).astype(np.float32)
    e0 = (rs.randint(-64, 65, size=n) / 64.0).astype(np.float32)
    run = Run(N, p0, ema0=e0, base_lr=2.0 ** -3, ema_decay=0.5, ema_warmup=warmup)
    g = torch.zeros(n, device="cuda")
    want = e0.astype(np.float64)
    for k in range(3):
        run.step(g)
        d = RR.ema_decay_at(k, 0.5, warmup)
        w = run.words()
        assert w["ema_decay"].tobytes() == np.float32(d).tobytes() and w["ema_updates"] == k + 1
        assert float(d) == (float(np.float32((0.1, 2 / 11, 0.25)[k])) if warmup else 0.5)
        want = np.float64(d) * want + (1.0 - np.float64(d)) * p0
        if not warmup:                                          # halves of integers / 64: exact in float32
            assert np.array_equal(_bits(run.ema.t), want.astype(np.float32).view(np.int32))
        else:                                                   # three roundings per step of values below 1
            assert np.abs(run.ema.t.cpu().numpy().astype(np.float64) - want).max() <= 3 * (k + 1) * 2.0 ** -24
    assert np.array_equal(_bits(run.p.t), p0.view(np.int32)) and run.intact()       # g = 0, no decay: p does not move


def test_schedule_words_on_the_device(N):
    W, T, base, ratio = 3, 8, 3e-5, 0.1
    g = torch.zeros(4, device="cuda")
    for kind in ("constant", "linear", "cosine"):
        run = Run(N, np.ones(4, dtype=np.float32), base_lr=base, sched_kind=kind, warmup_steps=W, total_steps=T, min_lr_ratio=ratio)
        for t in range(1, 11):
            run.step(g)
            w = run.words()
            want64 = N.lr_at(run.recipe, t)
            want = np.float32(want64)
            assert w["step"] == t
            if kind == "cosine":
                assert abs(float(w["lr"]) - float(want)) <= float(np.spacing(want)), (kind, t, w["lr"], want)
            else:
                assert w["lr"].tobytes() == want.tobytes() and w["lr64"] == want64, (kind, t, w["lr"], want)


# ---------------------------------------------------------------------------------------------------------------- the skip
def test_a_skipped_step_changes_nothing_and_does_not_advance_the_schedule(N, CG):
    C, _ = CG
    offs = _tables(C)["A"]
    n = 2 * C + 8
    offs = np.array([o for o in offs if o < n] + [n])          # table A cut at n = 2C+8: 0, C-4, C, C+8, 2C+8
    groups = list(zip(SCALES, RAND_WD))[:len(offs) - 1]
    rs = np.random.RandomState(9)
    p0 = rs.standard_normal(n).astype(np.float32)
    sched = dict(sched_kind="linear", warmup_steps=2, total_steps=6, min_lr_ratio=0.0)
    run = Run(N, p0, offs, groups, ema0=p0, base_lr=LR, decoupled=True, ema_decay=0.9, skip_nonfinite=True, use_norm=True, **sched)
    grads = [rs.standard_normal(n).astype(np.float32) * 1e-2 for _ in range(3)]
    grads[1][n // 3] = np.nan
    run.step(_dev(grads[0]))
    before, w0 = [_bits(t) for t in run.arrays()], run.words()
    run.step(_dev(grads[1]))
    after, w1 = [_bits(t) for t in run.arrays()], run.words()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and w1["rstate"].tobytes() == w0["rstate"].tobytes()
    assert (w0["step"], w0["skipped"]) == (1, 0) and (w1["step"], w1["skipped"]) == (1, 1)
    run.step(_dev(grads[2]))
    w2 = run.words()
    assert (w2["step"], w2["skipped"], w2["ema_updates"]) == (2, 1, 2)
    assert w2["lr"].tobytes() == np.float32(N.lr_at(run.recipe, 2)).tobytes() == np.float32(LR).tobytes()       # t = 2 = W, not 3
    assert w0["lr"].tobytes() == np.float32(N.lr_at(run.recipe, 1)).tobytes() and run.intact()
    assert not any(np.array_equal(a, b) for a, b in zip(after[:3], [_bits(t) for t in run.arrays()][:3]))


# ---------------------------------------------------------------------------------------------------------------- random operands
def _dist(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())


def _operands(n, steps=5):
    rs = np.random.RandomState(77)
    p0 = rs.standard_normal(n).astype(np.float32)
    return p0, [(s * rs.standard_normal(n)).astype(np.float32) for s in (1e-3, 1e-1, 1e-3, 1e-1, 1e-3)[:steps]]


def _yardstick(N, p0, grads):
    """rlt_grad_norm + rlt_adam_step_guarded (coupled, one group, constant lr, max_norm 1) against its restatement -> distances."""
    n = len(p0)
    p, m, v = _dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device="cuda")
    wsb = N.query("rlt_grad_norm_workspace", n, 0)
    ws = N.byte_buffer(wsb, "cuda")
    pr, mr, vr, rst = p0.astype(np.float64), np.zeros(n), np.zeros(n), R.OptState()
    for g_np in grads:
        g = _dev(g_np)
        N.call("rlt_grad_norm", N.ptr(g), n, None, 0, 1.0, N.ptr(ws), wsb, None, N.ptr(state), N.stream())
        N.call("rlt_adam_step_guarded", N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, N.ptr(state), LR, B1, B2, EPS, WD, 0, N.stream())
        R.grad_norm(g_np, None, 1.0, rst)
        R.adam_step_guarded(pr, g_np, mr, vr, rst, float(np.float32(LR)), B1, B2, EPS, float(np.float32(WD)), False)
    torch.cuda.synchronize()
    return [_dist(x.cpu().numpy(), ref) for x, ref in ((p, pr), (m, mr), (v, vr))], float(np.abs(pr).max())


def _recipe_vs_restatement(N, p0, grads, offs=None, groups=None, ema=False, **fields):
    n = len(p0)
    run = Run(N, p0, offs, groups, ema0=p0 if ema else None, base_lr=LR, beta1=B1, beta2=B2, eps=EPS, weight_decay=WD, use_norm=True,
              ema_decay=0.9 if ema else 0.0, **fields)
    run.max_norm = 1.0
    pr, mr, vr, er = p0.astype(np.float64), np.zeros(n), np.zeros(n), (p0.astype(np.float64) if ema else None)
    st, rst = R.OptState(), RR.RecipeState()
    scale, wd = RR.expand_groups(n, offs, groups, WD)
    for g_np in grads:
        run.step(_dev(g_np))
        R.grad_norm(g_np, None, 1.0, st)
        RR.adam_step_recipe(pr, g_np, mr, vr, er, st, rst, scale, wd, LR, B1, B2, EPS, decoupled=bool(fields.get("decoupled")),
                            ema_decay=0.9 if ema else 0.0, use_norm=True)
    assert run.intact() and run.words()["step"] == len(grads) == st.step and run.words()["clipped"] == st.clipped == 2
    got = [t.cpu().numpy() for t in run.arrays()]
    return got, [pr, mr, vr] + ([er] if ema else [])


def test_random_operands_within_twice_the_guarded_step(N, CG):
    C, _ = CG
    offs = _tables(C)["A"]
    big, small = int(offs[-1]), 2 * C + 8
    p0, grads = _operands(big)
    groups = list(zip(SCALES, RAND_WD))
    cases = {"coupled, one group": (small, {}), "coupled, one group, ema": (small, dict(ema=True)),
             "decoupled, table A": (big, dict(offs=offs, groups=groups, decoupled=True)),
             "decoupled, table A, ema": (big, dict(offs=offs, groups=groups, decoupled=True, ema=True))}
    yard = {n: _yardstick(N, p0[:n], [g[:n] for g in grads]) for n in (small, big)}
    failures = []
    for label, (n, kw) in cases.items():
        got, ref = _recipe_vs_restatement(N, p0[:n], [g[:n] for g in grads], **kw)
        again, _ = _recipe_vs_restatement(N, p0[:n], [g[:n] for g in grads], **kw)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again)), label      # the same bits twice
        (yp, ym, yv), pmax = yard[n]
        for name, a, r, y in zip(("p", "exp_avg", "exp_avg_sq"), got, ref, (yp, ym, yv)):
            d = _dist(a, r)
            print(f"{label:28s} n={n:6d} {name:10s}: recipe {d:.3e}  rlt_adam_step_guarded {y:.3e}  (of the largest magnitude)")
            if not (y > 0 and d <= 2 * y):
                failures.append((label, name, d, y))
        if len(got) == 4:
            err = float(np.abs(got[3].astype(np.float64) - ref[3]).max())
            bound = 2 * yp * pmax + len(grads) * 2.0 ** -22 * pmax
            print(f"{label:28s} n={n:6d} ema       : |error| {err:.3e}  allowance {bound:.3e}")
            if not err <= bound:
                failures.append((label, "ema", err, bound))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- FusedAdam
class _Slots(torch.nn.Module):
    """Five parameter tensors of table A's slot sizes; the gradients are set by hand, no forward."""

    def __init__(self, C, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        for name, k in zip(("body", "norm", "bias", "head", "wide"), (C - 4, 4, 8, C + 4, 3 * C + 12)):
            self.register_parameter(name, torch.nn.Parameter(torch.randn(k, generator=gen)))


RECIPE_OPTS = dict(max_grad_norm=1.0, skip_nonfinite=True, decoupled_weight_decay=True, ema_decay=0.9,
                   param_groups=[("norm", {"weight_decay": 0.0}), ("bias", {"weight_decay": 0.0, "lr_scale": 2.0}), ("head", {"lr_scale": 0.0})])


def _fused(C, seed=1, **opts):
    from rlt_hip.parallel import FlatModel, FusedAdam, LRSchedule
    flat = FlatModel(_Slots(C, seed).cuda())
    if opts.pop("sched", False):
        opts["schedule"] = LRSchedule("cosine", 2, 6, 0.1)
    return flat, FusedAdam(flat, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, **opts)


def _fused_grads(n, steps, nan_step=None):
    rs = np.random.RandomState(12)
    grads = [(s * rs.standard_normal(n)).astype(np.float32) for s in ([1e-3, 1e-1] * steps)[:steps]]
    if nan_step is not None:
        grads[nan_step][n // 2] = np.inf
    return grads


def test_fused_adam_recipe_against_the_restatement_and_ema_weights(N, CG):
    C, _ = CG
    flat, opt = _fused(C, sched=True, **RECIPE_OPTS)
    n = flat.numel
    assert flat.offsets.tolist() == _tables(C)["A"].tolist() and opt.recipe and opt.guarded
    p0 = flat.flat_param.cpu().numpy().copy()
    grads = _fused_grads(n, 6, nan_step=3)
    groups = opt.group_values
    assert groups == [(1.0, WD), (1.0, 0.0), (2.0, 0.0), (0.0, WD), (1.0, WD)]
    pr, mr, vr, er = p0.astype(np.float64), np.zeros(n), np.zeros(n), p0.astype(np.float64)
    st, rst = R.OptState(), RR.RecipeState()
    scale, wd = RR.expand_groups(n, flat.offsets.tolist(), groups)
    sched = dict(kind="cosine", warmup=2, total=6, min_lr_ratio=0.1)
    applied = []
    for g_np in grads:
        flat.flat_grad.copy_(_dev(g_np))
        opt.step()
        R.grad_norm(g_np, None, 1.0, st)
        applied.append(RR.adam_step_recipe(pr, g_np, mr, vr, er, st, rst, scale, wd, LR, B1, B2, EPS, decoupled=True, sched=sched,
                                           ema_decay=0.9, skip_nonfinite=True, use_norm=True))
    assert applied == [True, True, True, False, True, True]
    es = opt.epoch_stats(reset=False)
    assert (es["skipped_steps"], es["clipped_steps"], es["finite_steps"]) == (1, st.clipped, 5)
    assert es["lr"] == float(opt.current_lr()) and opt.current_lr().is_cuda
    assert abs(es["lr"] - opt.lr_at(5)) <= float(np.spacing(np.float32(opt.lr_at(5)))) and opt.state_dict()["steps"] == 5
    (yp, ym, yv), pmax = _yardstick(N, *_operands(n))
    for name, a, r, y in zip(("p", "exp_avg", "exp_avg_sq"), (flat.flat_param, opt.exp_avg, opt.exp_avg_sq), (pr, mr, vr), (yp, ym, yv)):
        d = _dist(a.cpu().numpy(), r)
        print(f"FusedAdam recipe {name:10s}: {d:.3e}  rlt_adam_step_guarded {y:.3e}")
        assert d <= 2 * y, (name, d, y)
    err = float(np.abs(opt.ema.cpu().numpy().astype(np.float64) - er).max())
    assert err <= 2 * yp * pmax + 5 * 2.0 ** -22 * pmax, err
    a, b = int(flat.offsets[3]), int(flat.offsets[4])          # the frozen tensor
    assert np.array_equal(_bits(flat.flat_param[a:b]), p0[a:b].view(np.int32)) and not bool(opt.exp_avg[a:b].any())
    # ema_weights: the bucket holds ema's bits, the module's parameters read them, and both come back exactly
    raw, avg = _bits(flat.flat_param), _bits(opt.ema)
    assert not np.array_equal(raw, avg)
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            assert np.array_equal(_bits(flat.flat_param), avg) and np.array_equal(_bits(opt.ema), raw)
            assert np.array_equal(_bits(flat.model.wide), avg[int(flat.offsets[4]):])
            with pytest.raises(RuntimeError):
                with opt.ema_weights():
                    pass
            with pytest.raises(RuntimeError):
                opt.step()
            1 / 0
    assert np.array_equal(_bits(flat.flat_param), raw) and np.array_equal(_bits(opt.ema), avg)
    with opt.ema_weights():                                     # usable again after the exception
        pass
    assert np.array_equal(_bits(flat.flat_param), raw)


@pytest.mark.parametrize("path", ["plain", "guarded", "recipe"])
def test_state_dict_round_trip_continues_bit_for_bit(N, CG, path):
    C, _ = CG
    opts = {"plain": {}, "guarded": dict(max_grad_norm=1.0, skip_nonfinite=True), "recipe": dict(sched=True, **RECIPE_OPTS)}[path]
    flat_a, opt_a = _fused(C, **dict(opts))
    grads = [_dev(g) for g in _fused_grads(flat_a.numel, 6, nan_step=1 if path != "plain" else None)]
    for g in grads[:3]:
        flat_a.flat_grad.copy_(g)
        opt_a.step()
    flat_b, opt_b = _fused(C, seed=2, **dict(opts))             # other initial weights: everything must come from the state
    flat_b.flat_param.copy_(flat_a.flat_param)
    sd = opt_a.state_dict()
    opt_b.load_state_dict({k: (v.clone().cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})      # as from a checkpoint file
    for g in grads[3:]:
        for flat, opt in ((flat_a, opt_a), (flat_b, opt_b)):
            flat.flat_grad.copy_(g)
            opt.step()
    torch.cuda.synchronize()
    pairs = [(flat_a.flat_param, flat_b.flat_param), (opt_a.exp_avg, opt_b.exp_avg), (opt_a.exp_avg_sq, opt_b.exp_avg_sq)]
    if path == "recipe":
        pairs += [(opt_a.ema, opt_b.ema), (opt_a.recipe_state, opt_b.recipe_state)]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in pairs)
    sa, sb = opt_a.state_dict(), opt_b.state_dict()
    keys = ("steps",) if path == "plain" else ("steps", "clipped_steps", "skipped_steps")
    assert [sa[k] for k in keys] == [sb[k] for k in keys] and sa["steps"] == (6 if path == "plain" else 5)


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_trainer_flags_schedule_adamw_and_ema_eval(tmp_path):
    from dataloader.synth import write_synthetic_robust04
    from rlt_hip.parallel import LRSchedule
    base, out = tmp_path / "data", tmp_path / "run"
    write_synthetic_robust04(str(base), "robust04", "drmm_tks", n_train=11, n_test=5, seq_len=40, seed=3)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO, os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, os.path.join(PKG, "run.py"), "--dataset-base", str(base), "--model-name", "attncut",
                          "--epochs", "2", "--batch-size", "4", "--use-conf", "0", "--seed", "3", "--lr", "1e-3", "--history-json",
                          str(out / "history.json"), "--tensorboard-dir", str(out / "tb"), "--save-path", str(out / "best"),
                          "--lr-schedule", "cosine", "--warmup-steps", "2", "--adamw", "1", "--ema-decay", "0.9", "--ema-eval", "1"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    hist = json.load(open(out / "history.json"))["history"]
    sched = LRSchedule("cosine", 2, 6, 0.0)                     # 11 lists in batches of 4: 3 steps per epoch, 6 in all
    assert len(hist) == 2
    for e, h in enumerate(hist):
        assert h["lr"] == float(np.float32(sched.lr_at(3 * (e + 1), 1e-3))) or \
            abs(h["lr"] - sched.lr_at(3 * (e + 1), 1e-3)) <= float(np.spacing(np.float32(h["lr"])))
        assert all(np.isfinite(x) for x in h["train"] + h["test"])
