"""tests/recipe_restate.py pinned to torch in float64 at 1e-12: torch.optim.Adam and torch.optim.AdamW with per-group lr and
weight_decay, the warm-up against LinearLR, the cosine branch against CosineAnnealingLR, the moving average against a plain loop,
and the skip.  Every float32-held constant of the restatement (lr, lr * lr_scale, weight decay, EMA decay) is given a value that
float32 holds exactly, so that its roundings are no-ops here and float64 torch computes from the same numbers."""
import numpy as np
import pytest
import torch

import opt_restate as R
import recipe_restate as RR

TOL = 1e-12
B1, B2, EPS = 0.9, 0.999, 1e-8
OFFS = [0, 12, 20, 52]
GROUPS = [(1.0, 2.0 ** -8), (0.5, 0.0), (2.0, 2.0 ** -6)]          # (lr_scale, weight_decay) per segment


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= TOL * max(np.abs(b).max(), 1e-300)


def _torch_lr(sched_cls, base, steps, **kw):
    """lr of steps 1..steps under a torch scheduler stepped once after every optimizer step (lr of step 1 = its initial value)."""
    w = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([w], lr=base)
    sched = sched_cls(opt, **kw)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("decoupled", [False, True])
def test_update_is_torch_adam_and_adamw_with_param_groups(decoupled):
    rs = np.random.RandomState(5)
    n, base = OFFS[-1], 2.0 ** -7
    p0 = rs.standard_normal(n)
    grads = [rs.standard_normal(n) * 0.1 for _ in range(5)]
    tp = [torch.tensor(p0[a:b], dtype=torch.float64, requires_grad=True) for a, b in zip(OFFS, OFFS[1:])]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": [t], "lr": base * s, "weight_decay": w} for t, (s, w) in zip(tp, GROUPS)], betas=(B1, B2), eps=EPS)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    scale, wd = RR.expand_groups(n, OFFS, GROUPS)
    st, rst = R.OptState(), RR.RecipeState()
    for g in grads:
        for t, (a, b) in zip(tp, zip(OFFS, OFFS[1:])):
            t.grad = torch.tensor(g[a:b], dtype=torch.float64)
        opt.step()
        assert RR.adam_step_recipe(p, g, m, v, None, st, rst, scale, wd, base, B1, B2, EPS, decoupled=decoupled)
        assert _close(p, torch.cat([t.detach() for t in tp]).numpy())
        assert _close(m, torch.cat([opt.state[t]["exp_avg"] for t in tp]).numpy())
        assert _close(v, torch.cat([opt.state[t]["exp_avg_sq"] for t in tp]).numpy())
    assert st.step == 5 and float(rst.lr) == base


def test_one_group_with_clipping_is_the_guarded_restatement():
    rs = np.random.RandomState(6)
    n = 40
    p0, g = rs.standard_normal(n), rs.standard_normal(n)
    pa, ma, va = p0.copy(), np.zeros(n), np.zeros(n)
    pb, mb, vb = p0.copy(), np.zeros(n), np.zeros(n)
    sa, _ = R.grad_norm(g.astype(np.float32), None, 1.0)
    sb, _ = R.grad_norm(g.astype(np.float32), None, 1.0)
    assert sa.coef < 1.0
    R.adam_step_guarded(pa, g, ma, va, sa, float(np.float32(1e-2)), B1, B2, EPS, float(np.float32(0.005)), False)
    scale, wd = RR.expand_groups(n, weight_decay=0.005)
    RR.adam_step_recipe(pb, g, mb, vb, None, sb, RR.RecipeState(), scale, wd, 1e-2, B1, B2, EPS, use_norm=True)
    assert _close(pb, pa) and _close(mb, ma) and _close(vb, va) and sb.clipped == 1


def test_frozen_segment_is_untouched():
    rs = np.random.RandomState(7)
    n = OFFS[-1]
    p0, g = rs.standard_normal(n), rs.standard_normal(n)
    p, m, v, ema = p0.copy(), np.zeros(n), np.zeros(n), p0.copy()
    scale, wd = RR.expand_groups(n, OFFS, [(1.0, 0.25), (0.0, 0.25), (1.0, 0.0)])
    RR.adam_step_recipe(p, g, m, v, ema, R.OptState(), RR.RecipeState(), scale, wd, 0.125, B1, B2, EPS, decoupled=True, ema_decay=0.5)
    a, b = OFFS[1], OFFS[2]
    assert np.array_equal(p[a:b], p0[a:b]) and not m[a:b].any() and not v[a:b].any() and np.array_equal(ema[a:b], p0[a:b])
    assert (p[:a] != p0[:a]).all() and m[:a].all() and (ema[b:] != p0[b:]).all()


@pytest.mark.parametrize("W", [3, 7])
def test_warmup_is_torch_linear_lr(W):
    base = 2.0 ** -5
    want = _torch_lr(torch.optim.lr_scheduler.LinearLR, base, W, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1)
    for kind in (RR.CONSTANT, RR.LINEAR, RR.COSINE):
        got = [RR.lr_at(t, base, kind, W, W + 5, 0.25) for t in range(1, W + 1)]
        assert _close(got, want), kind
        assert got[-1] == base


@pytest.mark.parametrize("W,T", [(3, 8), (0, 8), (2, 50)])
def test_cosine_is_torch_cosine_annealing(W, T):
    base, ratio = 2.0 ** -5, 0.25
    floor = base * ratio
    want = _torch_lr(torch.optim.lr_scheduler.CosineAnnealingLR, base, T - W + 1, T_max=T - W, eta_min=floor)     # e = 0 .. T - W
    closed = [floor + (base - floor) * (1.0 + np.cos(np.pi * e / (T - W))) / 2.0 for e in range(T - W + 1)]
    got = [RR.lr_at(W + e, base, RR.COSINE, W, T, ratio) for e in range(1, T - W + 1)]
    assert _close(got, want[1:]) and _close(got, closed[1:])
    assert abs(got[-1] - floor) <= TOL * floor and RR.lr_at(T + 1, base, RR.COSINE, W, T, ratio) == floor == RR.lr_at(T + 9, base, RR.LINEAR, W, T, ratio)


def test_linear_and_constant_branches():
    base, ratio, W, T = 2.0 ** -5, 0.25, 3, 8
    floor = base * ratio
    want = _torch_lr(torch.optim.lr_scheduler.LinearLR, base, T - W + 1, start_factor=1.0, end_factor=ratio, total_iters=T - W)
    got = [RR.lr_at(W + e, base, RR.LINEAR, W, T, ratio) for e in range(1, T - W + 1)]
    assert _close(got, want[1:]) and got[-1] == floor
    assert all(RR.lr_at(t, base, RR.CONSTANT, W, T, ratio) == base for t in range(W, T + 5))
    assert RR.lr_at(1, 0.1, RR.CONSTANT) == float(np.float32(0.1))          # the float argument of the C ABI


def test_ema_is_the_plain_loop_and_its_warmup():
    rs = np.random.RandomState(8)
    n = 16
    p0 = rs.standard_normal(n)
    grads = [rs.standard_normal(n) for _ in range(4)]
    scale, wd = RR.expand_groups(n)
    for warm in (False, True):
        p, m, v, ema = p0.copy(), np.zeros(n), np.zeros(n), p0.copy()
        q, mq, vq, loop = p0.copy(), np.zeros(n), np.zeros(n), p0.copy()
        st, rst, sq = R.OptState(), RR.RecipeState(), R.OptState()
        for k, g in enumerate(grads):
            RR.adam_step_recipe(p, g, m, v, ema, st, rst, scale, wd, 0.125, B1, B2, EPS, ema_decay=0.75, ema_warmup=warm)
            RR.adam_step_recipe(q, g, mq, vq, None, sq, RR.RecipeState(), scale, wd, 0.125, B1, B2, EPS)
            d = float(np.float32(min(0.75, (1 + k) / (10 + k)))) if warm else 0.75
            for i in range(n):
                loop[i] = d * loop[i] + (1 - d) * q[i]
            assert _close(ema, loop) and float(rst.ema_decay) == d and rst.ema_updates == k + 1
    assert [float(RR.ema_decay_at(k, 0.5, True)) for k in (0, 1, 2, 3)] == [float(np.float32(x)) for x in (0.1, 2 / 11, 0.25, 4 / 13)]
    assert float(RR.ema_decay_at(10 ** 6, 0.5, True)) == 0.5


def test_skip_changes_nothing_and_the_schedule_counts_applied_steps():
    n = 8
    g_bad = np.ones(n, dtype=np.float32)
    g_bad[3] = np.nan
    p, m, v, ema = np.ones(n), np.zeros(n), np.zeros(n), np.ones(n)
    st, rst = R.OptState(), RR.RecipeState()
    scale, wd = RR.expand_groups(n)
    sched = dict(kind=RR.LINEAR, warmup=2, total=6, min_lr_ratio=0.0)
    kw = dict(sched=sched, ema_decay=0.5, skip_nonfinite=True, use_norm=True)
    R.grad_norm(np.ones(n, dtype=np.float32), None, None, st)
    assert RR.adam_step_recipe(p, np.ones(n), m, v, ema, st, rst, scale, wd, 0.125, B1, B2, EPS, **kw)
    before = (p.copy(), m.copy(), v.copy(), ema.copy(), dict(vars(rst)))
    R.grad_norm(g_bad, None, None, st)
    assert not RR.adam_step_recipe(p, g_bad, m, v, ema, st, rst, scale, wd, 0.125, B1, B2, EPS, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(before[:4], (p, m, v, ema))) and dict(vars(rst)) == before[4]
    assert (st.step, st.skipped) == (1, 1)
    R.grad_norm(np.ones(n, dtype=np.float32), None, None, st)
    assert RR.adam_step_recipe(p, np.ones(n), m, v, ema, st, rst, scale, wd, 0.125, B1, B2, EPS, **kw)
    assert st.step == 2 and rst.lr64 == RR.lr_at(2, 0.125, **sched) == 0.125
