"""Float64 numpy restatement of the recipe step (include/rlt_hip.h: rlt_adam_step_recipe, rlt_lr_at): the learning-rate schedule,
per-segment parameter groups, coupled and decoupled weight decay, the moving average of the parameters and the non-finite skip.

Nothing here knows how the kernel cuts the bucket into chunks or walks the segment table: the groups are expanded to one value per
element and the update is torch.optim.Adam's / AdamW's formula written out.  Where the kernel holds a float32 constant the
restatement holds the same float32 value (lr rounded once from the float64 schedule, lr * lr_scale, the group's weight decay, the
clip coefficient, the EMA decay); every operation on them is float64.  tests/test_recipe_restate.py pins it to torch in float64;
tests/test_recipe_gpu.py holds the kernel to it."""
import math

import numpy as np

import opt_restate as R

CONSTANT, LINEAR, COSINE = "constant", "linear", "cosine"
f32 = np.float32


def lr_at(t, base_lr, kind=CONSTANT, warmup=0, total=0, min_lr_ratio=0.0):
    """The schedule's float64 value at applied step t >= 1, in the operation order the header states; base_lr and min_lr_ratio
    are float arguments of the C ABI: their float32 values enter."""
    B = np.float64(f32(base_lr))
    F = B * np.float64(f32(min_lr_ratio))
    W, T = int(warmup), int(total)
    if t <= W:
        return float(B * np.float64(t) / np.float64(W))
    if kind == CONSTANT:
        return float(B)
    if t > T:
        return float(F)
    if kind == LINEAR:
        return float(F + (B - F) * np.float64(T - t) / np.float64(T - W))
    return float(F + (B - F) * 0.5 * (1.0 + np.cos(np.float64(math.pi) * np.float64(t - W) / np.float64(T - W))))


def ema_decay_at(k, ema_decay, warmup):
    """The decay of the EMA update after k earlier ones, as the float32 value the kernel uses."""
    d = np.float64(f32(ema_decay))
    if warmup:
        d = min(d, (1.0 + k) / (10.0 + k))
    return f32(d)


def expand_groups(n, offsets=None, groups=None, weight_decay=0.0):
    """(lr_scale, weight_decay) per element, float64 arrays holding the groups' float32 values."""
    if offsets is None:
        return np.ones(n), np.full(n, np.float64(f32(weight_decay)))
    scale, wd = np.empty(n), np.empty(n)
    for (a, b), (s, w) in zip(zip(offsets, offsets[1:]), groups):
        scale[int(a):int(b)] = np.float64(f32(s))
        wd[int(a):int(b)] = np.float64(f32(w))
    return scale, wd


class RecipeState:
    """The members of rlt_recipe_state."""

    def __init__(self):
        self.lr64, self.lr, self.ema_updates, self.ema_decay, self.coef = 0.0, f32(0), 0, f32(0), f32(0)


def adam_step_recipe(p, g, m, v, ema, state, rstate, scale, wd, base_lr, beta1, beta2, eps, decoupled=False, sched=None,
                     ema_decay=0.0, ema_warmup=True, skip_nonfinite=False, use_norm=False):
    """In place on the float64 arrays p, m, v and ema (None without an average); g is read only.  state: opt_restate.OptState (after
    opt_restate.grad_norm when use_norm); scale, wd: expand_groups; sched: the keyword arguments of lr_at beside t and base_lr.
    Returns True when the step was applied."""
    coef = f32(1.0)
    if use_norm:
        if skip_nonfinite and state.nonfinite:
            state.skipped += 1
            return False
        coef = f32(state.coef)
    state.step += 1
    t = state.step
    if coef < 1.0:
        state.clipped += 1
    rstate.lr64 = lr_at(t, base_lr, **(sched or {}))
    rstate.lr = f32(rstate.lr64)
    rstate.coef = coef
    live = scale != 0                                          # frozen segments: nothing is written
    with np.errstate(all="ignore"):
        lr_s = (np.float64(rstate.lr) * scale).astype(np.float32).astype(np.float64)
        gr = np.asarray(g, dtype=np.float64) * np.float64(coef)
        if not decoupled:
            gr = gr + wd * p
        m_new = beta1 * m + (1.0 - beta1) * gr
        v_new = beta2 * v + (1.0 - beta2) * gr * gr
        bc1 = 1.0 - beta1 ** t
        bc2_sqrt = np.sqrt(1.0 - beta2 ** t)
        p_new = p * (1.0 - lr_s * wd) if decoupled else p      # torch.optim.AdamW: the decay first, on the old parameter
        p_new = p_new - (lr_s / bc1) * (m_new / (np.sqrt(v_new) / bc2_sqrt + eps))
        m[live], v[live], p[live] = m_new[live], v_new[live], p_new[live]
        if ema is not None:
            d = ema_decay_at(rstate.ema_updates, ema_decay, ema_warmup)
            rstate.ema_decay, rstate.ema_updates = d, rstate.ema_updates + 1
            d = np.float64(d)
            ema[live] = (d * ema + (1.0 - d) * p)[live]
    return True

