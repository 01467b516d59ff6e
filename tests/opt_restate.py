"""Float64 numpy restatement of the guarded optimizer step (include/rlt_hip.h: rlt_grad_norm, rlt_adam_step_guarded).

Nothing here knows how the kernels order their sums or cut the bucket into chunks: the figures are plain numpy reductions in
float64, the update is torch.optim.Adam's formula written out.  tests/test_opt_restate.py pins it to
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64; tests/test_opt_gpu.py holds the kernels to it."""
import numpy as np


def figures(x):
    """(float64 sum of squares over the finite elements, non-finite count, NaN count, max |x| over the finite elements)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    fin = np.isfinite(x)
    xf = x[fin]
    return (float(np.sum(xf * xf)), int(x.size - xf.size), int(np.isnan(x).sum()), float(np.abs(xf).max()) if xf.size else 0.0)


def clip_coef(norm, max_norm, dtype=np.float32):
    """torch's rule: min(1, max_norm / (norm + 1e-6)) in float64 (a NaN stays a NaN), rounded once to `dtype`; max_norm None,
    <= 0 or +inf: exactly 1.  max_norm is a float argument of the C ABI: its float32 value enters the quotient."""
    if max_norm is None or not max_norm > 0 or np.isinf(max_norm):
        return dtype(1.0)
    with np.errstate(all="ignore"):
        q = np.float64(np.float32(max_norm)) / (np.float64(norm) + 1e-6)
    return dtype(q if np.isnan(q) else min(q, 1.0))


class OptState:
    """The members of rlt_opt_state that outlive a call."""

    def __init__(self):
        self.step = self.skipped = self.clipped = 0
        self.nonfinite = self.nan_count = 0
        self.sumsq = self.norm = self.max_abs = 0.0
        self.norm_sum = self.norm_max = 0.0
        self.norm_steps = 0
        self.coef = np.float32(1.0)


def grad_norm(g, offsets=None, max_norm=None, state=None, coef_dtype=np.float32):
    """-> (state, segs): segs = one (sumsq, nonfinite, max_abs) per segment [offsets[s], offsets[s+1]) (None without offsets);
    the bucket's figures are the sum of the segments' (here: of the whole bucket - the same set of elements)."""
    g = np.asarray(g).ravel()
    st = state if state is not None else OptState()
    segs = None
    if offsets is not None:
        offsets = [int(o) for o in offsets]
        assert offsets[0] == 0 and offsets[-1] == g.size and all(a <= b and a % 4 == 0 for a, b in zip(offsets, offsets[1:]))
        segs = []
        for a, b in zip(offsets, offsets[1:]):
            ss, nf, _, mx = figures(g[a:b])
            segs.append((ss, nf, mx))
    st.sumsq, st.nonfinite, st.nan_count, st.max_abs = figures(g)
    st.norm = float("nan") if st.nan_count else (float("inf") if st.nonfinite else float(np.sqrt(st.sumsq)))
    st.coef = clip_coef(st.norm, max_norm, coef_dtype)
    if st.nonfinite == 0:
        st.norm_sum += st.norm
        st.norm_max = max(st.norm_max, st.norm)
        st.norm_steps += 1
    return st, segs


def adam_step_guarded(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, skip_nonfinite):
    """In place on the float64 arrays p, m, v; g is read only.  Returns True when the step was applied."""
    if skip_nonfinite and state.nonfinite:
        state.skipped += 1
        return False
    state.step += 1
    t = state.step
    if state.coef < 1.0:
        state.clipped += 1
    with np.errstate(all="ignore"):
        gr = np.asarray(g, dtype=np.float64) * np.float64(state.coef)
        if weight_decay != 0:
            gr = gr + weight_decay * p
        m[:] = beta1 * m + (1.0 - beta1) * gr
        v[:] = beta2 * v + (1.0 - beta2) * gr * gr
        bc1 = 1.0 - beta1 ** t
        bc2_sqrt = np.sqrt(1.0 - beta2 ** t)
        p[:] = p - (lr / bc1) * (m / (np.sqrt(v) / bc2_sqrt + eps))
    return True
