"""tests/opt_restate.py - the float64 restatement the guarded optimizer step is tested against - pinned on the CPU to
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(weight_decay=...) run in float64: 6 steps on 3 tensors of 4, 12 and 1028
elements, parameters and both moments within 1e-12 of the largest magnitude of each array (the bound tests/test_lstm_restate.py
uses for the same kind of pin).  torch keeps the clip coefficient in float64; the restatement rounds it to float once as the
kernel does, so the pin asks it for the unrounded coefficient (coef_dtype=np.float64) - that rounding is the only difference."""
import numpy as np
import torch

import opt_restate as R

SIZES = (4, 12, 1028)
LR, B1, B2, EPS, WD, MAX_NORM = 1e-2, 0.9, 0.999, 1e-8, 0.005, 1.0
# the gradient scale per step: norms of about 0.3 * sqrt(1044) ~ 10 (clipped) and 0.01 * 32 ~ 0.3 (not clipped)
SCALES = (0.3, 0.01, 0.3, 0.01, 0.3, 0.01)
TOL = 1e-12


def _inputs(seed=5):
    rs = np.random.RandomState(seed)
    params = [rs.standard_normal(n) for n in SIZES]
    grads = [[s * rs.standard_normal(n) for n in SIZES] for s in SCALES]
    return params, grads


def _flat(arrays):
    return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays])


def _torch_loop(params, grads, nan_step=None, skip=False):
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in params]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    norms = []
    for i, gs in enumerate(grads):
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        if i == nan_step:
            ps[2].grad[7] = float("nan")
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)))
        if not (skip and i == nan_step):
            opt.step()
    st = [opt.state[p] for p in ps]
    return (_flat(p.detach().numpy() for p in ps), _flat(s["exp_avg"].numpy() for s in st),
            _flat(s["exp_avg_sq"].numpy() for s in st), norms)


def _restated_loop(params, grads, nan_step=None, skip=False):
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    p, m, v = _flat(params), np.zeros(offs[-1]), np.zeros(offs[-1])
    st, norms, segs_last = R.OptState(), [], None
    for i, gs in enumerate(grads):
        g = _flat(gs)
        if i == nan_step:
            g[offs[2] + 7] = np.nan
        st, segs_last = R.grad_norm(g, offs, MAX_NORM, st, coef_dtype=np.float64)
        norms.append(st.norm)
        R.adam_step_guarded(p, g, m, v, st, LR, B1, B2, EPS, WD, skip)
    return p, m, v, norms, st, segs_last


def _close(a, b):
    return np.abs(a - b).max() <= TOL * np.abs(b).max()


def test_restatement_matches_clip_grad_norm_and_adam_in_float64():
    params, grads = _inputs()
    tp, tm, tv, tnorms = _torch_loop(params, grads)
    p, m, v, norms, st, segs = _restated_loop(params, grads)
    assert [n > MAX_NORM for n in tnorms] == [True, False] * 3           # steps that clip and steps that do not
    np.testing.assert_allclose(norms, tnorms, rtol=1e-14)
    assert _close(p, tp) and _close(m, tm) and _close(v, tv)
    assert (st.step, st.clipped, st.skipped, st.norm_steps) == (6, 3, 0, 6)
    assert abs(st.norm_sum - sum(tnorms)) <= 1e-13 * sum(tnorms) and st.norm_max == max(norms)
    # the segment figures are those of the last gradient's three tensors, and they add up to the bucket's
    last = grads[-1]
    for (ss, nf, mx), g in zip(segs, last):
        assert ss == float(np.sum(g * g)) and nf == 0 and mx == float(np.abs(g).max())
    assert abs(sum(s[0] for s in segs) - st.sumsq) <= 1e-15 * st.sumsq


def test_skip_rule_is_the_torch_loop_without_that_step():
    params, grads = _inputs(seed=6)
    tp, tm, tv, _ = _torch_loop(params, grads, nan_step=2, skip=True)
    p, m, v, norms, st, segs = _restated_loop(params, grads, nan_step=2, skip=True)
    assert np.isnan(norms[2]) and np.isfinite(np.delete(norms, 2)).all()
    assert _close(p, tp) and _close(m, tm) and _close(v, tv)            # bias corrections of steps 4..6 use t = 3..5
    assert (st.step, st.skipped, st.clipped, st.norm_steps) == (5, 1, 2, 5)


def test_without_the_skip_a_nan_poisons_everything_as_in_torch():
    params, grads = _inputs(seed=7)
    tp, tm, tv, _ = _torch_loop(params, grads, nan_step=2, skip=False)
    p, m, v, _, st, _ = _restated_loop(params, grads, nan_step=2, skip=False)
    for a, b in ((p, tp), (m, tm), (v, tv)):
        assert np.isnan(b).all() and np.isnan(a).all()                  # clip_grad_norm_ scales every gradient by a NaN coefficient
    assert (st.step, st.skipped) == (6, 0)


def test_figures_cover_finite_elements_only_and_the_coefficient_rule():
    g = np.array([3.0, -4.0, np.nan, np.inf, -np.inf, 0.5, 0.0, -12.0], dtype=np.float32)
    assert R.figures(g) == (9.0 + 16.0 + 0.25 + 144.0, 3, 1, 12.0)
    st, segs = R.grad_norm(g, [0, 4, 8], 1.0)
    assert segs == [(25.0, 2, 4.0), (144.25, 1, 12.0)] and np.isnan(st.norm) and np.isnan(st.coef) and st.norm_steps == 0
    st, _ = R.grad_norm(np.where(np.isnan(g), 0, g), None, 1.0)
    assert st.norm == np.inf and st.coef == 0.0
    for off in (None, 0, -1.0, np.inf):
        assert R.clip_coef(50.0, off).tobytes() == np.float32(1.0).tobytes()
    assert R.clip_coef(0.5, 1.0) == np.float32(1.0) and R.clip_coef(4.0, 1.0) == np.float32(1.0 / (4.0 + 1e-6))
    assert R.clip_coef(4.0, 1.0).dtype == np.float32
