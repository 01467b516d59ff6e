"""Pin tests/wass_restate.py (the float64 Sinkhorn restatement the device tests of csrc/wass.hip compare against) and check,
where no GPU is needed, the conditions that make those device tests mean something.  CPU only.

- In float32 at the default threshold the restatement is the oracle (oracle/losses.py: WassDistLoss) on every golden case.
- Its autograd gradient equals the explicit reverse sweep of csrc/wass.hip's header comment, in float64.
- Case-table conditions, per row of wass_restate.CASES, in float64: the stop sums drop by at least 1.5x at the chosen K, the
  chosen threshold lies strictly between e_K and e_{K-1}, and one iteration fewer or more changes the loss or dp by more than
  10x the tolerance the device gets for that measure - a device that stops at the wrong iteration cannot pass.  A case that
  fails is given another seed (wass_restate.SEED_OFFSET), not exempted.
  The rows with B = 1 or S = 1 cannot meet the last two: their cost C_ij does not depend on i, exp(-C / eps) has rank one, the
  first iteration lands on the fixed point and e_2 is zero up to float64 rounding, whatever the seed.  The table needs them for
  their kernel edges (single-term LSE, S = 1), so what is asserted for them is exactly that: 1, K, K + 1 and 100 iterations
  give the same loss and dp to 1e-9, so no stop iteration of the device can be told from another."""
import numpy as np
import pytest
import torch

import golden_util as gu
import wass_restate as wr
from oracle import losses as ol

torch.set_num_threads(8)
ROUND_OFF = 4 * 2.0 ** -24


def test_float32_restatement_is_the_oracle_on_the_golden_cases():
    gold = gu.load("wassdist")
    tags = sorted({k.split("/")[0] for k in gold})
    assert tags
    for tag in tags:
        eps, y = float(gold[f"{tag}/eps"]), torch.from_numpy(gold[f"{tag}/y"])
        p = torch.softmax(torch.from_numpy(gold[f"{tag}/logits"]), dim=1)
        q = p.clone().unsqueeze(2).requires_grad_(True)
        want = ol.WassDistLoss(eps=eps, max_iter=100)(q, y)
        want.backward()
        loss, dp, K, errs = wr.sinkhorn(p, y, eps, max_iter=100, thresh=0.1, dtype=torch.float32)
        assert 1 <= K <= 100 and (K == 100 or errs[-1] < 0.1)
        e_loss, e_dp, _ = wr.errors(loss, dp, float(want.item()), q.grad.squeeze(2).double().numpy())
        assert e_loss <= ROUND_OFF and e_dp <= ROUND_OFF, (tag, e_loss, e_dp)


def test_force_iters_ignores_the_threshold():
    p, y = wr.make_inputs(5, 9, 1.0, 3)
    _, _, K, errs = wr.sinkhorn(p, y, 1e-1, thresh=1e30, force_iters=4)
    assert K == 4 and len(errs) == 4
    _, _, K, _ = wr.sinkhorn(p, y, 1e-1, thresh=1e30)
    assert K == 1


@pytest.mark.parametrize("name", list(wr.CASES) + ["exhaust_" + n for n in wr.EXHAUST])
def test_autograd_equals_the_explicit_reverse_sweep(name):
    c = wr.prepare_exhaust(name[8:]) if name.startswith("exhaust_") else wr.prepare(name)
    loss, dp = wr.sweep(c["p"].numpy(), c["y"].numpy(), c["eps"], c["K"])
    assert abs(loss - c["loss64"]) <= 1e-10 * max(1.0, abs(c["loss64"]))
    assert np.abs(dp - c["dp64"]).max() <= 1e-10 * np.abs(c["dp64"]).max()


def _changes(c, iters):
    loss, dp, _, _ = wr.sinkhorn(c["p"], c["y"], c["eps"], force_iters=iters)
    return wr.errors(loss, dp, c["loss64"], c["dp64"])


def _stop_is_observable(c):
    for iters in (c["K"] - 1, c["K"] + 1):
        e_loss, e_dp, _ = _changes(c, iters)
        assert e_loss > 10 * c["tol"][0] or e_dp > 10 * c["tol"][1], (iters, e_loss, e_dp, c["tol"])


@pytest.mark.parametrize("name", list(wr.CASES))
def test_case_table_conditions(name):
    c = wr.prepare(name)
    K, errs = c["K"], c["errs"]
    assert len(errs) == wr.MAX_ITER and 2 <= K <= wr.MAX_ITER
    assert errs[K - 2] >= wr.MIN_RATIO * errs[K - 1]
    assert np.isfinite(c["dp64"]).all() and np.abs(c["dp64"]).max() > 0
    if B_or_S_one := wr.degenerate(c["B"], c["S"]):
        assert errs[K - 1] <= 1e-12 * errs[0]
        for iters in (1, K + 1, wr.MAX_ITER):
            assert max(_changes(c, iters)) <= 1e-9, (iters, _changes(c, iters))
    assert B_or_S_one == (c["B"] == 1 or c["S"] == 1)
    if not B_or_S_one:
        assert errs[K - 1] < c["thresh"] < errs[K - 2]
        _stop_is_observable(c)


@pytest.mark.parametrize("name", list(wr.DEFAULT_CASES))
def test_default_threshold_cases_straddle_it(name):
    c = wr.prepare_default(name)
    K, errs = c["K"], c["errs"]
    assert 2 <= K < wr.MAX_ITER and len(errs) == K
    assert errs[K - 1] * wr.MIN_RATIO <= wr.DEFAULT_THRESH and errs[K - 2] >= wr.MIN_RATIO * wr.DEFAULT_THRESH
    assert all(e >= wr.MIN_RATIO * wr.DEFAULT_THRESH for e in errs[:K - 1])
    _stop_is_observable(c)


def test_case_table_is_the_one_the_kernels_need():
    shapes = {(c[0], c[1]) for c in wr.CASES.values()}
    assert shapes == {(1, 40), (2, 40), (3, 40), (63, 40), (64, 40), (65, 40), (255, 7), (256, 7), (257, 7), (65, 1), (65, 300)}
    assert len(wr.CASES) == 4 * len(shapes)
    for name, (B, S, eps, scale) in wr.CASES.items():
        assert eps in (1e-1, 1e-3) and scale in (1.0, 6.0)
        p, y = wr.make_inputs(B, S, scale, wr.case_seed(name))
        assert p.dtype == torch.float32 and tuple(p.shape) == tuple(y.shape) == (B, S)
        assert torch.allclose(p.sum(1), torch.ones(B), atol=1e-5) and set(y.unique().tolist()) <= {0.0, 1.0}
        if B >= 2:
            assert not y[0].any()
        if B >= 3:
            assert y[B - 1].all()
