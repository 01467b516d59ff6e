"""tests/hazard_restate.py against a torch float64 autograd composition (logsigmoid, cumsum, exp), forward and backward, at 1e-12
- and the properties the hazard head is built for: p sums to 1, the uniform prior gives 1/S, the last logit gets no gradient.
No GPU, no library."""
import numpy as np
import pytest
import torch

import hazard_restate as H

SHAPES = [(1, 1), (3, 2), (4, 5), (5, 63), (3, 64), (2, 65), (2, 300), (1, 1024)]


def torch_composition(z, dp, dstop):
    zt = torch.from_numpy(z).clone().requires_grad_(True)
    S = z.shape[1]
    F = torch.nn.functional
    head = zt[:, :S - 1]
    log_keep = F.logsigmoid(-head)                                       # log(1 - h)
    L = torch.cat([torch.zeros(z.shape[0], 1, dtype=torch.float64), torch.cumsum(log_keep, 1)], 1)      # L_s, s = 0..S-1
    p = torch.exp(torch.cat([F.logsigmoid(head), torch.zeros(z.shape[0], 1, dtype=torch.float64)], 1) + L)
    stop = torch.cat([torch.sigmoid(head), torch.ones(z.shape[0], 1, dtype=torch.float64)], 1)
    ((p * torch.from_numpy(dp)).sum() + (stop * torch.from_numpy(dstop)).sum()).backward()
    return p.detach().numpy(), stop.detach().numpy(), zt.grad.numpy()


@pytest.mark.parametrize("B,S", SHAPES, ids=lambda v: str(v))
def test_restatement_matches_torch_float64(B, S):
    g = np.random.default_rng(100 * B + S)
    z = 2.0 * g.standard_normal((B, S)) + H.prior_offset(S)
    dp, dstop = g.standard_normal((B, S)), g.standard_normal((B, S))
    p_t, stop_t, dz_t = torch_composition(z, dp, dstop)
    p, stop = H.forward(z)
    assert np.abs(p - p_t).max() <= 1e-12 and np.abs(stop - stop_t).max() <= 1e-12
    assert np.abs(H.backward(z, dp, dstop) - dz_t).max() <= 1e-12
    zero = np.zeros_like(dstop)
    assert np.abs(H.backward(z, dp) - torch_composition(z, dp, zero)[2]).max() <= 1e-12
    assert np.abs(p.sum(1) - 1.0).max() <= 1e-15 * S
    assert (H.backward(z, dp, dstop)[:, S - 1] == 0.0).all() and (dz_t[:, S - 1] == 0.0).all()


@pytest.mark.parametrize("S", [1, 2, 3, 40, 65, 300, 1024])
def test_uniform_prior_gives_one_over_s(S):
    p, stop = H.forward(H.prior_offset(S)[None, :])
    assert np.abs(p - 1.0 / S).max() <= 1e-15 * S * (1.0 / S) + 1e-16 * S
    assert np.abs(stop[0] - 1.0 / np.arange(S, 0, -1)).max() <= 1e-15
    assert abs(p.sum() - 1.0) <= 1e-15 * S


def test_saturated_logits_stay_finite():
    z = np.array([[100.0, -100.0, 40.0, -40.0, 0.0], [-100.0] * 5, [100.0] * 5, [-745.0, 800.0, -800.0, 0.0, 0.0]])
    dp = np.ones_like(z)
    p, stop = H.forward(z)
    assert np.isfinite(p).all() and np.isfinite(stop).all() and np.isfinite(H.backward(z, dp, dp)).all()
    assert np.abs(p.sum(1) - 1.0).max() <= 1e-14
    assert p[1, 4] == pytest.approx(1.0, abs=1e-40) and p[2, 0] == 1.0 and p[2, 1] < 1e-43
