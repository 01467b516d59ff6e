"""tests/lstm_restate.py - the float64 reference of tests/test_lstm_dispatch_gpu.py - pinned to float64 torch.nn.LSTM(I, 128,
bidirectional=True): the hidden states, and the gradient with respect to the pre-activations through autograd.

nn.LSTM does not expose its pre-activations A = x W_ih^T + b_ih + b_hh + h_{t-1} W_hh^T, so autograd yields dL/dA through its
images: db = sum_t dA_t, dW_ih = sum_t dA_t^T x_t, dW_hh = sum_t dA_t^T h_{t-1}, dx_t = dA_t W_ih.  Per direction these are
C^T dA with C = [1 | x | h_prev] of shape (S*B, 1 + I + 128); the test asserts that C has full row rank at its shapes, so the
images determine dA, and compares every one of them.  No GPU."""
import numpy as np
import pytest
import torch

import lstm_restate as R

TOL = 1e-12


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.mark.parametrize("B,S,I", [(3, 5, 3), (2, 1, 1)], ids=["b3_s5_i3", "b2_s1_i1"])
def test_restatement_equals_float64_nn_lstm(B, S, I):
    torch.manual_seed(100 * B + 10 * S + I)
    lstm = torch.nn.LSTM(I, R.HID, bidirectional=True).double()
    x = torch.randn(S, B, I, dtype=torch.float64, requires_grad=True)
    d_hout = torch.randn(S, B, 2 * R.HID, dtype=torch.float64)
    y, _ = lstm(x)
    y.backward(d_hout)

    sfx = ("", "_reverse")
    w_ih = [getattr(lstm, "weight_ih_l0" + s) for s in sfx]
    w_hh = [getattr(lstm, "weight_hh_l0" + s) for s in sfx]
    b_ih = [getattr(lstm, "bias_ih_l0" + s) for s in sfx]
    b_hh = [getattr(lstm, "bias_hh_l0" + s) for s in sfx]
    with torch.no_grad():
        xf = x.reshape(S * B, I)
        pre = R.preactivations(xf, w_ih, b_ih, b_hh)
        act, c, h = R.forward(pre, w_hh, S, B)
        assert rel(h, y.reshape(S * B, 2 * R.HID)) <= TOL
        dpre = R.backward(act, c, w_hh, d_hout.reshape(S * B, 2 * R.HID), S, B)

        hs = h.reshape(S, B, 2, R.HID)
        dx = torch.zeros(S * B, I, dtype=torch.float64)
        for d in (0, 1):
            da = dpre[:, d]                                               # (S*B, 512)
            h_prev = torch.zeros(S, B, R.HID, dtype=torch.float64)
            if d == 0:
                h_prev[1:] = hs[:-1, :, 0]
            else:
                h_prev[:-1] = hs[1:, :, 1]
            h_prev = h_prev.reshape(S * B, R.HID)
            coeff = torch.cat([torch.ones(S * B, 1, dtype=torch.float64), xf, h_prev], 1)
            assert np.linalg.matrix_rank(coeff.numpy()) == S * B, "the compared images would not determine dgates"
            assert rel(da.sum(0), b_ih[d].grad) <= TOL
            assert rel(da.sum(0), b_hh[d].grad) <= TOL
            assert rel(da.T @ xf, w_ih[d].grad) <= TOL
            if S > 1:
                assert rel(da.T @ h_prev, w_hh[d].grad) <= TOL
            else:
                assert float(w_hh[d].grad.abs().max()) == 0.0 and float((da.T @ h_prev).abs().max()) == 0.0
            dx += da @ w_ih[d]
        assert rel(dx, x.grad.reshape(S * B, I)) <= TOL
