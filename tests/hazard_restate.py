"""numpy float64 restatement of the hazard cut head (include/rlt_hip.h, csrc/hazard.hip), forward and backward, from the stop
logits z (B,S) on: the kernels' own definitions, with sequential prefix sums in position order.

    s < S-1:  h_s = sigmoid(z_s),  L_s = -sum_{j<s} softplus(z_j),  p_s = exp(log sigmoid(z_s) + L_s)
    s = S-1:  h = 1,  p = exp(L_{S-1})
    T_j = sum_{k>j} p_k dp_k;   j < S-1: dz_j = (1-h_j) p_j dp_j - h_j T_j + dstop_j h_j (1-h_j);   dz_{S-1} = 0

tests/test_hazard_restate.py pins it to a torch float64 autograd composition."""
import numpy as np


def terms(z):
    """-> softplus(z), log sigmoid(z), sigmoid(z), 1 - sigmoid(z), each in its overflow-safe form"""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    t = np.log1p(e)
    r = 1.0 / (1.0 + e)
    return np.maximum(z, 0.0) + t, np.minimum(z, 0.0) - t, np.where(z >= 0, r, e * r), np.where(z >= 0, e * r, r)


def prior_offset(S):
    """offset_s = -log(S-1-s) for s < S-1, 0 at the end: with it z = 0 gives the uniform cut distribution"""
    off = np.zeros(S, dtype=np.float64)
    off[:S - 1] = -np.log(np.arange(S - 1, 0, -1, dtype=np.float64))
    return off


def forward(z):
    """z (B,S) -> (p, stop), float64"""
    z = np.asarray(z, dtype=np.float64)
    sp, logsig, h, _ = terms(z)
    S = z.shape[1]
    logp = logsig.copy()
    logp[:, S - 1] = 0.0
    stop = h.copy()
    stop[:, S - 1] = 1.0
    acc = np.zeros(z.shape[0])
    for s in range(S):                      # L_s in position order
        logp[:, s] -= acc
        acc = acc + sp[:, s]
    return np.exp(logp), stop


def backward(z, dp, dstop=None):
    """-> dz (B,S) float64"""
    z, dp = np.asarray(z, dtype=np.float64), np.asarray(dp, dtype=np.float64)
    p, _ = forward(z)
    _, _, h, omh = terms(z)
    S = z.shape[1]
    g = p * dp
    T = np.zeros_like(g)
    acc = np.zeros(z.shape[0])
    for s in range(S - 1, -1, -1):          # T_s from the end of the list
        T[:, s] = acc
        acc = acc + g[:, s]
    dz = omh * g - h * T
    if dstop is not None:
        dz = dz + np.asarray(dstop, dtype=np.float64) * h * omh
    dz[:, S - 1] = 0.0
    return dz


def ulp32(v):
    """the spacing of float32 at |v| (float64 array in, float64 out); 2^-149 below the normal range"""
    a = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
