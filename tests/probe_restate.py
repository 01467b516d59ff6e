"""Independent float64 numpy restatement of the probing study's heads and losses, and the seeded recipe of their inputs.

Shared by tools/make_probe_golden.py (which runs the reference's own modules on these inputs) and the tests, so the fixtures
hold no features: every side regenerates them from the recorded seed.
  probe_data(seed, B, S, E)      features x (B,S,E) float32 N(0,1) and labels y (B,S) float32 0/1 (robust04-shaped:
                                 Bernoulli(0.55 exp(-j/45) + 0.02) at rank j)
  head_params(seed, n, E)        n Linear(E,1) heads: w (n,E) ~ U(-1,1)/sqrt(E), b (n) ~ 0.1 U(-1,1)
  bce_head / rerank_head         loss, dw (E), db, out (B,S) of Linear -> Sigmoid -> nn.BCELoss (mean) and of
                                 Linear -> Softmax(dim=1) -> RerankLoss (utils/losses.py:99-141), in float64
"""
import math

import numpy as np

BCE, RERANK = 0, 1


def probe_data(seed, B, S, E):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, S, E)).astype(np.float32)
    prob = 0.55 * np.exp(-np.arange(S) / 45.0) + 0.02
    y = (rs.uniform(0, 1, (B, S)) < prob).astype(np.float32)
    return x, y


def head_params(seed, n, E):
    rs = np.random.RandomState(seed)
    w = (rs.uniform(-1, 1, (n, E)) / math.sqrt(E)).astype(np.float32)
    b = (0.1 * rs.uniform(-1, 1, n)).astype(np.float32)
    return w, b


def bce_head(x, y, w, b):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    z = x @ np.asarray(w, np.float64) + float(b)
    s = 1.0 / (1.0 + np.exp(-z))
    with np.errstate(divide="ignore"):
        l1 = np.maximum(np.log(s), -100.0)
        l0 = np.maximum(np.log1p(-s), -100.0)
    n = y.size
    loss = float(np.sum((y - 1.0) * l0 - y * l1) / n)
    g = (s - y) / np.maximum((1.0 - s) * s, 1e-12) / n * (1.0 - s) * s
    return loss, np.einsum("bs,bse->e", g, x), float(g.sum()), s


def rerank_head(x, y, w, b, margin=5e-4):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    z = x @ np.asarray(w, np.float64) + float(b)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    s = e / e.sum(axis=1, keepdims=True)
    pos, neg = y == 1.0, y == 0.0
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    E = x.shape[2]
    if n_pos == 0 or n_neg == 0:
        return 0.0, np.zeros(E), 0.0, s
    gap = s[neg].sum() / n_neg - s[pos].sum() / n_pos + margin
    if gap <= 0.0:
        return 0.0, np.zeros(E), 0.0, s
    g = np.where(pos, -1.0 / n_pos, np.where(neg, 1.0 / n_neg, 0.0))
    dz = s * (g - (s * g).sum(axis=1, keepdims=True))
    return float(gap), np.einsum("bs,bse->e", dz, x), float(dz.sum()), s


def head(kind, x, y, w, b, margin=5e-4):
    return bce_head(x, y, w, b) if kind == BCE else rerank_head(x, y, w, b, margin)
