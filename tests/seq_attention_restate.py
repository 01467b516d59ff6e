"""Float64 numpy restatement of within-list attention (csrc/attention_seq.hip: rlt_seq_attention_fwd / _bwd) and the inputs its
tests share.  tests/test_seq_attention_restate.py pins it to float64 torch.nn.MultiheadAttention / nn.TransformerEncoderLayer with
batch_first=True; tests/test_seq_attention_gpu.py compares the kernels with it.

Layout: qkv (S*B, 3E), row s*B + b, columns [q | k | v], head h = columns h*HD .. h*HD+HD of each.  The problem of (list b, head h)
is rows b, b+B, ...: scores q k^T / sqrt(HD), softmax over the keys, optional dropout on the normalised probabilities, P V.
Dropout: the stream of pair b*H + h is pair_seed(seed, b*H + h); weight (query i, key j) is kept iff keep(stream, i, j, threshold(p))
and then scaled by the fp32 value 1 / (1 - p) (tests/dropout_restate.py)."""
import math

import numpy as np

import dropout_restate as D


def heads(x, S, B, H, HD):
    """(S*B, n*H*HD) -> (n, B, H, S, HD) float64"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1] // (H * HD)
    return x.reshape(S, B, n, H, HD).transpose(2, 1, 3, 0, 4)


def rows(x):
    """(n, B, H, S, HD) -> (S*B, n*H*HD)"""
    n, B, H, S, HD = x.shape
    return x.transpose(3, 1, 0, 2, 4).reshape(S * B, n * H * HD)


def keep_mask(seed, S, B, H, p):
    """(B, H, S, S) float64 over (list, head, query, key): keep ? fp32(1 / (1 - p)) : 0"""
    out = np.empty((B, H, S, S))
    for b in range(B):
        for h in range(H):
            out[b, h] = D.mask(int(D.pair_seed(seed, b * H + h)), S, S, p)
    return out


def forward(qkv, S, B, H, HD, mask=None, keys=None):
    """-> out (S*B, E), lse (B, H, S), P (B, H, S, S) undropped.  keys: (K, V) as (B, H, n, HD) to attend to instead of the call's own
    (the yardsticks of the tests)."""
    q, k, v = heads(qkv, S, B, H, HD)
    if keys is not None:
        k, v = keys
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(HD)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = e / l
    pd = p if mask is None else p * mask
    return rows((pd @ v)[None]), (m + np.log(l))[..., 0], p


def backward(qkv, dout, S, B, H, HD, mask=None):
    """-> dqkv (S*B, 3E)"""
    q, k, v = heads(qkv, S, B, H, HD)
    do = heads(dout, S, B, H, HD)[0]
    p = forward(qkv, S, B, H, HD)[2]
    pd = p if mask is None else p * mask
    dv = pd.transpose(0, 1, 3, 2) @ do
    dp = do @ v.transpose(0, 1, 3, 2)
    if mask is not None:
        dp = dp * mask
    ds = p * (dp - (p * dp).sum(-1, keepdims=True)) / math.sqrt(HD)
    return rows(np.stack([ds @ k, ds.transpose(0, 1, 3, 2) @ q, dv]))


def rel(a, b):
    """relative max-norm error of a against the reference b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("randn", "last_key", "neighbour")
Q_COMMON = 2.0            # the component every query of a (list, head) has along that pair's unit vector w
LAST_KEY_WEIGHT = 0.65    # the median weight of the planted last key over the rows of its pair
TAIL_SCORE = 6.0          # scaled score, above log S, of the planted keys behind the buffer and in the neighbouring list


def inputs(kind, S, B, H, HD, seed=0):
    """-> qkv ((S + 1) * B, 3E) float32, dout (S * B, E) float32.  The rows of `position S` behind the S * B rows of the call hold, for
    every (list, head), a key along that pair's w with scaled score log S + TAIL_SCORE and a value of -4: a kernel that reads one key
    past S without masking it sees a dominant key (the tests hand the kernels this buffer with NaN behind it).
      randn      plain normal Q, K, V
      last_key   Q = its part orthogonal to w + Q_COMMON w, the other keys 0.5 randn, key S - 1 = c w with c such that the key holds
                 LAST_KEY_WEIGHT of the median row's weight (0.3 .. 0.9 of each row's: asserted on the host), value S - 1 = 4
      neighbour  Q as in last_key; the NEXT list's key at position S - 1 (row (S - 1) * B + b + 1) lies along list b's w with scaled
                 score log S + TAIL_SCORE, its value times 4: dominant for list b's queries if the kernel strays into that row"""
    assert kind in KINDS
    rng = np.random.default_rng([seed, KINDS.index(kind), S, B, H, HD])
    E = H * HD
    qkv = rng.standard_normal(((S + 1) * B, 3 * E))
    dout = rng.standard_normal((S * B, E))
    x = qkv.reshape(S + 1, B, 3, H, HD)                     # a view: [s, b, which, h]
    w = rng.standard_normal((B, H, HD))
    w /= np.linalg.norm(w, axis=-1, keepdims=True)
    big = (math.log(S) + TAIL_SCORE) * math.sqrt(HD) / Q_COMMON
    if kind != "randn":
        q = x[:S, :, 0]
        q += (Q_COMMON - (q * w).sum(-1, keepdims=True)) * w
    if kind == "last_key":
        x[:S - 1, :, 1] *= 0.5
        if S > 1:
            k = x[:S - 1, :, 1].transpose(1, 2, 0, 3)                                            # (B, H, S - 1, HD)
            qq = x[:S, :, 0].transpose(1, 2, 0, 3)
            sc = qq @ k.transpose(0, 1, 3, 2) / math.sqrt(HD)
            L = np.log(np.exp(sc - sc.max(-1, keepdims=True)).sum(-1)) + sc.max(-1)              # (B, H, S)
            score = np.median(L, -1) + math.log(LAST_KEY_WEIGHT / (1 - LAST_KEY_WEIGHT))         # the key's scaled score, per pair
            x[S - 1, :, 1] = (score * math.sqrt(HD) / Q_COMMON)[..., None] * w
        else:
            x[S - 1, :, 1] = w
        x[S - 1, :, 2] = 4.0
    if kind == "neighbour" and B > 1:                      # one list has no neighbour: nothing to plant (it would land on itself)
        nb = (np.arange(B) + 1) % B
        x[S - 1, nb, 1] = big * w
        x[S - 1, nb, 2] *= 4.0
    x[S, :, 1] = (big if kind != "randn" else big * Q_COMMON) * w          # randn: q . w is N(0, 1), not Q_COMMON
    x[S, :, 2] = -4.0
    return qkv.astype(np.float32), dout.astype(np.float32)


def yardsticks(qkv_tail, S, B, H, HD):
    """How far the float64 forward moves (relative max-norm of `out`) when a kernel gets a tile tail wrong -> dict:
      drop_last   the last key is left out
      past_S      key S - the planted row behind the buffer - is admitted
      past_S_zero key S is admitted as a zero row (what a kernel that zero-fills its tile but forgets the mask would see)
      neighbour   the last key / value of every list are read from the NEXT row in memory (list b + 1 at the same position)"""
    qkv = np.asarray(qkv_tail[:S * B], dtype=np.float64)
    ref = forward(qkv, S, B, H, HD)[0]
    _, k, v = heads(qkv, S, B, H, HD)
    tail = np.asarray(qkv_tail[S * B:], dtype=np.float64).reshape(1, B, 3, H, HD).transpose(2, 1, 3, 0, 4)      # (3, B, H, 1, HD)
    out = {}
    if S > 1:
        out["drop_last"] = rel(forward(qkv, S, B, H, HD, keys=(k[:, :, :S - 1], v[:, :, :S - 1]))[0], ref)
    out["past_S"] = rel(forward(qkv, S, B, H, HD, keys=(np.concatenate([k, tail[1]], 2), np.concatenate([v, tail[2]], 2)))[0], ref)
    zero = np.zeros_like(tail[1])
    out["past_S_zero"] = rel(forward(qkv, S, B, H, HD, keys=(np.concatenate([k, zero], 2), np.concatenate([v, zero], 2)))[0], ref)
    if B > 1:
        nb = (np.arange(B) + 1) % B
        k2, v2 = k.copy(), v.copy()
        k2[:, :, S - 1], v2[:, :, S - 1] = k[nb][:, :, S - 1], v[nb][:, :, S - 1]
        out["neighbour"] = rel(forward(qkv, S, B, H, HD, keys=(k2, v2))[0], ref)
    return out


# the shapes of the device tests: (S, B, H, HD).  Every tile-tail fill of both head dims once (the kernels' tiles: 64 keys staged, 32
# per product; 128 owned rows per pass at head dim 64, 32 at head dim 16), more than one workgroup per list (H 8 at head dim 16), a
# head group narrower than the workgroup's 64 columns (H 3 at head dim 16), B in {1, 3, 5}
SHAPES = [(1, 1, 1, 64), (2, 3, 3, 16), (15, 5, 4, 64), (16, 3, 8, 16), (17, 1, 3, 16), (31, 3, 1, 64), (32, 1, 8, 16), (33, 5, 3, 16),
          (63, 3, 4, 64), (64, 1, 1, 64), (64, 3, 3, 16), (65, 5, 8, 16), (65, 1, 4, 64), (127, 3, 3, 16), (127, 1, 1, 64),
          (128, 3, 4, 64), (129, 5, 1, 64), (129, 1, 8, 16), (300, 3, 4, 64), (300, 5, 8, 16)]
FWD_TOL, GRAD_TOL = 1e-5, 3e-5


def ulp32(x):
    """the spacing of float32 at |x| (normal range)"""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 23)


def lse_bound(lse_ref, score_max, fwd_tol=FWD_TOL):
    """lse = m + log l: a relative error eps in the normaliser l is an absolute error eps in lse, and eps is the forward tolerance;
    plus 4 fp32 ulps at the larger of |lse| and the row's largest |scaled score| for the rounding of the scores, of m + log l and
    of the stored value.  Derived, not measured; per row (the bound of the list-axis tests, restated)."""
    return fwd_tol + 4.0 * ulp32(np.maximum(np.abs(lse_ref), score_max))
