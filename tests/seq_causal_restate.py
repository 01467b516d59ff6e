"""Float64 numpy restatement of MASKED within-list attention (csrc/attention_seq.hip: rlt_seq_attention_fwd_ex / _bwd_ex with
RLT_SEQ_MASK_CAUSAL), on the layout helpers of tests/seq_attention_restate.py.  tests/test_seq_causal_restate.py pins it to float64
torch.nn.MultiheadAttention with a boolean attn_mask; tests/test_seq_causal_gpu.py compares the kernels with it.

`allow` is a boolean (S, S) matrix over (query i, key j): scores outside it are -inf before the softmax, so lse is the
log-normaliser over the admitted keys.  The default is the causal mask j <= i.  `mask` is the dropout keep mask of
seq_attention_restate.keep_mask, applied to the normalised probabilities as there."""
import math

import numpy as np

import seq_attention_restate as R

heads, rows, keep_mask, rel = R.heads, R.rows, R.keep_mask, R.rel


def causal(S):
    """(S, S) bool over (query, key): key <= query"""
    i = np.arange(S)
    return i[None, :] <= i[:, None]


def probabilities(qkv, S, B, H, HD, allow=None):
    """-> P (B, H, S, S) undropped (exactly 0 outside `allow`), lse (B, H, S) over the admitted keys"""
    allow = causal(S) if allow is None else np.asarray(allow, dtype=bool)
    assert allow.shape == (S, S) and allow.any(-1).all(), "every query needs one admitted key"
    q, k, _ = heads(qkv, S, B, H, HD)
    s = np.where(allow, q @ k.transpose(0, 1, 3, 2) / math.sqrt(HD), -np.inf)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    return e / l, (m + np.log(l))[..., 0]


def forward(qkv, S, B, H, HD, mask=None, allow=None):
    """-> out (S*B, E), lse (B, H, S), P (B, H, S, S) undropped"""
    p, lse = probabilities(qkv, S, B, H, HD, allow)
    v = heads(qkv, S, B, H, HD)[2]
    pd = p if mask is None else p * mask
    return rows((pd @ v)[None]), lse, p


def backward(qkv, dout, S, B, H, HD, mask=None, allow=None):
    """-> dqkv (S*B, 3E)"""
    q, k, v = heads(qkv, S, B, H, HD)
    do = heads(dout, S, B, H, HD)[0]
    p = probabilities(qkv, S, B, H, HD, allow)[0]
    pd = p if mask is None else p * mask
    dv = pd.transpose(0, 1, 3, 2) @ do
    dp = do @ v.transpose(0, 1, 3, 2)
    if mask is not None:
        dp = dp * mask
    ds = p * (dp - (p * dp).sum(-1, keepdims=True)) / math.sqrt(HD)
    return rows(np.stack([ds @ k, ds.transpose(0, 1, 3, 2) @ q, dv]))


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("randn", "ramp_v")


def inputs(kind, S, B, H, HD, seed=0):
    """-> qkv (S * B, 3E) float32, dout (S * B, E) float32.
      randn   plain normal Q, K, V
      ramp_v  randn Q, K, dout; V at position j scaled by j + 1: a weight near 1 / (i + 1) on one key too many or too few at the
              diagonal then still moves row i of `out` by O(1) of its size, at every tile edge and however long the row is"""
    assert kind in KINDS
    rng = np.random.default_rng([seed, 77 + KINDS.index(kind), S, B, H, HD])
    E = H * HD
    qkv = rng.standard_normal((S * B, 3 * E))
    dout = rng.standard_normal((S * B, E))
    if kind == "ramp_v":
        qkv.reshape(S, B, 3, E)[:, :, 2] *= (np.arange(S) + 1.0)[:, None, None]
    return qkv.astype(np.float32), dout.astype(np.float32)


# ------------------------------------------------------------------------------------------------ wrong diagonals
def variants(S):
    """the masks a kernel with a wrong diagonal would apply -> {name: (S, S) bool}"""
    i = np.arange(S)
    q, k = i[:, None], i[None, :]
    strict = k < q
    strict[0, 0] = True                                        # row 0 keeps key 0 (it has nothing else)
    return {"strict": strict, "one_more": k <= q + 1, "tile32": k // 32 <= q // 32, "tile64": k // 64 <= q // 64,
            "none": np.ones((S, S), dtype=bool), "transposed": k >= q}


def block_moves(got, ref, S, B, scale):
    """max |got - ref| / scale per 32-position block of a position-major (S*B, C) array -> (ceil(S / 32),)"""
    d = np.abs(np.asarray(got) - np.asarray(ref)).reshape(S, -1).max(-1)
    return np.array([d[t:t + 32].max() for t in range(0, S, 32)]) / scale
