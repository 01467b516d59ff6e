"""Plain numpy float64 restatement of the MMOE gates / mixture, BiCut's two-class head and BiCutLoss, the two layout maps and the
Choopy embedding, written from include/rlt_hip.h and the reference formulas it cites (models/MMOECut.py:93-94,101-102,
models/Bicut.py:11-16, utils/losses.py:11-45, models/Choopy.py:19-20) - not from the kernels.  No device code; pinned to the
oracle, to torch float64 autograd and to the reference's golden by tests/test_mmoe_bicut_restate.py.

Layouts, as the header states them: position-major rows are tok = s * B + b; a gate matrix w_gate[t] is (S * C, n_e) with row
index s * C + c; gates are (n_tasks, B, n_e); experts (n_e, S * B, E); mixed (n_tasks, S * B, E); the two-class head reads
position-major logits (S * B, 2) and writes (B, S, 2)."""
import numpy as np

F64 = np.float64


# ---------------------------------------------------------------------------------------------- layout
def to_position_major(x_bsf):
    """(B, S, F) -> (S * B, F), row s * B + b.  A pure re-indexing: the dtype (and every bit) is kept."""
    B, S, Fd = x_bsf.shape
    return np.ascontiguousarray(x_bsf.transpose(1, 0, 2)).reshape(S * B, Fd)


def from_position_major(x_sbf, B, S):
    """(S * B, F) -> (B, S, F)"""
    return np.ascontiguousarray(x_sbf.reshape(S, B, -1).transpose(1, 0, 2))


def choopy_embed(score_bs, pe):
    """out[s * B + b, 0] = score[b, s]; out[s * B + b, 1 + c] = pe[s, c]"""
    B, S = score_bs.shape
    out = np.empty((S, B, 1 + pe.shape[1]), dtype=score_bs.dtype)
    out[:, :, 0] = score_bs.T
    out[:, :, 1:] = pe[:, None, :]
    return out.reshape(S * B, -1)


# ---------------------------------------------------------------------------------------------- MMOE gates
def flatten_lists(h, S, B):
    """position-major (S * B, C) -> (B, S * C): list b's rows side by side, column s * C + c"""
    C = h.shape[1]
    return np.asarray(h, dtype=F64).reshape(S, B, C).transpose(1, 0, 2).reshape(B, S * C)


def gate_logits(h, w_gate, S, B):
    flat = flatten_lists(h, S, B)
    return np.stack([flat @ np.asarray(w, dtype=F64) for w in w_gate])                  # (n_tasks, B, n_e)


def softmax(z, axis=-1):
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def gates(h, w_gate, S, B):
    return softmax(gate_logits(h, w_gate, S, B))


def gate_dlogit(g, dg):
    g, dg = np.asarray(g, dtype=F64), np.asarray(dg, dtype=F64)
    return g * (dg - (g * dg).sum(-1, keepdims=True))


def gate_bwd(h, w_gate, g, dg, S, B):
    """-> dlogit (n_tasks, B, n_e), dh (S * B, C), dw_gate (n_tasks, S * C, n_e) from the gates g handed in and their
    gradient dg"""
    C = h.shape[1]
    dl = gate_dlogit(g, dg)
    flat = flatten_lists(h, S, B)
    dflat = sum(dl[t] @ np.asarray(w, dtype=F64).T for t, w in enumerate(w_gate))         # (B, S * C)
    dh = dflat.reshape(B, S, C).transpose(1, 0, 2).reshape(S * B, C)
    dw = np.stack([flat.T @ dl[t] for t in range(len(w_gate))])
    return dl, dh, dw


# ---------------------------------------------------------------------------------------------- MMOE mixture
def mix_fwd(experts, g, B):
    """experts (n_e, T, E), g (n_tasks, B, n_e) -> mixed (n_tasks, T, E): token tok belongs to list tok % B"""
    x, g = np.asarray(experts, dtype=F64), np.asarray(g, dtype=F64)
    b = np.arange(x.shape[1]) % B
    return np.einsum("tke,ekc->tkc", g[:, b, :], x)


def mix_bwd(experts, g, dmixed, B):
    """-> dexperts (n_e, T, E), dgates (n_tasks, B, n_e)"""
    x, g, dm = np.asarray(experts, dtype=F64), np.asarray(g, dtype=F64), np.asarray(dmixed, dtype=F64)
    T = x.shape[1]
    b = np.arange(T) % B
    dx = np.einsum("tke,tkc->ekc", g[:, b, :], dm)
    per_tok = np.einsum("tkc,ekc->tke", dm, x)                                            # (n_tasks, T, n_e)
    dg = np.zeros(g.shape, dtype=F64)
    for t in range(g.shape[0]):
        np.add.at(dg[t], b, per_tok[t])
    return dx, dg


# ---------------------------------------------------------------------------------------------- BiCut's two-class head
def pair_softmax(z, keep, S, B):
    """z, keep (S * B, 2) position-major, keep in {0, 1 / (1 - p)} -> out (B, S, 2) = softmax(z * keep)"""
    y = softmax(np.asarray(z, dtype=F64) * np.asarray(keep, dtype=F64))
    return from_position_major(y, B, S)


def pair_softmax_bwd(out, dout, keep, S, B):
    """out, dout (B, S, 2) -> dz (S * B, 2) = keep * y * (g - sum(y g))"""
    y, g = to_position_major(np.asarray(out, dtype=F64)), to_position_major(np.asarray(dout, dtype=F64))
    return np.asarray(keep, dtype=F64) * y * (g - (y * g).sum(1, keepdims=True))


# ---------------------------------------------------------------------------------------------- BiCutLoss
def bicut_last_truncate(out):
    """index of the last position whose argmax over the two classes is 0 (a tie is class 0), S when there is none"""
    S = out.shape[1]
    class0 = ~(out[..., 1] > out[..., 0])
    last0 = np.where(class0, np.arange(S)[None, :], -1).max(1)
    return np.where(last0 < 0, S, last0)


def bicut_reward(labels, nci, alpha, r, dtype=F64):
    """(B, S, 2) reward pairs.  dtype = float32 rounds them as the reference does (it keeps them in a float32 tensor)."""
    B, S = labels.shape
    pos = np.asarray(labels) == 1
    j = np.arange(S, dtype=F64)[None, :]
    rew = np.zeros((B, S, 2), dtype=F64)
    if nci:
        rew[..., 1] = np.where(pos, -1.0 / np.log2(j + 2.0), (j + 1.0) / alpha)
    else:
        rew[..., 0] = np.where(pos, (1.0 - alpha) / r, 0.0)
        rew[..., 1] = np.where(pos, 0.0, alpha / (1.0 - r))
    return rew.astype(dtype).astype(F64)


def bicut_loss(out, labels, nci, alpha, r, reward_dtype=F64):
    """-> per_list (B) unnormalised, loss = sum(per_list) / B, dout (B, S, 2) = mask * reward / B, mask (B, S) in {0, 1},
    abs_terms (B) = sum |out * mask * reward| (the scale of a list's summation error)"""
    out = np.asarray(out, dtype=F64)
    B, S = labels.shape
    idx = bicut_last_truncate(out)
    mask = (np.arange(S)[None, :] <= idx[:, None]).astype(F64)
    rew = bicut_reward(labels, nci, alpha, r, reward_dtype)
    terms = out * mask[..., None] * rew
    per_list = terms.sum((1, 2))
    return per_list, per_list.sum() / B, mask[..., None] * rew / B, mask, np.abs(terms).sum((1, 2))


# ---------------------------------------------------------------------------------------------- BiCutLoss inputs with placed edges
LAST0_PLACES = (0, 63, 64, 127, 128, "end", "none", "ties", "random")
LABEL_FILLS = ("zero", "one", "single", "random")


def bicut_edge_lists(B, S, offset=0, only=None, seed=0):
    """Probabilities built directly, (B, S, 2) float32 with a clear winner (0.55 .. 0.95 against its complement) at every
    position that is no tie, and labels (B, S).  Row i takes place LAST0_PLACES[(i + offset) % 9] (or `only`) where S has it:
    an integer k - the last class-0 position is k, class 1 after it; "end" - k = S - 1; "none" - class 1 everywhere (nothing
    is masked); "ties" - exact (0.5, 0.5) up to S // 2 and class 1 after it, so the mask ends at S // 2 only if a tie is
    class 0; "random" - class 0 with probability 0.3.  Labels by (i + i // 9) % 4: all 0, all 1, a single 1, Bernoulli(0.2).
    -> (out, labels, idx): idx the mask's last index each row must give (S for "none"; for "random" whatever it holds)."""
    g = np.random.default_rng(7919 * B + 104729 * S + 31 * offset + seed)
    cls = (g.random((B, S)) >= 0.3).astype(np.int64)
    hi = g.uniform(0.55, 0.95, (B, S)).astype(np.float32)
    labels = (g.random((B, S)) < 0.2).astype(np.float32)
    tie = np.zeros((B, S), dtype=bool)
    idx = np.empty(B, dtype=np.int64)
    for i in range(B):
        place = only if only is not None else LAST0_PLACES[(i + offset) % len(LAST0_PLACES)]
        if place == "end":
            place = S - 1
        if place == "ties":
            tie[i, :S // 2 + 1] = True
            cls[i, S // 2 + 1:] = 1
            idx[i] = S // 2
        elif place == "none":
            cls[i] = 1
            idx[i] = S
        elif place == "random" or place >= S:
            zeros = np.nonzero(cls[i] == 0)[0]
            idx[i] = zeros[-1] if len(zeros) else S
        else:
            cls[i, place] = 0
            cls[i, place + 1:] = 1
            idx[i] = place
        fill = LABEL_FILLS[(i + i // len(LAST0_PLACES)) % 4]
        if fill != "random":
            labels[i] = 1.0 if fill == "one" else 0.0
        if fill == "single":
            labels[i, g.integers(S)] = 1.0
    out = np.empty((B, S, 2), dtype=np.float32)
    lo = (np.float32(1.0) - hi).astype(np.float32)
    out[..., 0] = np.where(cls == 0, hi, lo)
    out[..., 1] = np.where(cls == 1, hi, lo)
    out[tie] = np.float32(0.5)
    return out, labels, idx
