"""Float64 restatement of rlt_pair_rank_loss (include/rlt_hip.h, "pairwise ranking losses"): RankNet and LambdaRank over the
documents of each list, the counting rank, n_pairs, the per-list and batch loss, d(loss)/d(score) and, for the tolerance of the
GPU test, A_i = the sum of |lam| over the pairs of document i at the gradient's scaling.  numpy only, one list at a time, (S,S)
matrices; the inputs are the float32 values the device sees, widened exactly.

`mistake` plants one of three errors a kernel could make, for tests/test_pair_rank_restate.py to show that the inputs of the GPU
test would catch it: "tie" reverses the tie-break of the counting rank, "drop_last" forgets the list's last document, "discount"
reads the discount one position late."""
import numpy as np

RANKNET, LAMBDARANK = 0, 1
KINDS = {"ranknet": RANKNET, "lambdarank": LAMBDARANK}
MAX_S = 1024
MISTAKES = ("tie", "drop_last", "discount")
CUSTOM_GAINS = (0.0, 0.5, 1.0, 3.0, 2.5, 7.0, 15.0, 31.5)       # 8 grades, not monotone: grade 4 gains less than grade 3


def grades(labels, n_grades):
    """rlt_reward_spec's rule: round to nearest (ties to even), clamp to 0..n_grades-1, NaN -> 0."""
    y = np.asarray(labels, dtype=np.float32).astype(np.float64)
    g = np.rint(y)
    g = np.where(np.isnan(g), 0.0, g)
    return np.clip(g, 0, n_grades - 1).astype(np.int64)


def default_gains(n_grades):
    return [float(2 ** g - 1) for g in range(n_grades)]


def counting_rank(s, reverse_ties=False):
    """pi_i = #{ j : s_j > s_i, or s_j == s_i and j < i } for each row of s (B,S) float32; int32."""
    s = np.asarray(s, dtype=np.float32)
    if s.ndim == 1:
        s = s[None]
    out = np.empty(s.shape, dtype=np.int32)
    idx = np.arange(s.shape[1])
    first = idx[None, :] > idx[:, None] if reverse_ties else idx[None, :] < idx[:, None]       # [i, j]
    for b in range(s.shape[0]):
        v = s[b]
        out[b] = ((v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & first)).sum(axis=1)
    return out


def discount(r):
    return 1.0 / np.log2(np.asarray(r, dtype=np.float64) + 2.0)


_PREFIX = np.concatenate([[0.0], np.cumsum(discount(np.arange(MAX_S)))])     # D[k] = sum_{j<k} 1/log2(j+2), sequential


def ideal_value(g, gains):
    """The ideal gain x discount value of a list as rlt_reward_spec defines it for a GAIN spec: the grades of positive gain in
    descending gain (ties: the higher grade first), each taking the next n_g positions."""
    order = sorted((k for k in range(len(gains)) if np.float32(gains[k]) > 0), key=lambda k: (-float(np.float32(gains[k])), -k))
    ideal, at = 0.0, 0
    for k in order:
        c = int((g == k).sum())
        ideal += float(np.float32(gains[k])) * (_PREFIX[at + c] - _PREFIX[at])
        at += c
    return ideal


def softplus_neg(x):
    """softplus(-x) = max(-x, 0) + log1p(exp(-|x|))"""
    return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid_neg(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def one_list(s, y, kind, sigma, gains, n_grades, normalize, scale, mistake=None):
    """-> (rank int32 (S), n_pairs, loss, dscore (S) float64, A (S) float64) of one list; `scale` = gscale / B."""
    s32 = np.asarray(s, dtype=np.float32)
    S = s32.shape[0]
    sd = s32.astype(np.float64)
    g = grades(y, n_grades)
    gv = np.array([float(np.float32(v)) for v in gains], dtype=np.float64)
    G = gv[g]
    rank = counting_rank(s32, reverse_ties=(mistake == "tie"))[0]
    alive = np.ones(S, dtype=bool)
    if mistake == "drop_last":
        alive[S - 1] = False
    pair = (g[:, None] > g[None, :]) & alive[:, None] & alive[None, :]        # [i, j]: i leads
    n_pairs = int((g[:, None] > g[None, :]).sum())
    n_used = int(pair.sum())
    sig = float(np.float32(sigma))
    if np.isnan(sd).any():                      # a NaN score: the list's loss and its row of dscore are NaN, pairs or not
        return rank, n_pairs, float("nan"), np.full(S, np.nan), np.zeros(S)
    if n_used == 0:
        z = np.zeros(S)
        return rank, n_pairs, 0.0, z, z.copy()
    if kind == LAMBDARANK:
        D = discount(rank + (1 if mistake == "discount" else 0))
        w = np.abs(G[:, None] - G[None, :]) * np.abs(D[:, None] - D[None, :])
        if normalize:
            ideal = ideal_value(g, gains)
            if ideal > 0:
                w = w / ideal
    else:
        w = np.ones((S, S))
    w = np.where(pair, w, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        x = sig * (sd[:, None] - sd[None, :])
        l = w * np.where(pair, softplus_neg(x), 0.0)
        lam = -sig * w * np.where(pair, sigmoid_neg(x), 0.0)
    norm = 1.0 / n_used if kind == RANKNET else 1.0
    loss = float(l.sum()) * norm
    d = scale * norm * (lam.sum(axis=1) - lam.sum(axis=0))
    A = abs(scale) * norm * (np.abs(lam).sum(axis=1) + np.abs(lam).sum(axis=0))
    return rank, n_pairs, loss, d, A


def restate(score, labels, kind, sigma=1.0, gains=None, n_grades=2, normalize=True, gscale=1.0, mistake=None, batch=None):
    """-> dict(rank (B,S) int32, n_pairs (B) int32, loss_per_list (B), loss, dscore (B,S), A (B,S)), float64 where not integer.
    batch: the B of the call these lists are the first rows of (the gradient's 1 / B), default their own count."""
    kind = KINDS.get(kind, kind)
    score = np.asarray(score, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.float32)
    B, S = score.shape
    if gains is None:
        gains = default_gains(n_grades)
    n_grades = len(gains)
    scale = float(np.float32(gscale)) / (batch or B)
    out = {"rank": np.empty((B, S), np.int32), "n_pairs": np.empty(B, np.int32), "loss_per_list": np.empty(B),
           "dscore": np.empty((B, S)), "A": np.empty((B, S))}
    for b in range(B):
        r, n, l, d, A = one_list(score[b], labels[b], kind, sigma, gains, n_grades, normalize, scale, mistake)
        out["rank"][b], out["n_pairs"][b], out["loss_per_list"][b], out["dscore"][b], out["A"][b] = r, n, l, d, A
    out["loss"] = float(np.sum(out["loss_per_list"])) / B
    return out


# ---- the inputs of the GPU test ---------------------------------------------------------------------------------------------
# name -> (score kind, label kind).  Every score kind holds at least one exact tie (a reversed tie-break must show) and every
# label kind but "none" / "all" - which have no pairs, so nothing can move - has pairs that involve the last document or not.
CLASSES = {
    "randn": ("randn", "binary"),
    "ties": ("ties", "binary"),
    "saturated": ("saturated", "binary"),
    "none": ("randn", "none"),
    "one": ("randn", "one"),
    "all": ("randn", "all"),
    "graded": ("randn", "graded"),
}
PAIRLESS = ("none", "all")


def class_args(name):
    """the keyword arguments (gains / n_grades) of restate and of the device call for an input class"""
    return {"gains": list(CUSTOM_GAINS)} if name == "graded" else {"n_grades": 2}


def inputs(name, B, S, sigma=1.0, seed=0):
    """(score (B,S) float32, labels (B,S) float32) of an input class."""
    skind, lkind = CLASSES[name]
    rng = np.random.default_rng(1000003 * seed + 7919 * S + 31 * B + sorted(CLASSES).index(name))
    if skind == "randn":
        s = rng.standard_normal((B, S))
    elif skind == "ties":
        s = rng.integers(-3, 4, size=(B, S)) / 4.0             # seven values, one of them zero
    else:
        s = rng.uniform(-30.0, 30.0, size=(B, S)) / sigma
        if S >= 2:
            s[:, 0], s[:, -1] = 30.0 / sigma, -30.0 / sigma
    s = s.astype(np.float32)
    if skind == "ties":
        zero = s == 0
        s[zero & (rng.random((B, S)) < 0.5)] = -0.0            # +0 and -0 are a tie
    if S >= 4:                                                  # one exact tie in every list, whatever the kind
        for b in range(B):
            i, j = rng.choice(S, size=2, replace=False)
            s[b, j] = s[b, i]
    if lkind == "binary":
        y = (rng.random((B, S)) < 0.3).astype(np.float32)
    elif lkind == "none":
        y = np.zeros((B, S), np.float32)
    elif lkind == "all":
        y = np.ones((B, S), np.float32)
    elif lkind == "one":
        y = np.zeros((B, S), np.float32)
        y[np.arange(B), rng.integers(0, S, size=B)] = 1.0
    else:
        y = rng.integers(0, 8, size=(B, S)).astype(np.float32)
        y += rng.uniform(-0.4, 0.4, size=(B, S)).astype(np.float32)           # rounds back to the grade
        if S >= 3:
            y[:, 1] = np.nan                                    # NaN label: grade 0
            y[:, 2] = 9.25                                      # above the top grade: clamped to 7
    return s, y


# ---- the tolerance of the GPU test (the issue's form; K is measured there) ---------------------------------------------------
def fp32_rounding(v):
    """one fp32 rounding of v: half the spacing of float32 at v (the subnormal spacing near 0)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    return 0.5 * np.spacing(np.maximum(v, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


K_MEASURED = 3.1            # worst ratio over all ids of tests/test_pair_rank_gpu.py on an MI355X: loss 1.283, gradient 3.099
K_ASSERT = 4.0 * K_MEASURED


def loss_bound(ref, K):
    return K * 2.0 ** -24 * np.abs(ref) + fp32_rounding(ref)


def grad_bound(ref, A, K):
    return K * 2.0 ** -24 * np.asarray(A) + fp32_rounding(ref)
