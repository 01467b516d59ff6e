"""Float64 numpy restatement of the reward losses for any cut reward (include/rlt_hip.h: rlt_reward_spec,
rlt_reward_spec_matrix, rlt_reward_any_loss), written from their semantics: the spec rewards, the ideal value of a list, q, the
four loss kinds with d(loss)/dp, and the per-list outputs.  Independent of the library; tests/test_reward_any_restate.py pins it
to tests/loss_restate.py, to torch's float64 autograd and to a brute-force ideal ordering, tests/test_reward_any_gpu.py compares
the device against it."""
import numpy as np

EXPECT, CE, KL, JS = 0, 1, 2, 3
KINDS = (EXPECT, CE, KL, JS)
MAX_GRADES = 8


class Spec:
    """family 'fbeta' (beta) or 'gain' (gains per grade, discount: S numbers or None = 1 / log2(j + 2), normalize)."""

    def __init__(self, family, beta=1.0, gains=(), discount=None, normalize=False):
        self.family, self.beta, self.gains, self.normalize = family, float(beta), tuple(float(g) for g in gains), bool(normalize)
        self.discount = None if discount is None else np.asarray(discount, dtype=np.float64)


def fbeta(beta):
    return Spec("fbeta", beta=beta)


def gain(gains, discount=None, normalize=False):
    return Spec("gain", gains=gains, discount=discount, normalize=normalize)


def ndcg(penalty=-1.0):
    return gain((penalty, 1.0), None, True)


def grades(y, n_grades):
    """The label rounded to the nearest integer, clamped to 0..n_grades-1; NaN gives 0."""
    y = np.asarray(y, dtype=np.float64)
    g = np.where(np.isnan(y), 0.0, np.rint(np.where(np.isnan(y), 0.0, y)))
    return np.clip(g, 0, n_grades - 1).astype(np.int64)


def discounts(spec, S):
    return 1.0 / np.log2(np.arange(S) + 2.0) if spec.discount is None else spec.discount[:S].astype(np.float64)


def ideal(y, spec):
    """(B): sum over the grades of positive gain, in descending gain (ties: the higher grade first), of
    gain[g] * (D[a_g + n_g] - D[a_g]); D the prefix sum of the discounts, n_g the list's documents of grade g, a_g those of the
    grades taken before it."""
    y = np.asarray(y)
    B, S = y.shape
    g = grades(y, len(spec.gains))
    D = np.concatenate([[0.0], np.cumsum(discounts(spec, S))])
    order = sorted((t for t in range(len(spec.gains)) if spec.gains[t] > 0), key=lambda t: (-spec.gains[t], -t))
    out = np.zeros(B)
    at = np.zeros(B, dtype=np.int64)
    for t in order:
        n = (g == t).sum(1)
        out = out + spec.gains[t] * (D[at + n] - D[at])
        at = at + n
    return out


def reward64(y, spec):
    """(B,S) float64: r[b, k-1], the value of cutting list b after position k."""
    y = np.asarray(y, dtype=np.float64)
    B, S = y.shape
    if spec.family == "fbeta":
        rel = (y >= 1.0).astype(np.float64)
        c = np.cumsum(rel, axis=1)
        n = rel.sum(1, keepdims=True)
        k = np.arange(1, S + 1, dtype=np.float64)[None]
        b2 = spec.beta * spec.beta
        return np.where(c > 0, (1.0 + b2) * c / (b2 * n + k), 0.0)
    g = grades(y, len(spec.gains))
    cum = np.cumsum(np.asarray(spec.gains)[g] * discounts(spec, S)[None], axis=1)
    if not spec.normalize:
        return cum
    idl = ideal(y, spec)[:, None]
    return np.where(idl > 0, cum / np.where(idl > 0, idl, 1.0), 0.0)


def reward(y, spec):
    """The reward as the library hands it on: float64, rounded to fp32 once."""
    return reward64(y, spec).astype(np.float32)


def distribution(r, tau):
    """q = softmax(r / tau), the row maximum subtracted."""
    x = np.asarray(r, dtype=np.float64)
    e = np.exp((x - x.max(axis=1, keepdims=True)) / float(tau))
    return e / e.sum(axis=1, keepdims=True)


def _xlogx(x):
    return np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0)), 0.0)


def loss(p, r, kind, tau=1.0):
    """The loss on a reward matrix r (the fp32 values the library works from, taken as exact).
    -> dict: per_list (B), loss = sum(per_list) / B, dp (B,S) = d loss / d p, q, k (first maximum of p, plus 1), r_k, r_best,
    best_k (first maximum of r, plus 1), sums = [sum r_k, sum r_best, #(r_k == r_best), B].
    EXPECT: -sum p r; CE: -sum q ln p; KL: sum q (ln q - ln p); JS: (KL(q || m) + KL(p || m)) / 2 with m = (p + q) / 2, the
    gradient flowing through ln m and the target p."""
    p = np.asarray(p, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    B = p.shape[0]
    q = distribution(r, tau)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.log(p)
        if kind == EXPECT:
            terms, dp = -(p * r), -r
        elif kind == CE:
            terms, dp = np.where(q > 0, -q * lp, 0.0), -q / p
        elif kind == KL:
            terms, dp = _xlogx(q) - np.where(q > 0, q * lp, 0.0), -q / p
        elif kind == JS:
            lm = np.log((p + q) / 2.0)
            terms = 0.5 * ((_xlogx(q) - np.where(q > 0, q * lm, 0.0)) + (_xlogx(p) - np.where(p > 0, p * lm, 0.0)))
            dp = 0.5 * (lp - lm)
        else:
            raise ValueError(kind)
    per = terms.sum(1)
    rows = np.arange(B)
    k = np.argmax(p, axis=1) + 1
    best_k = np.argmax(r, axis=1) + 1
    r_k, r_best = r[rows, k - 1], r[rows, best_k - 1]
    return {"per_list": per, "loss": per.sum() / B, "dp": dp / B, "q": q, "k": k, "r_k": r_k, "r_best": r_best, "best_k": best_k,
            "sums": np.array([r_k.sum(), r_best.sum(), float((r_k == r_best).sum()), float(B)])}


def spec_loss(p, y, spec, kind, tau=1.0):
    return loss(p, reward(y, spec), kind, tau)


def distance(got, want):
    """max |got - want| as a fraction of the largest magnitude of `want` (0 for two all-zero arrays)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max())
    top = float(np.abs(want).max())
    return 0.0 if err == 0.0 else err / top if top > 0 else float("inf")


# ---- the text form of a reward (utils/rewards.py: RewardSpec.parse) ----------------------------------------------------
def parse(text):
    """'fbeta:<beta>' | 'ndcg' | 'ndcg:<penalty>' | 'gain:<g0>,<g1>[,...]' | 'gain:...:norm' -> Spec; ValueError otherwise."""
    head, _, rest = text.strip().partition(":")
    if head == "fbeta" and rest:
        b = float(rest)
        if not (b > 0 and np.isfinite(b)):
            raise ValueError(text)
        return fbeta(b)
    if head == "ndcg":
        return ndcg(float(rest)) if rest else ndcg()
    if head == "gain" and rest:
        body, sep, flag = rest.partition(":")
        if sep and flag != "norm":
            raise ValueError(text)
        gains = tuple(float(g) for g in body.split(","))
        if not 2 <= len(gains) <= MAX_GRADES:
            raise ValueError(text)
        return gain(gains, None, bool(sep))
    raise ValueError(text)
