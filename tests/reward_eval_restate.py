"""Float64 numpy restatement of the evaluation pass in any cut reward (include/rlt_hip.h: rlt_reward_eval), written from its
semantics on top of tests/reward_any_restate.py's reward(): the (S+1)-entry row with r[b,0] = 0 in front, the reward at T
given cuts with clamping, the count of better cuts, the best cut (np.argmax: the first maximum) and the float64 split sums.
Independent of the library; tests/test_reward_eval_restate.py pins it, tests/test_reward_eval_gpu.py compares the device
against it."""
import numpy as np

import reward_any_restate as R


def row(r):
    """(B,S) reward for k = 1..S -> (B,S+1) for k = 0..S: cutting before the first document keeps nothing, r[b,0] = 0."""
    r = np.asarray(r)
    return np.concatenate([np.zeros((r.shape[0], 1), dtype=r.dtype), r], axis=1)


def evaluate(r, k=None, allow_empty=True):
    """r: the (B,S) reward, taken as exact (fp32 as the library hands it on, or float64).  k: (B,T) integer cuts or None.
    -> dict: r_at (B,T), better (B,T), best (B), best_k (B), curve (S+1), best_hist (S+1), sums (3 + 3T), clamped (B,T) bool."""
    r = np.asarray(r)
    B, S = r.shape
    full = row(r)
    kmin = 0 if allow_empty else 1
    span = full[:, kmin:]
    best_k = np.argmax(span, axis=1) + kmin
    best = full[np.arange(B), best_k]
    out = {"best": best, "best_k": best_k, "curve": full.astype(np.float64).sum(0),
           "best_hist": np.bincount(best_k, minlength=S + 1).astype(np.float64)}
    T = 0 if k is None else np.asarray(k).reshape(B, -1).shape[1]
    sums = np.zeros(3 + 3 * T)
    sums[0], sums[1] = B, best.astype(np.float64).sum()
    if T:
        k = np.asarray(k).reshape(B, T).astype(np.int64)
        kc = np.clip(k, 0, S)
        r_at = np.take_along_axis(full, kc, axis=1)
        better = (span[:, None, :] > r_at[:, :, None]).sum(2)
        out.update({"r_at": r_at, "better": better, "clamped": kc != k})
        sums[2] = (kc != k).sum()
        sums[3::3] = r_at.astype(np.float64).sum(0)
        sums[4::3] = (r_at == best[:, None]).sum(0)
        sums[5::3] = better.sum(0)
    out["sums"] = sums
    return out


def spec_evaluate(y, spec, k=None, allow_empty=True):
    """evaluate() on the reward of a spec, formed in float64 and rounded to fp32 once."""
    return evaluate(R.reward(y, spec), k, allow_empty)


def greedy_k(train_r, test_r, allow_empty=True):
    """(the test split's mean reward at k*, k*): k* = the first maximum of the train split's mean curve over kmin..S."""
    kmin = 0 if allow_empty else 1
    tr = row(train_r).astype(np.float64).sum(0) / len(train_r)
    k = int(np.argmax(tr[kmin:])) + kmin
    return float(row(test_r).astype(np.float64).sum(0)[k] / len(test_r)), k


def exact_f1_maximisers(y):
    """Per 0/1 list: the set of k in 0..S at which F1@k = 2 c_k / (N + k) (0 at k = 0 and where c_k = 0) is largest, in exact
    rational arithmetic.  The ground truth of a tie: the float64 chain of cal_F1 (p = c / k, r = c / N, 2 p r / (p + r)) rounds
    three times and may break - by one float64 ulp - a tie that the single correctly rounded division of the F_beta reward keeps."""
    from fractions import Fraction
    out = []
    for row_ in np.asarray(y):
        n = int((row_ >= 1).sum())
        c, vals = 0, [Fraction(0)]
        for k, v in enumerate(row_, 1):
            c += int(v >= 1)
            vals.append(Fraction(2 * c, n + k) if c else Fraction(0))
        top = max(vals)
        out.append([k for k, v in enumerate(vals) if v == top])
    return out
