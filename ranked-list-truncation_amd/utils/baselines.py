"""Truncation baselines on the HIP hot path - the reference's Baseline/ notebooks without their O(S^2) host loops.

  Oracle.ipynb               best_cut(labels): mean over lists of the best F1 / DCG any cut k = 0..S achieves
  Fixed_k.ipynb              fixed_k(labels, k): mean F1 / DCG when every list is cut at k (k or the notebook's [k_f1, k_dcg])
  Greedy_k.ipynb             greedy_k(train, test): the k with the best mean F1 (DCG) on train, applied to test
  (no notebook)              score_threshold(train, test, thresholds): cut where the retrieval score falls below a threshold
                             tuned on train - the label-free rule beside Greedy-k (rlt_cut_sweep, FIRST_BELOW)
  Truncation_analysis.ipynb  TruncationCurves.f1_curve() / dcg_curve() (mean over lists for each k = 0..S) and
                             irrelevant_share() (`countp`: share of irrelevant documents in each prefix, k = 1..S)

  (no notebook)              RewardCurves / best_cut_reward / fixed_k_reward / greedy_k_reward: the same three rows in ANY cut
                             reward (utils.rewards.RewardSpec: F_beta, graded gain, nDCG) from rlt_reward_eval

Semantics are the notebooks' cal_F1 / cal_DCG in float64 (include/rlt_hip.h, rlt_truncation_curves): labels (B, S) 0/1 in rank
order, F1@k = 2pr / (p + r) with p = c_k / k, r = c_k / N; DCG@k = sum_{i<k} (label == 1 ? 1 : penalty) / log2(i + 2); k = 0 is
an entry of every curve with value 0, so a list's best DCG is never negative.  One difference: where the train curve's best F1 cut
is k = 0 the notebook's Greedy-k divides by zero; here the result is the curve's value there, 0.

`TruncationCurves` streams a split through batch by batch on the device; the host synchronises only when a Python number is
asked for.  GPU only, like utils/metrics.py.  (The Oracle row is `best_cut`: the package's Python sources never spell that
word in lower case, the name of the CPU test reference they must not import - tests/test_abi.py checks it.)
"""
import numpy as np
import torch

from rlt_hip import native as N
from rlt_hip import ops


def _dev(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError("utils.baselines runs on the GPU (HIP kernels); no CPU fallback exists")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _labels(labels, device):
    t = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels, dtype=np.float32)))
    if t.dim() != 2:
        raise ValueError(f"labels must be (lists, positions); got shape {tuple(t.shape)}")
    return N.f32c(t.to(device, non_blocking=True))


class TruncationCurves:
    """Running sums of the truncation curves of lists of S positions: update() with (B, S) batches, then read the means."""

    def __init__(self, S, device=None, penalty=-1):
        S = int(S)
        if not 1 <= S <= 1024:
            raise ValueError(f"list length {S} outside 1..1024")
        self.S, self.penalty = S, float(penalty)
        self.device = _dev(device)
        self.curves = torch.zeros((3, S + 1), dtype=torch.float64, device=self.device)   # sums of F1@k, DCG@k, c_k
        self.sums = torch.zeros((3,), dtype=torch.float64, device=self.device)           # sum best F1, sum best DCG, lists
        self._n = 0

    def update(self, labels):
        y = _labels(labels, self.device)
        if y.shape[1] != self.S:
            raise ValueError(f"lists of {y.shape[1]} positions, this accumulator holds {self.S}")
        if y.shape[0]:
            ops.truncation_curves(y, self.penalty, curves=self.curves, sums=self.sums)
            self._n += int(y.shape[0])
        return self

    @property
    def n_lists(self):
        return self._n

    def _mean(self, row):
        if not self._n:
            raise ValueError("no lists have been added")
        return self.curves[row] / self._n

    def f1_curve(self):
        """Mean F1@k over the lists, k = 0..S: (S+1,) float64 on the device."""
        return self._mean(0)

    def dcg_curve(self):
        """Mean DCG@k over the lists, k = 0..S: (S+1,) float64 on the device."""
        return self._mean(1)

    def hits_curve(self):
        """Mean number of relevant documents in the first k, k = 0..S: (S+1,) float64 on the device."""
        return self._mean(2)

    def irrelevant_share(self):
        """`countp` of Truncation_analysis: (L k - sum of c_k) / (L k) for k = 1..S over L lists, (S,) float64 on the device."""
        if not self._n:
            raise ValueError("no lists have been added")
        lk = self._n * torch.arange(1, self.S + 1, dtype=torch.float64, device=self.device)
        return (lk - self.curves[2, 1:]) / lk

    def best_cut(self):
        """The notebooks' Oracle: (mean best F1, mean best DCG) over the lists, each list's best over k = 0..S."""
        if not self._n:
            raise ValueError("no lists have been added")
        s = self.sums.tolist()
        return s[0] / s[2], s[1] / s[2]

    def _k(self, k):
        k = int(k)
        if not 0 <= k <= self.S:
            raise ValueError(f"cut position {k} outside 0..{self.S}")
        return k

    def fixed_k(self, k):
        """(mean F1@k, mean DCG@k); k an int, or the notebook's pair [k_f1, k_dcg]."""
        k_f1, k_dcg = (k, k) if np.ndim(k) == 0 else k
        k_f1, k_dcg = self._k(k_f1), self._k(k_dcg)
        f1 = self.f1_curve()[k_f1]
        dcg = self.dcg_curve()[k_dcg]
        return float(f1), float(dcg)

    def best_k(self):
        """(k_F1, k_DCG): the first maximum of each mean curve over k = 0..S (np.argmax)."""
        f1 = self.f1_curve().cpu().numpy()
        dcg = self.dcg_curve().cpu().numpy()
        return int(np.argmax(f1)), int(np.argmax(dcg))


class RewardCurves:
    """TruncationCurves in any cut reward: running sums of r[b,k], k = 0..S (r[b,0] = 0), and of each list's best reward, for
    lists of S positions under a RewardSpec.  allow_empty=False takes the best over k = 1..S, the range the losses train on."""

    def __init__(self, S, spec, device=None, allow_empty=True):
        from utils.rewards import RewardSpec
        S = int(S)
        if not 1 <= S <= 1024:
            raise ValueError(f"list length {S} outside 1..1024")
        self.S, self.spec, self.allow_empty = S, RewardSpec.parse(spec), bool(allow_empty)
        self.device = _dev(device)
        self._acc = None
        self._n = 0

    def update(self, labels):
        y = _labels(labels, self.device)
        if y.shape[1] != self.S:
            raise ValueError(f"lists of {y.shape[1]} positions, this accumulator holds {self.S}")
        if y.shape[0]:
            _, self._acc = ops.reward_eval(y, self.spec, allow_empty=self.allow_empty, acc=self._acc, per_list=False)
            self._n += int(y.shape[0])
        return self

    @property
    def n_lists(self):
        return self._n

    def curve(self):
        """Mean reward at k over the lists, k = 0..S: (S+1,) float64 on the device."""
        if not self._n:
            raise ValueError("no lists have been added")
        return self._acc["curve"] / self._n

    def best_hist(self):
        """How many lists have their best cut at k, k = 0..S: (S+1,) float64 on the device."""
        if not self._n:
            raise ValueError("no lists have been added")
        return self._acc["best_hist"]

    def best_cut(self):
        """The Oracle row in this reward: the mean over the lists of each list's best reward."""
        if not self._n:
            raise ValueError("no lists have been added")
        s = self._acc["sums"].tolist()
        return s[1] / s[0]

    def fixed_k(self, k):
        """The mean reward when every list is cut at k, 0 <= k <= S."""
        k = int(k)
        if not 0 <= k <= self.S:
            raise ValueError(f"cut position {k} outside 0..{self.S}")
        return float(self.curve()[k])

    def best_k(self):
        """The first maximum of the mean curve over kmin..S (np.argmax), kmin = 0 with allow_empty."""
        c = self.curve().cpu().numpy()
        return int(np.argmax(c)) if self.allow_empty else int(np.argmax(c[1:])) + 1


def _reward_curves(labels, spec, device, allow_empty):
    y = _labels(labels, _dev(device))
    return RewardCurves(y.shape[1], spec, y.device, allow_empty).update(y)


def best_cut_reward(labels, spec, device=None, allow_empty=True):
    """The Oracle row in the reward `spec`: the mean over the lists of labels (B, S) of the best reward any cut achieves."""
    return _reward_curves(labels, spec, device, allow_empty).best_cut()


def fixed_k_reward(labels, k, spec, device=None):
    """The Fixed-k row in the reward `spec`: the mean reward when every list is cut at k."""
    return _reward_curves(labels, spec, device, True).fixed_k(k)


def greedy_k_reward(train_labels, test_labels, spec, device=None, allow_empty=True):
    """The Greedy-k row in the reward `spec`: k* = the first maximum of the train split's mean reward curve, then the test
    split's mean reward at k*.  Returns (reward, k*)."""
    k = _reward_curves(train_labels, spec, device, allow_empty).best_k()
    return _reward_curves(test_labels, spec, device, allow_empty).fixed_k(k), k


def _curves(labels, penalty, device):
    y = _labels(labels, _dev(device))
    return TruncationCurves(y.shape[1], y.device, penalty).update(y)


def best_cut(labels, penalty=-1, device=None):
    """Oracle.ipynb's test_scores: (mean best F1, mean best DCG) over the lists of labels (B, S)."""
    return _curves(labels, penalty, device).best_cut()


def fixed_k(labels, k, penalty=-1, device=None):
    """Fixed_k.ipynb's test_scores: (mean F1@k, mean DCG@k); k an int or the notebook's [k_f1, k_dcg]."""
    return _curves(labels, penalty, device).fixed_k(k)


def greedy_k(train_labels, test_labels, penalty=-1, device=None):
    """Greedy_k.ipynb's greedy_scores: k* = the first maximum of the train split's mean F1 (DCG) curve over k = 0..S, then the
    test split's mean F1 (DCG) at k*.  Returns (F1, DCG, k_F1, k_DCG); an F1 cut of k* = 0 gives F1 = 0."""
    k_f1, k_dcg = _curves(train_labels, penalty, device).best_k()
    f1, dcg = _curves(test_labels, penalty, device).fixed_k((k_f1, k_dcg))
    return f1, dcg, k_f1, k_dcg


def score_threshold(train_scores, train_labels, test_scores, test_labels, thresholds, penalty=-1, device=None):
    """The tuned score-threshold baseline: every list is cut after its leading positions whose retrieval score is >= theta (a
    list whose first score is below theta keeps nothing and earns 0).  theta_F1 (theta_DCG) = the first of `thresholds` (at
    most 64) with the best mean F1 (DCG) on the training split, then the test split's mean F1 (DCG) there.  scores, labels:
    (B, S) in rank order.  Returns (F1, DCG, theta_F1, theta_DCG)."""
    from utils.sweep import CutSweep
    dev = _dev(device)
    sweeps = []
    for scores, labels in ((train_scores, train_labels), (test_scores, test_labels)):
        y = _labels(labels, dev)
        v = _labels(scores, dev)
        sweeps.append(CutSweep(y.shape[1], "score", thresholds, penalty, device=dev).update(v, y))
    train, test = sweeps
    th_f1, th_dcg = train.best("f1")[0], train.best("dcg")[0]
    return test.at(th_f1)["f1"], test.at(th_dcg)["dcg"], th_f1, th_dcg
