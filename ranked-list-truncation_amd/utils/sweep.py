"""Where on the effectiveness / cost trade-off to cut: threshold cut rules and their curve, on the HIP hot path.

Every model cuts a list at the mode of its cut distribution (BiCut by its pair rule).  `CutSweep` evaluates T thresholds of one
of three rules at once instead, streaming a split through `rlt_cut_sweep` batch by batch (one fused pass per batch over the
values and the labels, no host read):

  'quantile'  values = a cut distribution; k = the smallest cut whose predicted mass reaches the share tau
  'above'     values = a per-position stop probability (BiCut's class-0 column); k = the first position with value >= tau
  'score'     values = retrieval scores; k = the number of leading positions with score >= tau (0 keeps nothing)

and `curve()` gives, per threshold, the mean cut length (the cost), mean F1 / DCG / precision / recall / F_beta at the cut and
the share of lists left uncut.  `tune_cut_rule` picks tau* on a training split and reports a test split there.  The host
synchronises only when the curve is read.  GPU only, like utils/metrics.py.
"""
import numpy as np
import torch

from rlt_hip import native as N
from rlt_hip import ops

METRICS = ("f1", "dcg", "precision", "recall", "fbeta")
REWARD = "reward"               # the metric name of a sweep that was given a reward spec


def parse_sweep(spec):
    """'RULE:LO:HI:N' -> (rule, N thresholds from LO to HI inclusive as a float64 numpy array), RULE quantile | above | score;
    'score:auto:N' -> ('score', N): N quantiles of the training split's scores, chosen by the caller.  ValueError otherwise."""
    parts = str(spec).split(":")
    if parts[0] not in ("quantile", "above", "score"):
        raise ValueError(f"--cut-sweep {spec!r}: the rule is one of quantile, above, score")
    try:
        if len(parts) == 3 and parts[1] == "auto":
            if parts[0] != "score":
                raise ValueError("auto thresholds exist for the score rule only")
            n = int(parts[2])
            thresholds = n
        elif len(parts) == 4:
            lo, hi, n = float(parts[1]), float(parts[2]), int(parts[3])
            if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
                raise ValueError("LO and HI must be finite with LO <= HI")
            thresholds = np.linspace(lo, hi, n) if n >= 1 else None
        else:
            raise ValueError("expected RULE:LO:HI:N or score:auto:N")
        if not 1 <= n <= N.SWEEP_MAX_T:
            raise ValueError(f"N must be in 1..{N.SWEEP_MAX_T}")
    except ValueError as e:
        raise ValueError(f"--cut-sweep {spec!r}: {e}") from None
    return parts[0], thresholds


def score_quantiles(scores, n):
    """n thresholds for the score rule: the i / (n + 1) quantiles, i = 1..n, of all the scores of a split (host, float64)."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    return np.quantile(s, np.arange(1, n + 1) / (n + 1.0))


class CutSweep:
    """Running effectiveness / cost curve of T thresholds of one cut rule over lists of S positions."""

    def __init__(self, S, rule, thresholds, penalty=-1, beta=1, device=None, reward=None):
        S = int(S)
        if not 1 <= S <= 1024:
            raise ValueError(f"list length {S} outside 1..1024")
        if not torch.cuda.is_available():
            raise RuntimeError("utils.sweep runs on the GPU (HIP kernels); no CPU fallback exists")
        self.rule = ops.sweep_rule(rule)
        th = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        if th.ndim != 1 or not 1 <= th.size <= N.SWEEP_MAX_T:
            raise ValueError(f"{th.size} thresholds, outside 1..{N.SWEEP_MAX_T}")
        self.S, self.thresholds = S, th.copy()
        self.penalty, self.beta = float(penalty), float(beta)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._thr = torch.from_numpy(self.thresholds).to(self.device)
        # reward: a RewardSpec (or its text form) - the (B,T) cuts of every batch are also valued in it (rlt_reward_eval)
        self.reward = None
        if reward is not None:
            from utils.rewards import RewardSpec
            self.reward = RewardSpec.parse(reward)
        self._curve = None
        self._racc = None
        self._n = 0

    def update(self, values, labels):
        """values: (B,S) / (B,S,1), BiCut's (B,S,2) (read at stride 2 without a copy), or a multi-task model's list whose last
        entry is the cut distribution; labels (B,S).  Adds the batch into the curve; no host read."""
        v = values[-1] if isinstance(values, (list, tuple)) else values
        if v.shape[1] != self.S:
            raise ValueError(f"lists of {v.shape[1]} positions, this sweep holds {self.S}")
        if v.shape[0] == 0:
            return self
        v = v.detach().to(self.device, non_blocking=True)
        labels = torch.as_tensor(labels).to(self.device, non_blocking=True)
        k, self._curve = ops.cut_sweep(v, self._thr, self.rule, labels, self.penalty, self.beta, curve=self._curve,
                                       want_k=self.reward is not None)
        if self.reward is not None:             # the sweep's cuts go straight back in: device memory, no host read
            _, self._racc = ops.reward_eval(N.f32c(labels), self.reward, k=k, allow_empty=True, acc=self._racc, per_list=False)
        self._n += int(v.shape[0])
        return self

    @property
    def n_lists(self):
        return self._n

    def sums(self):
        """The (8,T) float64 sums over the lists as the pass leaves them (native.SWEEP_ROWS), numpy: one host read."""
        if not self._n:
            raise ValueError("no lists have been added")
        return self._curve.cpu().numpy()

    def curve(self):
        """{thresholds, k, f1, dcg, precision, recall, fbeta, uncut}: per threshold the means over the lists ((T,) float64 numpy;
        uncut = the share of lists with k = S), and n = the number of lists."""
        s = self.sums()
        n = s[7]
        out = {"thresholds": self.thresholds.copy(), "n": self._n}
        for i, name in enumerate(N.SWEEP_ROWS[:7]):
            out[name] = s[i] / n
        if self._racc is not None:
            r = self._racc["sums"].cpu().numpy()            # lists, sum best, clamped cuts, then 3 per threshold
            out[REWARD] = r[3::3] / r[0]
            out["best_reward"] = float(r[1] / r[0])
        return out

    def _metrics(self):
        return METRICS + ((REWARD,) if self.reward is not None else ())

    def best(self, metric="f1"):
        """(tau*, its index, the mean `metric` there): the first maximum over the thresholds in the order they were given."""
        if metric not in self._metrics():
            raise ValueError(f"metric {metric!r}: one of {self._metrics()}")
        row = self.curve()[metric]
        i = int(np.argmax(row))
        return float(self.thresholds[i]), i, float(row[i])

    def at(self, tau):
        """The curve's figures at the threshold `tau` (one of those given): dict of Python floats."""
        hit = np.nonzero(self.thresholds == float(tau))[0]
        if hit.size == 0:
            raise ValueError(f"{tau} is not one of this sweep's thresholds")
        c = self.curve()
        i = int(hit[0])
        return {"tau": float(self.thresholds[i]), "index": i, **{n: float(c[n][i]) for n in N.SWEEP_ROWS[:7]},
                **({REWARD: float(c[REWARD][i])} if self.reward is not None else {})}


def tune_cut_rule(train_batches, test_batches, rule, thresholds, S=None, metric="f1", penalty=-1, beta=1, device=None, reward=None):
    """Pick tau* on the training split, report the test split there.  train_batches / test_batches: iterables of (values,
    labels) as CutSweep.update takes them.  Returns a dict: tau, index, train (the figures at tau* on the training split), test
    (on the test split), train_curve and test_curve (CutSweep.curve()).  reward: a RewardSpec - tau* is then picked on the mean
    reward of the cuts (`metric` is 'reward'), and every figure gains a `reward` entry beside the F1 / DCG / F_beta ones."""
    if reward is not None:
        metric = REWARD
    elif metric not in METRICS:
        raise ValueError(f"metric {metric!r}: one of {METRICS}")
    sweeps = []
    for batches in (train_batches, test_batches):
        sw = None
        for values, labels in batches:
            if sw is None:
                v = values[-1] if isinstance(values, (list, tuple)) else values
                sw = CutSweep(v.shape[1] if S is None else S, rule, thresholds, penalty, beta, device, reward=reward)
            sw.update(values, labels)
        if sw is None or not sw.n_lists:
            raise ValueError("tune_cut_rule: a split without lists")
        sweeps.append(sw)
    train, test = sweeps
    tau, i, _ = train.best(metric)
    return {"rule": rule, "metric": metric, "tau": tau, "index": i, "train": train.at(tau), "test": test.at(tau),
            "train_curve": train.curve(), "test_curve": test.curve()}
