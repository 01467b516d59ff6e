"""What a trained model does with a split: per-query cuts and the curves of the reference's `--draw` figure, on the HIP hot path.

`CutReport` streams a split through `rlt_cut_report` batch by batch: one fused pass per batch over the model's output and the
labels yields each list's cut k, the winning value and its margin, F1@k / DCG@k, the list's best F1 / DCG with their
cuts and the number of cuts that would have been rewarded better, and adds the batch into the split's histogram of k and into
the two curves `Trainer.plot` draws (run.py:242-298): the mean softmax of the per-position reward, softmax_j(r_j / tau), and the
mean sharpened softmax of the model's output, softmax_j(p_j / (tau * 1e-3)).  Both softmaxes subtract the row maximum and are
formed in float64, so they stay finite where the reference's fp32 exp(p / 9e-4) overflows (any p above about 0.08).  Labels are
optional: without them only k, the winning value, the margin, the histogram and the prediction curve exist.

The host synchronises only when arrays or Python numbers are asked for.  GPU only, like utils/metrics.py.
"""
import numpy as np
import torch

from rlt_hip import native as N
from rlt_hip import ops

_METRICS = {"f1": N.METRIC_F1, "dcg": N.METRIC_DCG}


class CutReport:
    """Running report over lists of S positions: update() with batches, then per_query() / curves() / summary()."""

    def __init__(self, S, metric="f1", penalty=-1.0, metric_penalty=-1.0, tau=0.9, sharpen=None, device=None, reward=None):
        S = int(S)
        if not 1 <= S <= 1024:
            raise ValueError(f"list length {S} outside 1..1024")
        if metric not in _METRICS:
            raise ValueError(f"metric {metric!r}: one of {sorted(_METRICS)}")
        if not torch.cuda.is_available():
            raise RuntimeError("utils.report runs on the GPU (HIP kernels); no CPU fallback exists")
        self.S, self.metric = S, metric
        self.penalty, self.metric_penalty = float(penalty), float(metric_penalty)
        self.tau = float(tau)
        self.sharpen = self.tau * 1e-3 if sharpen is None else float(sharpen)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # reward: a RewardSpec (or its text form) - every list's cut is also valued in that reward (rlt_reward_eval)
        self.reward = None
        if reward is not None:
            from utils.rewards import RewardSpec
            self.reward = RewardSpec.parse(reward)
        self._acc = None
        self._racc = None
        self._parts = []
        self._n = 0
        self._labelled = None

    def update(self, output, labels=None):
        """output: a model's output - (B,S,1) / (B,S), BiCut's (B,S,2), or a multi-task model's list whose last entry is the cut
        distribution; labels (B,S) or None.  A report is either labelled throughout or label-free throughout."""
        cut = output[-1] if isinstance(output, (list, tuple)) else output
        if self._labelled is None:
            self._labelled = labels is not None
        elif self._labelled != (labels is not None):
            raise ValueError("a CutReport takes labels with every batch or with none")
        if cut.shape[1] != self.S:
            raise ValueError(f"lists of {cut.shape[1]} positions, this report holds {self.S}")
        if cut.shape[0] == 0:
            return self
        cut = cut.detach().to(self.device, non_blocking=True)
        if labels is not None:
            labels = torch.as_tensor(labels).to(self.device, non_blocking=True)
        per, self._acc = ops.cut_report(cut, labels, _METRICS[self.metric], self.penalty, self.metric_penalty, self.tau,
                                        self.sharpen, acc=self._acc)
        if self.reward is not None and labels is not None:
            # the k the pass above just wrote goes straight back in: device memory, no host read
            ev, self._racc = ops.reward_eval(N.f32c(labels), self.reward, k=per["k"], allow_empty=False, acc=self._racc)
            per.update({"reward": ev["r_at"].reshape(-1), "best_reward": ev["best"], "best_reward_k": ev["best_k"],
                        "better_reward": ev["better"].reshape(-1)})
        self._parts.append(per)
        self._n += int(cut.shape[0])
        return self

    @property
    def n_lists(self):
        return self._n

    def _need(self):
        if not self._n:
            raise ValueError("no lists have been added")

    def per_query(self):
        """{name: numpy array over the lists in the order they were added}: k, p_k, margin and, with labels, f1, dcg, best_f1,
        best_f1_k, best_dcg, best_dcg_k, better; with `reward=` also reward (the reward at k), best_reward, best_reward_k (the
        list's best over k = 1..S and its first position) and better_reward (cuts 1..S that earn strictly more)."""
        self._need()
        return {n: torch.cat([p[n] for p in self._parts]).cpu().numpy() for n in self._parts[0]}

    def curves(self, tail_fix=True):
        """(reward curve, prediction curve), each (S,) float64 numpy, normalised as `Trainer.plot` draws them: the mean over the
        lists.  tail_fix applies the figure's `norm_s[-3:] = norm_s[-4]` (run.py:283) to the prediction curve (lists of at
        least four positions).  The reward curve is None for a label-free report."""
        self._need()
        pred = (self._acc["pred_curve"] / self._n).cpu().numpy()
        if tail_fix and self.S >= 4:
            pred[-3:] = pred[-4]
        reward = (self._acc["reward_curve"] / self._n).cpu().numpy() if self._labelled else None
        return reward, pred

    def histogram(self):
        """Counts of k = 0..S, (S+1,) float64 numpy."""
        self._need()
        return self._acc["hist"].cpu().numpy()

    def summary(self):
        """Means over the lists: f1, dcg, best_f1, best_dcg, regret_f1 / regret_dcg (best - achieved), best_cut_share_f1 /
        best_cut_share_dcg (share of lists cut at their first-best position), mean_k, plus n and the k histogram."""
        self._need()
        hist = self.histogram()
        out = {"n": self._n, "hist": hist.tolist(), "mean_k": float((hist * np.arange(self.S + 1)).sum() / self._n)}
        if self._labelled:
            s = self._acc["sums"].tolist()
            n = s[4]
            q = self.per_query()
            out.update({"f1": s[0] / n, "dcg": s[1] / n, "best_f1": s[2] / n, "best_dcg": s[3] / n,
                        "regret_f1": (s[2] - s[0]) / n, "regret_dcg": (s[3] - s[1]) / n,
                        "best_cut_share_f1": float(np.mean(q["k"] == q["best_f1_k"])),
                        "best_cut_share_dcg": float(np.mean(q["k"] == q["best_dcg_k"]))})
            if self._racc is not None:
                r = self._racc["sums"].tolist()         # lists, sum best, clamped cuts, sum reward, #(reward == best), sum better
                out.update({"reward_spec": self.reward_text(), "reward": r[3] / r[0], "best_reward": r[1] / r[0],
                            "regret_reward": (r[1] - r[3]) / r[0], "best_cut_share_reward": r[4] / r[0],
                            "better_reward": r[5] / r[0]})
        return out

    def reward_text(self):
        """str(spec) of the report's reward, None without one (a reward with its own discounts: its repr)."""
        if self.reward is None:
            return None
        try:
            return str(self.reward)
        except ValueError:
            return repr(self.reward)
