"""Rerank, then truncate: does re-ranking with an auxiliary head and then cutting beat cutting the retrieval order?

The multi-task models score every document with a rerank head (and, in the 3 / 2.1-task forms, a per-document classifier).
`RerankedEval` streams a split through batch by batch: `ops.rerank_lists` sorts every list by the head's values (descending,
stable, NaNs last: np.argsort(-v, kind="stable")) and carries the labels along, and the SAME accumulators the rest of the
package uses - `CutReport`, `TruncationCurves`, `RewardCurves`, `CutSweep` - are driven twice, once with the labels in the
retrieval order and once with the re-ranked labels.  The model's cut k is the same number in both columns: the model decides how
many documents to keep, the head decides which ones come first.  No evaluation arithmetic lives here.

The host synchronises only when figures are read.  GPU only, like utils/metrics.py.
"""
import numpy as np
import torch

from rlt_hip import native as N
from rlt_hip import ops
from utils.baselines import RewardCurves, TruncationCurves
from utils.report import CutReport
from utils.sweep import CutSweep

HEADS = ("rerank", "classi")
ORDERS = ("orig", "rr")                 # the retrieval order, the head's order


class _Column:
    """The accumulators of one order."""

    def __init__(self, S, metric, metric_penalty, reward, sweep, device):
        self.report = CutReport(S, metric=metric, metric_penalty=metric_penalty, device=device, reward=reward)
        self.curves = TruncationCurves(S, device, penalty=metric_penalty)
        self.rcurves = RewardCurves(S, reward, device) if reward is not None else None
        self.sweep = CutSweep(S, "score", sweep, penalty=metric_penalty, device=device, reward=reward) if sweep is not None else None

    def update(self, values, cut_p, labels):
        self.report.update(cut_p, labels)
        self.curves.update(labels)
        if self.rcurves is not None:
            self.rcurves.update(labels)
        if self.sweep is not None:
            self.sweep.update(values, labels)

    def figures(self, fixed_k, greedy_from):
        """Flat {name: Python number}: the report's means, Oracle, Fixed-k, Greedy-k, and the sweep's best threshold."""
        rep = self.report.summary()
        out = {name: rep[name] for name in ("f1", "dcg", "mean_k", "regret_f1", "regret_dcg")}
        out["best_cut_f1"], out["best_cut_dcg"] = self.curves.best_cut()
        for k in fixed_k:
            out[f"fixed_k{k}_f1"], out[f"fixed_k{k}_dcg"] = self.curves.fixed_k(k)
        k_f1, k_dcg = greedy_from.curves.best_k()
        out["greedy_k_kf1"], out["greedy_k_kdcg"] = k_f1, k_dcg
        out["greedy_k_f1"], out["greedy_k_dcg"] = self.curves.fixed_k((k_f1, k_dcg))
        if self.rcurves is not None:
            out["reward"], out["regret_reward"] = rep["reward"], rep["regret_reward"]
            out["best_cut_reward"] = self.rcurves.best_cut()
            for k in fixed_k:
                out[f"fixed_k{k}_reward"] = self.rcurves.fixed_k(k)
            k_r = greedy_from.rcurves.best_k()
            out["greedy_k_kreward"], out["greedy_k_reward"] = k_r, self.rcurves.fixed_k(k_r)
        if self.sweep is not None:
            tau, _, _ = greedy_from.sweep.best("reward" if self.rcurves is not None else self.report.metric)
            at = self.sweep.at(tau)
            out["sweep_tau"] = tau
            out.update({f"sweep_{name}": at[name] for name in ("k", "f1", "dcg") + (("reward",) if self.rcurves is not None else ())})
        return out


class RerankedEval:
    """Every evaluation figure of a split in two orders: the retrieval order and the order of an auxiliary head.

    S: the list length; by: 'rerank' | 'classi', the head whose values order the lists (recorded, not interpreted: the caller
    passes that head's output); metric, metric_penalty: as CutReport takes them (metric_penalty is also the DCG penalty of the
    baselines and the sweep); reward: a RewardSpec or its text form - every figure then also exists in that reward
    (rlt_reward_eval); fixed_k: the cuts of the Fixed-k rows; sweep: up to 64 thresholds - a CutSweep with the 'score' rule over
    the head values is then kept per order: in the head's order the values descend, so the rule is a label-free learned score
    threshold."""

    def __init__(self, S, by="rerank", metric="f1", metric_penalty=-1.0, reward=None, fixed_k=(5, 10, 50), sweep=None, device=None):
        if by not in HEADS:
            raise ValueError(f"by {by!r}: one of {HEADS}")
        S = int(S)
        if not 1 <= S <= 1024:
            raise ValueError(f"list length {S} outside 1..1024")
        if not torch.cuda.is_available():
            raise RuntimeError("utils.rerank runs on the GPU (HIP kernels); no CPU fallback exists")
        self.S, self.by = S, by
        self.fixed_k = tuple(int(k) for k in fixed_k if 0 <= int(k) <= S)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if reward is not None:
            from utils.rewards import RewardSpec
            reward = RewardSpec.parse(reward)
        self.reward = reward
        self._cols = {o: _Column(S, metric, float(metric_penalty), reward, sweep, self.device) for o in ORDERS}
        self._n = 0

    def update(self, head_values, cut_p, labels):
        """head_values: the head's output, (B,S) / (B,S,1); cut_p: the model's cut distribution in the retrieval order, as
        CutReport.update takes it; labels (B,S).  Adds the batch into both columns; no host read."""
        v = head_values.detach().to(self.device, non_blocking=True)
        if v.shape[1] != self.S:
            raise ValueError(f"lists of {v.shape[1]} positions, this evaluation holds {self.S}")
        if v.shape[0] == 0:
            return self
        v = v.reshape(v.shape[0], self.S)
        labels = N.f32c(torch.as_tensor(labels).to(self.device, non_blocking=True))
        want_sorted = self._cols["rr"].sweep is not None
        _, _, v_rr, (labels_rr,) = ops.rerank_lists(v, labels, want_perm=False, want_sorted=want_sorted)
        self._cols["orig"].update(v, cut_p, labels)
        self._cols["rr"].update(v_rr, cut_p, labels_rr)
        self._n += int(v.shape[0])
        return self

    @property
    def n_lists(self):
        return self._n

    def summary(self, train=None):
        """{'by', 'n', 'orig': {...}, 'rr': {...}, 'diff': {...}}: per order the means over the lists - f1, dcg, mean_k and the
        regrets at the model's k; best_cut_f1 / best_cut_dcg; fixed_k<k>_f1 / _dcg; greedy_k_* (k from `train`, a RerankedEval over
        the training split, order by order; without one the k is this split's own best: an in-sample figure); with a reward the
        same rows in it; with a sweep the figures at the best threshold (tuned on `train` likewise) - and rr - orig of each."""
        if not self._n:
            raise ValueError("no lists have been added")
        src = train if train is not None else self
        cols = {o: self._cols[o].figures(self.fixed_k, src._cols[o]) for o in ORDERS}
        diff = {name: cols["rr"][name] - cols["orig"][name] for name in cols["orig"]}
        return {"by": self.by, "n": self._n, "greedy_in_sample": train is None, "orig": cols["orig"], "rr": cols["rr"], "diff": diff}

    def per_query(self):
        """{name: numpy array over the lists in the order they were added}: k (the model's cut, the same in both orders), then
        f1, dcg, best_f1, best_k (the first cut that reaches best_f1) in the retrieval order and, with an `_rr` suffix, in the
        head's order; with a reward also reward and best_reward.  No permutation is kept: the arrays are per list, so they fit
        utils.compare.compare_reports as two systems on the same queries."""
        if not self._n:
            raise ValueError("no lists have been added")
        out = {}
        for o, suffix in zip(ORDERS, ("", "_rr")):
            q = self._cols[o].report.per_query()
            if not out:
                out["k"] = q["k"]
            names = {"f1": "f1", "dcg": "dcg", "best_f1": "best_f1", "best_f1_k": "best_k"}
            if self.reward is not None:
                names.update({"reward": "reward", "best_reward": "best_reward"})
            out.update({new + suffix: q[old] for old, new in names.items()})
        return out


def mean_over_lengths(summaries):
    """{length: RerankedEval.summary()} -> {'orig': {...}, 'rr': {...}}: the list-weighted means of f1 and dcg over the lengths."""
    n = sum(s["n"] for s in summaries.values())
    return {o: {m: float(np.sum([s[o][m] * s["n"] for s in summaries.values()]) / n) for m in ("f1", "dcg")} for o in ORDERS}
