"""Reward losses on the HIP hot path - drop-in for the criteria of the reference's utils/losses.py
that are on the hot path: ChoopyLoss :48-68, AttnCutLoss :71-96, RerankLoss :99-141,
MtCutLoss :164-191, DivLoss :194-233, BiCutLoss :11-45 and WassDistLoss :236-311 (section 8f row N4).  Same constructor signatures; `criterion(output, labels)`
returns a 0-d tensor supporting .backward() and .item().  PairwiseRankLoss (RankNet / LambdaRank on the rerank head) has no
counterpart there; MtCutLoss takes it in place of the hinge with `rerank_loss=`.

The reference builds its (B,S) reward matrix with B*S python calls of O(S) tensor ops; here the
reward matrix, its softmax, the divergence and d(loss)/d(output) come out of ONE kernel pass
(`rlt_reward_loss`), one ranked list per wavefront or per half wavefront.

`metric=` is 'f1' or 'dcg' (that pass, unchanged), or any other cut reward: a utils.rewards.RewardSpec, or a string its
parse() understands ('fbeta:2', 'ndcg', 'ndcg:-0.5', 'gain:-1,1,3[:norm]'), which goes through `rlt_reward_any_loss`.
RewardMatrixLoss takes a reward matrix of the caller's instead of labels.
"""
import torch
from torch import nn

from rlt_hip import native as N
from rlt_hip import ops
from utils.rewards import RewardSpec


def _metric_code(metric):
    return N.METRIC_F1 if metric == 'f1' else N.METRIC_DCG      # anything else => DCG (utils/losses.py:218-225)


def _spec(metric):
    """The RewardSpec of a `metric=` argument, None for 'f1' / 'dcg' (and whatever else _metric_code takes as DCG)."""
    return RewardSpec.parse(metric) if RewardSpec.is_spec(metric) else None


def _reward_loss(p, y, metric, kind, tau, with_metrics=False, owner=None):
    """The criterion on today's F1 / DCG pass, or on rlt_reward_any_loss for any other reward.  with_metrics: (loss, k, sums)
    with sums = [sum F1@k, sum DCG@k]: from the same pass for 'f1' / 'dcg' (RewardLossFn); for a RewardSpec the pass yields k
    and the REWARD statistics - left in `owner.last_reward_sums`, (4) float64 = [sum r_k, sum r_best, lists cut at their best
    reward, B] - and F1@k / DCG@k come from the existing metric call on that k."""
    spec = _spec(metric)
    if spec is None:
        if with_metrics:
            return ops.RewardLossFn.apply(p, y, _metric_code(metric), kind, tau, -1.0, True)
        return ops.RewardLossFn.apply(p, y, _metric_code(metric), kind, tau)
    if not with_metrics:
        return ops.RewardAnyLossFn.apply(p, y, spec, None, kind, tau)
    loss, k, _r_k, _r_best, _best_k, rsums = ops.RewardAnyLossFn.apply(p, y, spec, None, kind, tau, True)
    if owner is not None:
        owner.last_reward_sums = rsums
    return loss, k, ops.cut_metrics(p.detach(), y, k_in=k)[3]


def _prep(output, labels):
    N.require_cuda(output, labels)
    if output.dim() != 3 or output.shape[2] != 1:
        raise ValueError(f"expected a (B,S,1) cut distribution, got {tuple(output.shape)}")
    return N.f32c(output), N.f32c(labels)


class ChoopyLoss(nn.Module):
    def __init__(self, metric: str = 'f1'):
        super().__init__()
        self.metric = metric

    def forward(self, output, labels):
        p, y = _prep(output, labels)
        return _reward_loss(p, y, self.metric, N.LOSS_EXPECT, 1.0)

    def forward_with_metrics(self, output, labels):
        """(loss, k, [sum F1@k, sum DCG@k]) from one kernel pass (utils.metrics.Metric.step)."""
        p, y = _prep(output, labels)
        return _reward_loss(p, y, self.metric, N.LOSS_EXPECT, 1.0, True, self)


class AttnCutLoss(nn.Module):
    def __init__(self, metric: str = 'f1', tau: float = 0.95):
        super().__init__()
        self.metric, self.tau = metric, tau

    def forward(self, output, labels):
        p, y = _prep(output, labels)
        return _reward_loss(p, y, self.metric, N.LOSS_CE, float(self.tau))

    def forward_with_metrics(self, output, labels):
        p, y = _prep(output, labels)
        return _reward_loss(p, y, self.metric, N.LOSS_CE, float(self.tau), True, self)


class DivLoss(nn.Module):
    def __init__(self, metric: str = 'f1', tau: float = 0.85, div_type: str = 'kl', augmented: bool = True):
        super().__init__()
        self.metric, self.div_type, self.augmented = metric, div_type, augmented
        self.tau = tau if augmented else 1.

    def forward(self, output, labels):
        p, y = _prep(output, labels)
        kind = N.LOSS_KL if self.div_type == 'kl' else N.LOSS_JS
        return _reward_loss(p, y, self.metric, kind, float(self.tau))

    def forward_with_metrics(self, output, labels):
        p, y = _prep(output, labels)
        kind = N.LOSS_KL if self.div_type == 'kl' else N.LOSS_JS
        return _reward_loss(p, y, self.metric, kind, float(self.tau), True, self)


class RerankLoss(nn.Module):
    """Batch-wide hinge between mean irrelevant and mean relevant score.  A batch without
    positives (or without negatives) gives a zero loss with zero gradients (the reference's intent,
    utils/losses.py:138; under torch>=2 the reference itself raises there)."""

    def __init__(self, margin: float = 5e-4, reduction: str = 'mean'):
        super().__init__()
        self.margin, self.reduction = margin, reduction

    def forward(self, output, labels):
        s, y = _prep(output, labels)
        return ops.RerankLossFn.apply(s, y, float(self.margin))


RERANK_LOSSES = ('hinge', 'ranknet', 'lambdarank')


class PairwiseRankLoss(nn.Module):
    """Pairwise logistic ranking loss over the documents of each list (rlt_pair_rank_loss): 'ranknet' - the mean of
    softplus(-sigma (s_i - s_j)) over the pairs with grade_i > grade_j - or 'lambdarank' - their sum, each pair weighted by
    |gain_i - gain_j| |D(rank_i) - D(rank_j)| (divided by the list's ideal DCG with `normalize`), the weights held constant in
    the gradient.  The batch loss is the mean over lists; a list without such a pair gives 0.  gains: gain per grade (its length
    is n_grades), None = 2^g - 1 over `n_grades` grades; labels are rounded to grades as utils.rewards.RewardSpec does.
    forward(output, labels): output (B,S,1) or (B,S) scores, labels (B,S)."""

    def __init__(self, kind: str = 'lambdarank', sigma: float = 1.0, gains=None, n_grades: int = 2, normalize: bool = True):
        super().__init__()
        ops._pair_rank_args(kind, sigma, gains, n_grades)           # raises on anything the library would refuse
        self.kind, self.sigma, self.normalize = kind, float(sigma), bool(normalize)
        self.gains = None if gains is None else tuple(float(g) for g in gains)
        self.n_grades = int(n_grades) if gains is None else len(self.gains)

    def forward(self, output, labels):
        N.require_cuda(output, labels)
        if not (output.dim() == 2 or (output.dim() == 3 and output.shape[2] == 1)):
            raise ValueError(f"expected (B,S,1) or (B,S) scores, got {tuple(output.shape)}")
        return ops.PairRankLossFn.apply(N.f32c(output), N.f32c(labels), self.kind, self.sigma, self.gains, self.n_grades,
                                        self.normalize)


class MtCutLoss(nn.Module):
    def __init__(self, metric: str = 'f1', rerank_weight: float = 0.5, classi_weight: float = 0.5,
                 num_tasks: float = 3, rerank_loss: str = 'hinge', rerank_sigma: float = 1.0):
        super().__init__()
        if rerank_loss not in RERANK_LOSSES:
            raise ValueError(f"rerank_loss must be one of {RERANK_LOSSES}, got {rerank_loss!r}")
        self.rerank_weight, self.classi_weight = rerank_weight, classi_weight
        # 'hinge': the reference's batch-wide RerankLoss, on exactly the path it always took; 'ranknet' / 'lambdarank': a
        # PairwiseRankLoss on the rerank head in its place (binary relevance, label >= 0.5, as the hinge and the BCE see it)
        self.rerank_loss = rerank_loss
        self.pairloss = None if rerank_loss == 'hinge' else PairwiseRankLoss(kind=rerank_loss, sigma=rerank_sigma)
        # the reference registers this (unused) parameter too (utils/losses.py:173): kept for
        # state_dict / RNG-consumption compatibility
        self.weights = nn.Parameter(torch.randn(int(num_tasks)), requires_grad=True)
        self.cutloss = DivLoss(metric=metric, div_type='js', augmented=True)
        self.rerankloss = RerankLoss()
        self.num_tasks = num_tasks
        self.metric = metric

    def _apply(self, output, labels, with_metrics):
        y_class = y_rerank = None
        if self.num_tasks == 3:
            y_class, y_rerank, y_cut = output
        elif self.num_tasks == 2.1:
            y_class, y_cut = output
        else:
            y_rerank, y_cut = output
        p, y = _prep(y_cut, labels)
        rr = None if y_rerank is None else N.f32c(y_rerank)
        cl = None if y_class is None else N.f32c(y_class)
        if self.pairloss is not None and rr is not None:
            # cut term + w_r * pair loss + w_c * BCE, added on the tape in that order; the BCE from the multi-task pass
            # without a rerank input, the cut term on whichever pass the metric selects
            cut = _reward_loss(p, y, self.metric, N.LOSS_JS, float(self.cutloss.tau), with_metrics, self)
            total = (cut[0] if with_metrics else cut) + float(self.rerank_weight) * self.pairloss(rr, y)
            if cl is not None:
                total = total + ops.MtSideLossFn.apply(None, cl, y, float(self.rerank_weight), float(self.classi_weight),
                                                       float(self.rerankloss.margin))
            return (total,) + tuple(cut[1:]) if with_metrics else total
        if _spec(self.metric) is not None:
            # any other reward: the cut term on rlt_reward_any_loss, the rerank hinge and the BCE from the multi-task pass with a
            # zero cut term of its own, added on the tape in the reference's order (cut + w_r * hinge + w_c * bce)
            cut = _reward_loss(p, y, self.metric, N.LOSS_JS, float(self.cutloss.tau), with_metrics, self)
            side = ops.MtSideLossFn.apply(rr, cl, y, float(self.rerank_weight), float(self.classi_weight),
                                          float(self.rerankloss.margin))
            return (cut[0] + side,) + tuple(cut[1:]) if with_metrics else cut + side
        return ops.MtCutLossFn.apply(p, rr, cl, y, _metric_code(self.metric), float(self.cutloss.tau),
                                     float(self.rerank_weight), float(self.classi_weight),
                                     float(self.rerankloss.margin), with_metrics)

    def forward(self, output, labels):
        return self._apply(output, labels, False)

    def forward_with_metrics(self, output, labels):
        return self._apply(output, labels, True)


class RewardMatrixLoss(nn.Module):
    """The reward losses on a reward matrix of the caller's: forward(output, r) with r (B,S), r[b,k-1] the value of cutting list b
    after position k, finite.  kind: 'expect' (ChoopyLoss), 'ce' (AttnCutLoss), 'kl' or 'js' (DivLoss); q = softmax(r / tau).
    No gradient flows into r."""

    KINDS = {'expect': N.LOSS_EXPECT, 'ce': N.LOSS_CE, 'kl': N.LOSS_KL, 'js': N.LOSS_JS}

    def __init__(self, kind: str = 'js', tau: float = 0.85):
        super().__init__()
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {sorted(self.KINDS)}, got {kind!r}")
        if not tau > 0:
            raise ValueError(f"tau must be positive, got {tau!r}")
        self.kind, self.tau = kind, float(tau)

    def _apply(self, output, r, with_stats):
        p, r = _prep(output, r)
        if r.shape != p.shape[:2]:
            raise ValueError(f"expected a {tuple(p.shape[:2])} reward matrix, got {tuple(r.shape)}")
        return ops.RewardAnyLossFn.apply(p, None, None, r.detach(), self.KINDS[self.kind], self.tau, with_stats)

    def forward(self, output, r):
        return self._apply(output, r, False)

    def forward_with_stats(self, output, r):
        """(loss, k, stats) as the spec losses' forward_with_metrics."""
        loss, k, r_k, r_best, best_k, sums = self._apply(output, r, True)
        return loss, k, {"r_k": r_k, "r_best": r_best, "best_k": best_k, "sums": sums}


class BiCutLoss(nn.Module):
    """utils/losses.py:11-45 on the (B,S,2) output of BiCut; the position mask, the label-dependent reward pairs, the sum
    and d(loss)/d(output) come out of one kernel pass (`rlt_bicut_loss`)."""

    def __init__(self, alpha: float = 0.65, r: float = 0.0971134020, metric: str = 'nci'):
        super().__init__()
        self.metric, self.alpha, self.r = metric, alpha, r

    def forward(self, output, labels):
        N.require_cuda(output, labels)
        if output.dim() != 3 or output.shape[2] != 2:
            raise ValueError(f"expected the (B,S,2) output of BiCut, got {tuple(output.shape)}")
        return ops.BiCutLossFn.apply(N.f32c(output), N.f32c(labels), self.metric == 'nci', float(self.alpha), float(self.r))


class WassDistLoss(nn.Module):
    """utils/losses.py:236-311 (Sinkhorn distance between the batch's cut distributions and its label vectors); `metric`
    and `tau` are accepted and unused, as in the reference."""

    def __init__(self, eps: float = 1e-3, max_iter: int = 100, metric: str = 'f1', tau: float = 0.95, reduction='mean'):
        super().__init__()
        self.eps, self.max_iter, self.reduction = eps, max_iter, reduction     # one (B,B) problem: mean == sum

    def forward(self, output, labels):
        p, y = _prep(output, labels)
        B, S = y.shape
        return ops.WassDistLossFn.apply(p.reshape(B, S), y, float(self.eps), int(self.max_iter), 1e-1)
