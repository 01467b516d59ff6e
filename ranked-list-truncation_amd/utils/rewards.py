"""Cut rewards as values: what `metric=` of the reward losses (utils/losses.py) and `--criterion` of run.py accept beside
'f1' and 'dcg'.  A RewardSpec names a reward r[b,k] - the value of cutting list b after position k - that the library builds
from the labels in registers (rlt_reward_any_loss, csrc/reward_any.hip):

    RewardSpec.fbeta(2.0)                     F_beta of the cut: recall-heavy (beta > 1) or precision-heavy (beta < 1)
    RewardSpec.gain((-1, 1, 3))               graded gain: a document of grade g adds gain[g] * discount[j]
    RewardSpec.gain((0, 1), discount=d)       ... under the caller's discounts (S floats) instead of 1 / log2(j + 2)
    RewardSpec.gain((-1, 1, 3), normalize=True)   ... divided by the value of the list's ideal ordering
    RewardSpec.ndcg(-1.0)                     gain((penalty, 1), None, True): one tau means the same on every list
    RewardSpec.parse("fbeta:2" | "ndcg" | "ndcg:-0.5" | "gain:-1,1,3" | "gain:-1,1,3:norm")

The grade of a document is its label rounded to the nearest integer and clamped to 0..len(gains)-1.  Graded labels enter through
this interface only: the data loaders produce 0/1 labels, and the 'f1' / 'dcg' kernels test `label == 1`, where a grade 2
reads as non-relevant."""
import math

import torch

from rlt_hip import native as N

MAX_GRADES = N.REWARD_MAX_GRADES


class RewardSpec:
    def __init__(self, family, beta=1.0, gains=(), discount=None, normalize=False):
        self.family = family
        self.beta = float(beta)
        self.gains = tuple(float(g) for g in gains)
        self.normalize = bool(normalize)
        self.discount = None if discount is None else torch.as_tensor(discount, dtype=torch.float32).reshape(-1).clone()
        if family == N.REWARD_FBETA:
            if not (self.beta > 0.0 and math.isfinite(self.beta)):
                raise ValueError(f"fbeta needs a finite beta > 0, got {beta!r}")
        elif family == N.REWARD_GAIN:
            if not 2 <= len(self.gains) <= MAX_GRADES:
                raise ValueError(f"a gain reward takes 2..{MAX_GRADES} gains (one per grade), got {len(self.gains)}")
            if not all(math.isfinite(g) for g in self.gains):
                raise ValueError(f"gains must be finite, got {self.gains}")
        else:
            raise ValueError(f"unknown reward family {family!r}")
        self._device_discount = {}

    # ---- constructors ------------------------------------------------------------------------------------------------
    @classmethod
    def fbeta(cls, beta):
        return cls(N.REWARD_FBETA, beta=beta)

    @classmethod
    def gain(cls, gains, discount=None, normalize=False):
        return cls(N.REWARD_GAIN, gains=gains, discount=discount, normalize=normalize)

    @classmethod
    def ndcg(cls, penalty=-1.0):
        return cls.gain((penalty, 1.0), None, True)

    @classmethod
    def parse(cls, text):
        """'fbeta:<beta>' | 'ndcg' | 'ndcg:<penalty>' | 'gain:<g0>,<g1>[,...]' | 'gain:<g0>,<g1>[,...]:norm'."""
        if isinstance(text, cls):
            return text
        if not isinstance(text, str):
            raise ValueError(f"not a reward: {text!r}")
        head, _, rest = text.strip().partition(":")
        try:
            if head == "fbeta" and rest:
                return cls.fbeta(float(rest))
            if head == "ndcg":
                return cls.ndcg(float(rest)) if rest else cls.ndcg()
            if head == "gain" and rest:
                body, sep, flag = rest.partition(":")
                if sep and flag != "norm":
                    raise ValueError(flag)
                return cls.gain(tuple(float(g) for g in body.split(",")), None, bool(sep))
        except ValueError as e:
            raise ValueError(f"malformed reward {text!r}: {e}") from None
        raise ValueError(f"malformed reward {text!r}: expected fbeta:<beta>, ndcg[:<penalty>] or gain:<g0>,<g1>,...[:norm]")

    @classmethod
    def is_spec(cls, metric):
        """True for a RewardSpec and for a string in parse's grammar ('f1', 'dcg' and every other string: False)."""
        if isinstance(metric, cls):
            return True
        return isinstance(metric, str) and metric.strip().partition(":")[0] in ("fbeta", "ndcg", "gain")

    # ---- text form ---------------------------------------------------------------------------------------------------
    def __str__(self):
        """The string parse() reads back (a custom discount has no text form)."""
        if self.family == N.REWARD_FBETA:
            return f"fbeta:{self.beta!r}"
        if self.discount is not None:
            raise ValueError("a reward with its own discounts has no text form")
        if self.normalize and len(self.gains) == 2 and self.gains[1] == 1.0:
            return f"ndcg:{self.gains[0]!r}"
        return "gain:" + ",".join(repr(g) for g in self.gains) + (":norm" if self.normalize else "")

    def __repr__(self):
        if self.discount is None or self.family == N.REWARD_FBETA:
            return f"RewardSpec({str(self)!r})"
        return f"RewardSpec(gain={self.gains}, discount=<{self.discount.numel()} floats>, normalize={self.normalize})"

    def key(self):
        return (self.family, self.beta if self.family == N.REWARD_FBETA else None, self.gains, self.normalize,
                None if self.discount is None else tuple(self.discount.tolist()))

    def __eq__(self, other):
        return isinstance(other, RewardSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    # ---- the library's view -------------------------------------------------------------------------------------------
    def native(self, S, device):
        """-> (rlt_reward_spec struct for lists of S positions on `device`, the tensors it points into)."""
        disc = None
        if self.family == N.REWARD_GAIN and self.discount is not None:
            if self.discount.numel() < S:
                raise ValueError(f"the reward has {self.discount.numel()} discounts, the lists {S} positions")
            dkey = str(torch.device(device))
            if dkey not in self._device_discount:
                self._device_discount[dkey] = self.discount.to(device)
            disc = self._device_discount[dkey]
        return N.reward_spec_struct(self.family, self.beta, self.gains, self.normalize, disc), disc
