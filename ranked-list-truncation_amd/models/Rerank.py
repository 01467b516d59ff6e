"""TaskR on the HIP hot path - drop-in for the reference's models/Rerank.py:3-12 (a re-ranking probe)."""
from torch import nn

from rlt_hip import native as N
from . import _common as C
from ._probe import probe_forward, probe_loss


class TaskR(nn.Module):
    probe_kind = N.PROBE_RERANK    # Linear -> Softmax over the positions, trained with RerankLoss (verify_BMT.py:37-44)

    def __init__(self, d_model: int = 128) -> None:
        super().__init__()
        self.rerank_layer = C.head_params(d_model)

    @property
    def linear(self):
        return getattr(self.rerank_layer, "0")

    def forward(self, x):
        """x (B,S,d_model) frozen features -> re-ranking scores (B,S,1), a softmax over each list."""
        return probe_forward([self], x)[0]

    def loss(self, x_pm, labels, S, B, margin=5e-4, want_out=True):
        """RerankLoss of the probe on position-major features (S*B,d_model): (loss (1,), [(B,S,1)] or None)."""
        return probe_loss([self], x_pm, labels, S, B, margin, want_out)
