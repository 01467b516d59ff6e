"""TaskC on the HIP hot path - drop-in for the reference's models/Classification.py:3-12 (a relevance-classification probe)."""
from torch import nn

from rlt_hip import native as N
from . import _common as C
from ._probe import probe_forward, probe_loss


class TaskC(nn.Module):
    probe_kind = N.PROBE_BCE       # Linear -> Sigmoid, trained with nn.BCELoss (verify_BMT.py:37-44)

    def __init__(self, d_model: int = 128) -> None:
        super().__init__()
        self.classification_layer = C.head_params(d_model)

    @property
    def linear(self):
        return getattr(self.classification_layer, "0")

    def forward(self, x):
        """x (B,S,d_model) frozen features -> class probabilities (B,S,1)."""
        return probe_forward([self], x)[0]

    def loss(self, x_pm, labels, S, B, want_out=True):
        """nn.BCELoss of the probe on position-major features (S*B,d_model): (loss (1,), [(B,S,1)] or None)."""
        return probe_loss([self], x_pm, labels, S, B, want_out=want_out)
