"""Probe heads on frozen features (the reference's probing study: models/Classification.py, models/Rerank.py,
models/Probe.py): one fused pass of rlt_probe_heads gives the activations, each head's loss and its weight gradients."""
import torch

from rlt_hip import ops
from . import _common as C


def probe_loss(heads, x_pm, labels, S, B, margin=5e-4, want_out=True):
    """Losses (n,) of the probe heads `heads` (modules with .linear and .probe_kind) on the frozen position-major features
    x_pm (S*B,E) against labels (B,S), and their activations [(B,S,1)] (None with want_out=False).  loss.sum().backward()
    fills each head's gradients of its own loss."""
    return ops.probe_heads(x_pm, [h.linear.weight for h in heads], [h.linear.bias for h in heads],
                           [h.probe_kind for h in heads], labels, S, B, margin, want_out)


def probe_forward(heads, x):
    """Activations of the probe heads on batch-major frozen features x (B,S,E): [(B,S,1)].  Not differentiable in x (the
    features are frozen); the weights' gradients come from probe_loss."""
    x = C.check_input(x.detach())
    B, S, _ = x.shape
    labels = torch.zeros((B, S), dtype=torch.float32, device=x.device)
    with torch.no_grad():
        return probe_loss(heads, ops.to_position_major(x), labels, S, B)[1]
