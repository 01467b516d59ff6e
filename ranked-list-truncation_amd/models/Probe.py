"""ProbeBase and Probe on the HIP hot path - drop-in for the reference's models/Probe.py:56-123.

ProbeBase is MMOECut (models/MMOECut.py) with its intermediates returned; Probe holds the six probe towers that read them."""
from torch import nn

from .MMOECut import Expert, MMOECut, TowerClass, TowerCut, TowerRerank
from ._probe import probe_forward, probe_loss

__all__ = ["Expert", "TowerCut", "TowerClass", "TowerRerank", "ProbeBase", "Probe"]


class ProbeBase(MMOECut):
    """models/Probe.py:56-99: int(num_tasks) gates and always the towers [Class, Rerank (softmax), Cut]; forward returns
    (experts_in (B,S,2*encoding_size), experts_o [(B,S,d_model)] per expert, towers [(B,S,1)] - one per gate, as the
    reference's zip gives), batch-major views of the position-major tensors forward_pm returns."""

    def __init__(self, seq_len: int = 300, num_experts=2, num_tasks=3, input_size=3, encoding_size=128, d_model=256,
                 n_head=4, num_layers=1, dropout=0.2, attention_axis="list", attention_mask="none"):
        super().__init__(seq_len, num_experts, num_tasks, input_size, encoding_size, d_model, n_head, num_layers, dropout,
                         attention_axis, attention_mask)
        if num_tasks != 3:
            self.towers = nn.ModuleList([TowerClass(d_model), TowerRerank(d_model), TowerCut(d_model)])

    def forward(self, x):
        h, expert_out, outs = self.forward_pm(x)
        B, S = x.shape[0], x.shape[1]

        def bm(t):
            return t.view(S, B, t.shape[-1]).transpose(0, 1)
        return bm(h), [bm(e) for e in expert_out], outs


class Probe(nn.Module):
    """models/Probe.py:102-122: probes c1 / r1 on the BiLSTM output, ce1 / re1 on expert 0, ce2 / re2 on expert 1."""

    def __init__(self, encoding_size=128, d_model=256) -> None:
        super().__init__()
        self.probe_c1 = TowerClass(d_model=encoding_size * 2)
        self.probe_r1 = TowerRerank(d_model=encoding_size * 2)
        self.probe_ce1 = TowerClass(d_model=d_model)
        self.probe_ce2 = TowerClass(d_model=d_model)
        self.probe_re1 = TowerRerank(d_model=d_model)
        self.probe_re2 = TowerRerank(d_model=d_model)

    def groups(self):
        """The probes by the feature tensor they read: experts_in, expert 0, expert 1 (one fused pass each)."""
        return ([self.probe_c1, self.probe_r1], [self.probe_ce1, self.probe_re1], [self.probe_ce2, self.probe_re2])

    def forward(self, experts_in, experts_o):
        """Batch-major frozen features -> (probe_c1, probe_r1, probe_ce1, probe_ce2, probe_re1, probe_re2), (B,S,1) each."""
        c1, r1 = probe_forward([self.probe_c1, self.probe_r1], experts_in)
        ce1, re1 = probe_forward([self.probe_ce1, self.probe_re1], experts_o[0])
        ce2, re2 = probe_forward([self.probe_ce2, self.probe_re2], experts_o[1])
        return c1, r1, ce1, ce2, re1, re2

    def losses(self, features_pm, labels, S, B, margin=5e-4, want_out=True):
        """The six probes' losses on the three position-major feature tensors (experts_in, expert 0, expert 1): three fused
        passes.  Returns {name: (loss (0-d), activations (B,S,1) or None)} with the reference's probe names."""
        res = {}
        names = (("c1", "r1"), ("ce1", "re1"), ("ce2", "re2"))
        for heads, x_pm, nm in zip(self.groups(), features_pm, names):
            loss, outs = probe_loss(heads, x_pm, labels, S, B, margin, want_out)
            for i, n in enumerate(nm):
                res[n] = (loss[i], None if outs is None else outs[i])
        return res
