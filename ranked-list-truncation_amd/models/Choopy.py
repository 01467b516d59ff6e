"""Choopy on the HIP hot path - drop-in for the reference's models/Choopy.py:6-23."""
import torch
from torch import nn

from rlt_hip import ops
from . import _common as C


class Choopy(C.CutModel):
    def __init__(self, seq_len: int = 300, d_model: int = 128, n_head: int = 8, num_layers: int = 3, dropout=0.2,
                 attention_axis: str = "list", attention_mask: str = "none",
                 cut_head: str = "softmax", hazard_prior: str = "uniform"):
        super().__init__()
        self.attention_axis = C.check_attention_axis(attention_axis)
        self.attention_mask = C.check_attention_mask(attention_mask, attention_axis)
        self.cut_head, self.hazard_prior = C.check_cut_head(cut_head, hazard_prior)
        self.seq_len, self.n_head, self.dropout = seq_len, n_head, dropout
        self.position_encoding = nn.Parameter(torch.randn(seq_len, 127), requires_grad=True)
        self.attention_layer = C.encoder_params(d_model, n_head, num_layers, dropout)
        self.decison_layer = C.head_params(d_model)

    def forward(self, x):
        x = C.check_input(x)
        drop_p = C.check_dropout(self, self.dropout)
        B, S, _ = x.shape
        if S != self.seq_len:
            raise ValueError(f"Choopy was built for seq_len={self.seq_len}, got {S}")
        h = ops.choopy_embed(x, self.position_encoding)
        h = C.encoder(h, self.attention_layer, self.n_head, S, B, drop_p, self.attention_axis, self.attention_mask == "causal")
        return C.cut_head(self, h, S, B)

    def stream(self, tau, batch_size, compact_every=None, compact_below=1.0):
        """-> utils.stream.StreamingTruncator: the model fed a page of ranks at a time, stopping each list on the device at the
        first rank whose stop probability reaches tau (what truncate(rule='above', tau=tau) gives on the whole list).  Needs
        attention_axis='position', attention_mask='causal' and cut_head='hazard': anything else is a ValueError naming the option.
        compact_every=n takes the stopped lists out of the batch after every n-th page (None: never), compact_below is the live
        fraction at or below which that moves anything (StreamingTruncator.compact)."""
        for name, want, why in (("attention_axis", "position", "the list axis attends across the lists of a batch, not over ranks"),
                                ("attention_mask", "causal", "without the mask rank i attends to the ranks below it"),
                                ("cut_head", "hazard", "the softmax head normalises over the whole list")):
            if getattr(self, name) != want:
                raise ValueError(f"Choopy.stream needs {name}={want!r}, this model has {name}={getattr(self, name)!r}: {why}")
        from utils.stream import StreamingTruncator
        return StreamingTruncator(self, tau, batch_size, compact_every=compact_every, compact_below=compact_below)
