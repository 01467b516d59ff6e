"""Streaming truncation: a ranked list arrives a page of ranks at a time and the model says, page by page, whether to stop.

`StreamingTruncator` drives a position-axis, causal, hazard-head Choopy without ever holding the whole list: every encoder layer
keeps a K/V cache of the ranks seen so far (ops.encoder_layer_append over rlt_seq_attention_append), the hazard head carries its
survival sum from page to page and takes the stop decision on the device (ops.hazard_head_append), and a list that has stopped
is retired: its attention, head and decision work is skipped from the next page on.  The chunk's GEMMs and LayerNorms still run
over all C*B rows - compacting the batch is not done.  Inference only: eval mode, no dropout, no gradient."""
import torch

from rlt_hip import native as N
from rlt_hip import ops


class StreamingTruncator:
    """model: a Choopy with attention_axis='position', attention_mask='causal', cut_head='hazard' (model.stream builds this and
    checks it); tau: the stop threshold of truncate(rule='above'); batch_size: the number of lists streamed side by side.

    push(scores) consumes the next C ranks of every list and returns device tensors; it reads nothing back to the host."""

    def __init__(self, model, tau, batch_size):
        missing = [f"{name}={want!r}" for name, want in (("attention_axis", "position"), ("attention_mask", "causal"), ("cut_head", "hazard"))
                   if getattr(model, name, None) != want]
        if missing or not hasattr(model, "position_encoding"):
            raise ValueError(f"StreamingTruncator needs a Choopy built with {', '.join(missing) or 'a position encoding'}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        self.model, self.tau, self.B = model, float(tau), int(batch_size)
        self.seq_len, self.n_head = model.seq_len, model.n_head
        dev = model.position_encoding.device
        if dev.type != "cuda":
            raise RuntimeError("the HIP models run on the GPU only: move the model to 'cuda' before model.stream (no CPU fallback exists)")
        self.E = model.position_encoding.shape[1] + 1
        self.layers = list(model.attention_layer.layers.children())
        # one (seq_len*B, 2E) K | V cache per layer; never initialised: the append kernel reads only what it wrote
        self.caches = [torch.empty((self.seq_len * self.B, 2 * self.E), dtype=torch.float32, device=dev) for _ in self.layers]
        self.carry = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self.active = torch.ones(self.B, dtype=torch.int32, device=dev)
        self.k = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._read = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.position = 0

    def reset(self):
        """Start new lists: position 0, every list active, k = 0.  The caches are reused as they are."""
        self.carry.zero_()
        self.active.fill_(1)
        self.k.zero_()
        self._read.zero_()
        self.position = 0

    def push(self, scores):
        """scores: (B, C) or (B, C, 1), the retrieval scores of ranks position .. position+C-1, any C >= 1.  ->
        {'stop': (B, C) fp32 stop probabilities of the chunk (NaN rows for the lists retired before this call),
         'active': (B,) bool, 'k': (B,) int32 - the 1-based cut of a stopped list, 0 while undecided}.
        The chunk that reaches seq_len ends the lists: every list still active stops at its last rank."""
        if scores.dim() == 2:
            scores = scores.unsqueeze(2)
        if scores.dim() != 3 or scores.shape[0] != self.B or scores.shape[2] != 1 or scores.shape[1] < 1:
            raise ValueError(f"push: scores must be ({self.B}, C) or ({self.B}, C, 1) with C >= 1, got {tuple(scores.shape)}")
        if not scores.is_cuda:
            raise RuntimeError("the HIP models run on the GPU only: move the scores to 'cuda' (no CPU fallback exists)")
        C, t0 = int(scores.shape[1]), self.position
        if t0 + C > self.seq_len:
            raise ValueError(f"push: ranks {t0} .. {t0 + C - 1} go past seq_len = {self.seq_len}")
        model = self.model
        with torch.no_grad():
            self._read += self.active * C                      # a list that is active on entry reads this page
            h = ops.choopy_embed(N.f32c(scores), model.position_encoding[t0:t0 + C])
            for layer, cache in zip(self.layers, self.caches):
                h = ops.encoder_layer_append(h, layer, cache, t0, self.seq_len, self.B, self.n_head, self.active)
            lin = getattr(model.decison_layer, "0")
            off = model.hazard_offset(self.seq_len, h.device)
            out = ops.hazard_head_append(h, lin.weight, lin.bias, t0, self.B, self.carry, tau=self.tau, final=t0 + C == self.seq_len,
                                         active=self.active, k=self.k, offset=None if off is None else off[t0:t0 + C])
        self.position = t0 + C
        return {"stop": out["stop"], "active": self.active != 0, "k": self.k.clone()}

    def documents_read(self):
        """(B,) int32 on the device: the ranks each list has consumed - whole pages up to and including the page of its stop."""
        return self._read.clone()
