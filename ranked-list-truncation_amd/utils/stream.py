"""Streaming truncation: a ranked list arrives a page of ranks at a time and the model says, page by page, whether to stop.

`StreamingTruncator` drives a position-axis, causal, hazard-head Choopy without ever holding the whole list: every encoder layer
keeps a K/V cache of the ranks seen so far (ops.encoder_layer_append over rlt_seq_attention_append), the hazard head carries its
survival sum from page to page and takes the stop decision on the device (ops.hazard_head_append), and a list that has stopped
is retired: its attention, head and decision work is skipped from the next page on.  The chunk's GEMMs and LayerNorms run over
C * (slots of the batch) rows: by default the slots are the B lists the stream started with, retired or not; with `compact_every`
the retired lists are taken OUT of the batch (ops.stream_compact_plan, ops.kv_cache_compact), the slots are the live lists alone,
and a stopped list costs nothing from then on.  The public results stay in the caller's list order either way.  Inference only:
eval mode, no dropout, no gradient."""
import torch

from rlt_hip import native as N
from rlt_hip import ops


class StreamingTruncator:
    """model: a Choopy with attention_axis='position', attention_mask='causal', cut_head='hazard' (model.stream builds this and
    checks it); tau: the stop threshold of truncate(rule='above'); batch_size: the number of lists streamed side by side.
    compact_every: None never compacts - push launches what it always launched -, n calls compact() after every n-th push;
    compact_below: compact() moves only when the live lists are at most this fraction of the slots.

    push(scores) consumes the next C ranks of every list and returns device tensors; it reads nothing back to the host.  compact()
    reads one int32 back: that is the only host read of a stream."""

    def __init__(self, model, tau, batch_size, compact_every=None, compact_below=1.0):
        missing = [f"{name}={want!r}" for name, want in (("attention_axis", "position"), ("attention_mask", "causal"), ("cut_head", "hazard"))
                   if getattr(model, name, None) != want]
        if missing or not hasattr(model, "position_encoding"):
            raise ValueError(f"StreamingTruncator needs a Choopy built with {', '.join(missing) or 'a position encoding'}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if compact_every is not None and int(compact_every) < 1:
            raise ValueError(f"compact_every must be None or a positive number of pushes, got {compact_every}")
        if not 0.0 <= float(compact_below) <= 1.0:
            raise ValueError(f"compact_below must lie in [0, 1], got {compact_below}")
        self.model, self.tau, self.B = model, float(tau), int(batch_size)
        self.compact_every, self.compact_below = None if compact_every is None else int(compact_every), float(compact_below)
        self.seq_len, self.n_head = model.seq_len, model.n_head
        dev = model.position_encoding.device
        if dev.type != "cuda":
            raise RuntimeError("the HIP models run on the GPU only: move the model to 'cuda' before model.stream (no CPU fallback exists)")
        self.E = model.position_encoding.shape[1] + 1
        self.layers = list(model.attention_layer.layers.children())
        # one (seq_len*B, 2E) K | V cache per layer; never initialised: the append kernel reads only what it wrote
        self._buffers = [torch.empty((self.seq_len * self.B, 2 * self.E), dtype=torch.float32, device=dev) for _ in self.layers]
        self._spare = None                 # one more buffer of that size, shared by the layers: allocated by the first compaction;
                                           # a compaction rotates it through _buffers
        self.carry = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self.active = torch.ones(self.B, dtype=torch.int32, device=dev)
        self._k = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._read = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._start()

    def _start(self):
        # the slots of the batch: `slots` of them, slot j holding list origin[j] (None: the identity, nothing was compacted);
        # carry, active and _k are per SLOT, _read and _k_full per list; a layer's cache is the leading rows of its buffer
        self.slots, self._origin, self._origin_long, self._k_full = self.B, None, None, None
        self.caches = list(self._buffers)
        self.position, self._pushes, self._rows = 0, 0, 0

    def reset(self):
        """Start new lists: position 0, the full batch and the identity slot map, every list active, k = 0.  The cache buffers
        (and the spare one, once a compaction has allocated it) are reused as they are."""
        if self._origin is None:
            self.carry.zero_()
            self.active.fill_(1)
            self._k.zero_()
        else:
            dev = self._read.device
            self.carry = torch.zeros(self.B, dtype=torch.float64, device=dev)
            self.active = torch.ones(self.B, dtype=torch.int32, device=dev)
            self._k = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._read.zero_()
        self._start()

    @property
    def k(self):
        """(B,) int32 in list order: the 1-based cut of a stopped list, 0 while undecided.  Before any compaction this IS the array
        the head writes; after one it is put together from the cuts the retired lists handed over and those of the slots."""
        if self._origin is None:
            return self._k
        k = self._k_full.clone()
        if self.slots:
            k[self._origin_long] = self._k
        return k

    def push(self, scores, live_only=False):
        """scores: (B, C) or (B, C, 1), the retrieval scores of ranks position .. position+C-1 of all B lists in the caller's order,
        any C >= 1 (the rows of the live lists are selected on the device); with live_only=True (B_live, C) or (B_live, C, 1): the
        rows of live_lists() alone, in that order, for a caller that no longer fetches the pages of stopped lists.  ->
        {'stop': (B, C) fp32 stop probabilities of the chunk (NaN rows for the lists retired before this call),
         'active': (B,) bool, 'k': (B,) int32 - the 1-based cut of a stopped list, 0 while undecided}, in list order.
        The chunk that reaches seq_len ends the lists: every list still active stops at its last rank.  Once every list has been
        compacted away a push launches nothing and returns the final k."""
        if scores.dim() == 2:
            scores = scores.unsqueeze(2)
        rows = self.slots if live_only else self.B
        if scores.dim() != 3 or scores.shape[0] != rows or scores.shape[2] != 1 or scores.shape[1] < 1:
            raise ValueError(f"push: scores must be ({rows}, C) or ({rows}, C, 1) with C >= 1, got {tuple(scores.shape)}")
        if not scores.is_cuda:
            raise RuntimeError("the HIP models run on the GPU only: move the scores to 'cuda' (no CPU fallback exists)")
        C, t0 = int(scores.shape[1]), self.position
        if t0 + C > self.seq_len:
            raise ValueError(f"push: ranks {t0} .. {t0 + C - 1} go past seq_len = {self.seq_len}")
        model, Bs = self.model, self.slots
        compacted = self._origin is not None
        if compacted and not live_only and Bs:
            scores = scores.index_select(0, self._origin_long)
        stop = None
        with torch.no_grad():
            if Bs:
                if compacted:
                    self._read.index_add_(0, self._origin_long, self.active * C)
                else:
                    self._read += self.active * C              # a list that is active on entry reads this page
                h = ops.choopy_embed(N.f32c(scores), model.position_encoding[t0:t0 + C])
                for layer, cache in zip(self.layers, self.caches):
                    h = ops.encoder_layer_append(h, layer, cache, t0, self.seq_len, Bs, self.n_head, self.active)
                lin = getattr(model.decison_layer, "0")
                off = model.hazard_offset(self.seq_len, h.device)
                stop = ops.hazard_head_append(h, lin.weight, lin.bias, t0, Bs, self.carry, tau=self.tau, final=t0 + C == self.seq_len,
                                              active=self.active, k=self._k, offset=None if off is None else off[t0:t0 + C])["stop"]
            self.position = t0 + C
            self._pushes += 1
            self._rows += C * Bs
            if compacted:                                      # back to list order: tiny (B,) scatters
                full = torch.full((self.B, C), float("nan"), dtype=torch.float32, device=self._read.device)
                active = torch.zeros(self.B, dtype=torch.bool, device=self._read.device)
                if Bs:
                    full[self._origin_long] = stop
                    active[self._origin_long] = self.active != 0
                res = {"stop": full, "active": active, "k": self.k}
            else:
                res = {"stop": stop, "active": self.active != 0, "k": self._k.clone()}
            if self.compact_every is not None and self._pushes % self.compact_every == 0:
                self.compact()
        return res

    def compact(self):
        """Take the retired lists out of the batch.  -> the number of live lists (a host int).

        One rlt_stream_compact_plan launch builds the slot map, gathers the carry and hands the cuts of the retired slots over to
        the list-order k; then its n_live is read back - a 4-byte copy, the ONLY host read of a whole stream (push reads nothing).
        Only if n_live <= compact_below * (slots now) and n_live < slots now does anything move: one rlt_kv_cache_compact per layer
        gathers the ranks seen so far into a spare buffer (layer 0 into the spare, whose old buffer is the spare of layer 1, and so
        on: ONE extra buffer of the original cache size for all layers, allocated here the first time), and the truncator switches
        to the compacted slot arrays.  With nothing retired the call is the plan launch and the read.  A compaction moves the live
        part of the caches, at most compact_below of what the one before left: with compact_below = 0.5 the bytes moved over a
        whole stream are bounded by the size of the caches, 1/2 + 1/4 + .. of it."""
        Bs = self.slots
        if Bs == 0:
            return 0
        with torch.no_grad():
            if self._k_full is None:
                self._k_full = torch.zeros(self.B, dtype=torch.int32, device=self._read.device)
            plan = ops.stream_compact_plan(self.active, self._origin, self.carry, self._k, self._k_full)
            n_live = int(plan["n_live"].item())
            if n_live >= Bs or n_live > self.compact_below * Bs:
                return n_live
            if n_live and self.position:
                if self._spare is None:
                    self._spare = torch.empty_like(self._buffers[0])
                for i, cache in enumerate(self.caches):
                    ops.kv_cache_compact(cache, self._spare, plan["slot_src"], self.position, Bs, n_live)
                    self._spare, self._buffers[i] = self._buffers[i], self._spare
            self.caches = [b[:self.seq_len * n_live] for b in self._buffers]
            self.slots = n_live
            self._origin = plan["origin"][:n_live]
            self._origin_long = self._origin.long()
            self.carry = plan["carry"][:n_live]
            self.active = torch.ones(n_live, dtype=torch.int32, device=self._read.device)
            self._k = torch.zeros(n_live, dtype=torch.int32, device=self._read.device)
        return n_live

    def live_lists(self):
        """(B_live,) int32 on the device: the original numbers of the lists that hold a slot, ascending - the rows push(live_only=True)
        takes.  Before any compaction these are all B lists."""
        if self._origin is None:
            return torch.arange(self.B, dtype=torch.int32, device=self._read.device)
        return self._origin.clone()

    def rows_computed(self):
        """A host int, no device read: the sum over the pushes of C * (slots at that push) - the rows the chunk's GEMMs and LayerNorms
        ran over."""
        return self._rows

    def documents_read(self):
        """(B,) int32 on the device: the ranks each list has consumed - whole pages up to and including the page of its stop."""
        return self._read.clone()
