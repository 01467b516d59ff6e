"""Data-parallel training glue: flat parameter / gradient buckets, one RCCL all-reduce per step,
one fused Adam launch per step.

The reference is single-process (no torch.distributed anywhere).  Ranked lists
are independent apart from the list-axis attention and the batch-wide rerank hinge, which couple
the lists of ONE mini-batch; the multi-GPU semantics are therefore "shard-wise reference semantics"
(SURVEY.md section 8e): every rank runs the reference computation on its own sub-batch, losses are
averaged over ranks, i.e. gradients are averaged with ONE all-reduce of the flat fp32 bucket
(AttnCut: 1,846,785 params = 7.4 MB) over xGMI.  No collective sits on the data path.

`FlatModel` re-points every parameter (and its .grad) of an nn.Module at views of two flat fp32
buffers, so that zero_grad is one memset, the all-reduce is one collective on one buffer, and
`FusedAdam` (torch.optim.Adam semantics: coupled L2, bias correction; run.py:104) is one
`rlt_adam_step` launch - or, with gradient-norm clipping, the non-finite skip or per-parameter norms switched on, one
`rlt_grad_norm` pass over the gradient bucket followed by `rlt_adam_step_guarded`, all decided on the device.
"""
import os

import torch
import torch.distributed as dist

from . import native as N

# RLT_FORCE_DIST=1 (tests / one-GPU rehearsals): run every collective of the step even in a ONE-rank process group, so that
# the RCCL code path (all-reduce AVG on the flat bucket, parameter broadcast) executes on a one-GPU box.
FORCE_COLLECTIVES = os.environ.get("RLT_FORCE_DIST") == "1"


def _flat_view(buf, p):
    """`buf` (p.numel() elements of a flat bucket) seen with the parameter's OWN shape and strides: a plain view for a contiguous
    parameter; for a dense permuted one (BiCut's column-major layer-0 input weights) the same permutation over the slot, so that
    re-pointing the parameter does not silently make it row-major.  Adam is element-wise and does not care."""
    if p.is_contiguous():
        return buf.view(p.shape)
    order = sorted(range(p.dim()), key=lambda i: -p.stride(i))
    if not p.permute(order).is_contiguous():
        raise ValueError(f"parameter of shape {tuple(p.shape)} and strides {p.stride()} is not dense: it has no slot in a flat bucket")
    return buf.as_strided(p.shape, p.stride())


class FlatModel:
    def __init__(self, model: torch.nn.Module):
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError("model has no trainable parameters")
        dev = params[0].device
        # 4-float (16-byte) aligned slots so every view keeps the alignment the kernels want
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.numel = total
        self.params = params
        # the slots as a segment table for the per-parameter gradient norms (rlt_grad_norm): n_slots + 1 ascending offsets, the last
        # one = numel (a slot's padding up to 4 floats stays zero and belongs to it), and each slot's name for reporting
        self.offsets = torch.tensor(offs + [total], dtype=torch.int64, device=dev)
        by_id = {id(p): n for n, p in model.named_parameters()}
        self.names = [by_id[id(p)] for p in params]
        with torch.no_grad():
            for p, o in zip(params, offs):
                n = p.numel()
                view = _flat_view(self.flat_param[o:o + n], p)
                view.copy_(p.detach())
                grad = _flat_view(self.flat_grad[o:o + n], p)
                p.data = view
                p.grad = grad

    def zero_grad(self):
        """One memset; keeps the .grad views alive (autograd then accumulates in place)."""
        self.flat_grad.zero_()
        for p in self.params:          # a None grad would make autograd allocate a fresh tensor
            if p.grad is None or p.grad.data_ptr() < self.flat_grad.data_ptr():
                raise RuntimeError("a parameter lost its flat gradient view; use FlatModel.zero_grad(), "
                                   "not optimizer.zero_grad(set_to_none=True)")

    def all_reduce_grads(self, group=None):
        """Average the flat gradient bucket over the ranks (one collective)."""
        if not dist.is_available() or not dist.is_initialized():
            return
        world = dist.get_world_size(group)
        if world == 1 and not FORCE_COLLECTIVES:
            return
        if dist.get_backend(group) == "nccl":
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.AVG, group=group)     # RCCL over xGMI
        else:                                                                       # gloo (CPU tests, rehearsals)
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=group)
            self.flat_grad.mul_(1.0 / world)

    def broadcast_params(self, src=0, group=None):
        if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or FORCE_COLLECTIVES):
            dist.broadcast(self.flat_param, src=src, group=group)


class FusedAdam:
    """torch.optim.Adam(lr, betas, eps, weight_decay) on a FlatModel, one HIP launch per step.

    max_grad_norm / skip_nonfinite / segment_norms (all off by default: step() is then the one rlt_adam_step launch) switch to
    the guarded step: rlt_grad_norm over flat_grad - the bucket's norm, the clip coefficient of torch's clip_grad_norm_, the
    non-finite count and, with segment_norms, the figures of every parameter tensor - followed by rlt_adam_step_guarded, which
    applies the coefficient inside the update (flat_grad itself is left unclipped) and, with skip_nonfinite, leaves the
    parameters and both moments untouched when the gradient holds a NaN or an Inf.  The step count then lives on the device;
    nothing is allocated per step and the host reads nothing until epoch_stats() / state_dict()."""

    def __init__(self, flat: FlatModel, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, skip_nonfinite=False, segment_norms=False):
        self.flat = flat
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(flat.flat_param)
        self.exp_avg_sq = torch.zeros_like(flat.flat_param)
        self.steps = 0
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.0
        self.skip_nonfinite, self.segment_norms = bool(skip_nonfinite), bool(segment_norms)
        self.guarded = self.max_grad_norm > 0.0 or self.skip_nonfinite or self.segment_norms
        if self.guarded:
            dev = flat.flat_param.device
            self.n_seg = len(flat.params) if self.segment_norms else 0
            self.opt_state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device=dev)
            self.seg_stats = torch.zeros(max(self.n_seg, 1), N.GRAD_SEG_WORDS, dtype=torch.int64, device=dev)
            self.ws_bytes = N.query("rlt_grad_norm_workspace", flat.numel, self.n_seg)
            self.ws = N.byte_buffer(self.ws_bytes, dev)
            self.totals = {"clipped": 0, "skipped": 0}          # of the epochs that epoch_stats(reset=True) has closed

    def zero_grad(self):
        self.flat.zero_grad()

    def step(self):
        f = self.flat
        if not f.flat_param.is_cuda:
            raise RuntimeError("FusedAdam runs on the GPU (rlt_adam_step); no CPU fallback exists")
        if self.guarded:
            N.call("rlt_grad_norm", N.ptr(f.flat_grad), f.numel, N.ptr(f.offsets) if self.n_seg else None, self.n_seg,
                   self.max_grad_norm, N.ptr(self.ws), self.ws_bytes, N.ptr(self.seg_stats), N.ptr(self.opt_state), N.stream())
            N.call("rlt_adam_step_guarded", N.ptr(f.flat_param), N.ptr(f.flat_grad), N.ptr(self.exp_avg), N.ptr(self.exp_avg_sq),
                   f.numel, N.ptr(self.opt_state), self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                   int(self.skip_nonfinite), N.stream())
            return
        self.steps += 1
        N.call("rlt_adam_step", N.ptr(f.flat_param), N.ptr(f.flat_grad), N.ptr(self.exp_avg), N.ptr(self.exp_avg_sq),
               f.numel, self.steps, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, N.stream())

    def _need_guard(self):
        if not self.guarded:
            raise RuntimeError("gradient statistics exist only with max_grad_norm, skip_nonfinite or segment_norms set")

    def grad_stats(self):
        """The last step's figures as DEVICE tensors (views of the optimizer state: no copy, no synchronisation): norm, sumsq
        and max_abs float64, coef float32, nonfinite int64; with segment_norms also seg_sumsq, seg_max_abs (float64) and
        seg_nonfinite (int64), one entry per parameter tensor in the order of FlatModel.names."""
        self._need_guard()
        st, f64 = self.opt_state, self.opt_state.view(torch.float64)
        out = {"norm": f64[N.OPT_NORM], "sumsq": f64[N.OPT_SUMSQ], "max_abs": f64[N.OPT_MAX_ABS],
               "coef": st.view(torch.float32)[N.OPT_COEF_F32], "nonfinite": st[N.OPT_NONFINITE]}
        if self.segment_norms:
            seg64 = self.seg_stats.view(torch.float64)
            out.update(seg_sumsq=seg64[:, 0], seg_nonfinite=self.seg_stats[:, 1], seg_max_abs=seg64[:, 2])
        return out

    def epoch_stats(self, reset=True):
        """The one host read: mean and maximum gradient norm over the steps since the last reset whose gradient was finite
        (NaN / 0.0 when there was none), the number of those steps, the clipped and skipped steps since the last reset and, with
        segment_norms, the last step's norm of every parameter tensor by name.  reset=True zeroes the running figures and the
        two counters on the device; state_dict() keeps their totals."""
        self._need_guard()
        words = self.opt_state.clone()
        seg = self.seg_stats.clone() if self.segment_norms else None
        if reset:
            self.opt_state[N.OPT_NORM_SUM:N.OPT_NORM_STEPS + 1].zero_()
            self.opt_state[N.OPT_SKIPPED:N.OPT_CLIPPED + 1].zero_()
        words = words.cpu()                                     # the synchronisation
        f64 = words.view(torch.float64)
        n = int(words[N.OPT_NORM_STEPS])
        out = {"grad_norm_mean": float(f64[N.OPT_NORM_SUM]) / n if n else float("nan"), "grad_norm_max": float(f64[N.OPT_NORM_MAX]),
               "finite_steps": n, "clipped_steps": int(words[N.OPT_CLIPPED]), "skipped_steps": int(words[N.OPT_SKIPPED])}
        if reset:
            self.totals["clipped"] += out["clipped_steps"]
            self.totals["skipped"] += out["skipped_steps"]
        if seg is not None:
            norms = seg.view(torch.float64)[:, 0].sqrt().cpu().tolist()
            out["segment_norms"] = dict(zip(self.flat.names, norms))
        return out

    def state_dict(self):
        if not self.guarded:
            return {"steps": self.steps, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        words = self.opt_state.cpu()                            # the applied step count lives on the device
        return {"steps": int(words[N.OPT_STEP]), "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "clipped_steps": self.totals["clipped"] + int(words[N.OPT_CLIPPED]),
                "skipped_steps": self.totals["skipped"] + int(words[N.OPT_SKIPPED])}


def shard_batch(x, y, rank, world):
    """Equal contiguous shards of a global batch (the lists of one shard attend to each other)."""
    n = x.shape[0]
    if n % world:
        raise ValueError(f"global batch {n} is not divisible by world size {world}")
    per = n // world
    return x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per]


def shard_bounds(n, rank, world):
    """[lo, hi) of rank's contiguous shard of an n-list batch when n need not divide: the first n % world ranks take one
    list more; a rank may get an empty shard (n < world).  The shards of all ranks partition range(n) exactly."""
    per, extra = divmod(n, world)
    lo = rank * per + min(rank, extra)
    return lo, lo + per + (1 if rank < extra else 0)
