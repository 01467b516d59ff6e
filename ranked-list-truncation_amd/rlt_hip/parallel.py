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
`rlt_grad_norm` pass over the gradient bucket followed by `rlt_adam_step_guarded`, all decided on the device.  A learning-rate
schedule, per-tensor parameter groups, decoupled (AdamW) weight decay or averaged (EMA) weights switch the step to
`rlt_adam_step_recipe`, still one streaming pass over the bucket.
"""
import contextlib
import ctypes
import fnmatch
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


class LRSchedule:
    """Linear warm-up over `warmup_steps` applied steps to the optimizer's lr, then `kind`: 'constant', or a 'linear' / 'cosine' decay
    to lr * min_lr_ratio at applied step `total_steps`, where it stays (include/rlt_hip.h, rlt_adam_step_recipe).  The device
    evaluates it from its own applied-step count; lr_at is the same expression on the host, for logging."""

    def __init__(self, kind="constant", warmup_steps=0, total_steps=0, min_lr_ratio=0.0):
        if kind not in N.SCHED_KINDS:
            raise ValueError(f"unknown schedule kind {kind!r}: one of {N.SCHED_KINDS}")
        self.kind, self.warmup_steps, self.total_steps, self.min_lr_ratio = kind, int(warmup_steps), int(total_steps), float(min_lr_ratio)
        if self.warmup_steps < 0 or not 0.0 <= self.min_lr_ratio <= 1.0:
            raise ValueError("warmup_steps must be >= 0 and min_lr_ratio in [0, 1]")
        if kind != "constant" and self.total_steps <= self.warmup_steps:
            raise ValueError(f"a {kind} decay needs total_steps ({self.total_steps}) > warmup_steps ({self.warmup_steps})")

    def fields(self):
        return dict(sched_kind=self.kind, warmup_steps=self.warmup_steps, total_steps=self.total_steps, min_lr_ratio=self.min_lr_ratio)

    def lr_at(self, t, base_lr=1.0):
        """The float64 schedule value at applied step t >= 1 for the base rate `base_lr` (rlt_lr_at; the step uses it rounded to
        float); with the default base rate, the schedule's factor."""
        return N.lr_at(N.recipe_struct(base_lr=base_lr, **self.fields()), t)


def resolve_param_groups(names, param_groups, weight_decay):
    """[(lr_scale, weight_decay)] per name of `names`: param_groups is a list of (pattern, {"lr_scale": f, "weight_decay": f}),
    matched with fnmatch; the first matching pattern wins, a key it leaves out and an unmatched name get (1, weight_decay).  A
    pattern that matches no name at all raises: a typo would otherwise train silently with the defaults."""
    out, used = [], [False] * len(param_groups)
    for _, opts in param_groups:
        if set(opts) - {"lr_scale", "weight_decay"}:
            raise ValueError(f"unknown parameter-group options {sorted(set(opts) - {'lr_scale', 'weight_decay'})}")
    for name in names:
        hits = [i for i, (pat, _) in enumerate(param_groups) if fnmatch.fnmatchcase(name, pat)]
        for i in hits:
            used[i] = True
        opts = param_groups[hits[0]][1] if hits else {}
        out.append((float(opts.get("lr_scale", 1.0)), float(opts.get("weight_decay", weight_decay))))
    unused = [param_groups[i][0] for i, u in enumerate(used) if not u]
    if unused:
        raise ValueError(f"parameter-group pattern(s) {unused} match no parameter; the names are {list(names)}")
    return out


class FusedAdam:
    """torch.optim.Adam(lr, betas, eps, weight_decay) on a FlatModel, one HIP launch per step.

    max_grad_norm / skip_nonfinite / segment_norms (all off by default: step() is then the one rlt_adam_step launch) switch to
    the guarded step: rlt_grad_norm over flat_grad - the bucket's norm, the clip coefficient of torch's clip_grad_norm_, the
    non-finite count and, with segment_norms, the figures of every parameter tensor - followed by rlt_adam_step_guarded, which
    applies the coefficient inside the update (flat_grad itself is left unclipped) and, with skip_nonfinite, leaves the
    parameters and both moments untouched when the gradient holds a NaN or an Inf.  The step count then lives on the device;
    nothing is allocated per step and the host reads nothing until epoch_stats() / state_dict().

    schedule (an LRSchedule) / param_groups / decoupled_weight_decay / ema_decay (any of them) switch to the recipe step,
    rlt_adam_step_recipe, after rlt_grad_norm when a guard option is set: lr follows the schedule of the APPLIED steps, counted and
    evaluated on the device (a skipped step does not advance it); param_groups = [(name pattern, {"lr_scale": f, "weight_decay":
    f}), ...] gives the tensors of FlatModel.names their own learning-rate factor and weight decay (resolve_param_groups);
    decoupled_weight_decay is torch.optim.AdamW's decay; ema_decay keeps `ema`, an exponential moving average of the parameters
    updated in the same pass (with ema_warmup the decay is min(ema_decay, (1 + k) / (10 + k)) at the k-th update), which
    ema_weights() swaps into the model for evaluation.  Still no host read, no allocation and no host-advanced scalar per step.
    lr_scale 0 freezes a tensor: nothing of it is written.  It stays in the bucket and its gradient is still computed, so
    freezing saves no backward work."""

    def __init__(self, flat: FlatModel, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, skip_nonfinite=False, segment_norms=False,
                 schedule=None, param_groups=None, decoupled_weight_decay=False, ema_decay=None, ema_warmup=True):
        self.flat = flat
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(flat.flat_param)
        self.exp_avg_sq = torch.zeros_like(flat.flat_param)
        self.steps = 0
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.0
        self.skip_nonfinite, self.segment_norms = bool(skip_nonfinite), bool(segment_norms)
        self.guarded = self.max_grad_norm > 0.0 or self.skip_nonfinite or self.segment_norms
        self.recipe = schedule is not None or bool(param_groups) or bool(decoupled_weight_decay) or bool(ema_decay)
        dev = flat.flat_param.device
        if self.recipe:
            self.schedule = schedule if schedule is not None else LRSchedule()
            self.decoupled, self.ema_decay, self.ema_warmup = bool(decoupled_weight_decay), float(ema_decay or 0.0), bool(ema_warmup)
            if not 0.0 <= self.ema_decay < 1.0:
                raise ValueError(f"ema_decay {ema_decay} is outside [0, 1)")
            self.group_values = resolve_param_groups(flat.names, param_groups, weight_decay) if param_groups else None
            self.group_table = None if self.group_values is None else torch.tensor(self.group_values, dtype=torch.float32, device=dev)
            self.ema = flat.flat_param.clone() if self.ema_decay else None
            self.recipe_state = torch.zeros(N.RECIPE_STATE_WORDS, dtype=torch.int64, device=dev)
            self._recipe_struct = N.recipe_struct(
                base_lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay, decoupled=self.decoupled,
                ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, skip_nonfinite=self.skip_nonfinite, use_norm=self.guarded,
                **self.schedule.fields())
            self._ema_swapped = False
            if not self.guarded:
                self.opt_state = torch.zeros(N.OPT_STATE_WORDS, dtype=torch.int64, device=dev)
                self.totals = {"clipped": 0, "skipped": 0}
        if self.guarded:
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
        if self.recipe and self._ema_swapped:
            raise RuntimeError("step() inside ema_weights(): the bucket holds the averaged weights")
        if self.guarded:
            N.call("rlt_grad_norm", N.ptr(f.flat_grad), f.numel, N.ptr(f.offsets) if self.n_seg else None, self.n_seg,
                   self.max_grad_norm, N.ptr(self.ws), self.ws_bytes, N.ptr(self.seg_stats), N.ptr(self.opt_state), N.stream())
        if self.recipe:
            groups = self.group_table is not None
            N.call("rlt_adam_step_recipe", N.ptr(f.flat_param), N.ptr(f.flat_grad), N.ptr(self.exp_avg), N.ptr(self.exp_avg_sq),
                   N.ptr(self.ema), f.numel, N.ptr(f.offsets) if groups else None, N.ptr(self.group_table), len(f.names) if groups else 0,
                   N.ptr(self.opt_state), N.ptr(self.recipe_state), ctypes.byref(self._recipe_struct), N.stream())
            return
        if self.guarded:
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

    def _need_recipe(self, what):
        if not self.recipe:
            raise RuntimeError(f"{what} exists only with schedule, param_groups, decoupled_weight_decay or ema_decay set")

    def lr_at(self, t):
        """The schedule's float64 value at applied step t >= 1 for this optimizer's lr, on the host (rlt_lr_at)."""
        self._need_recipe("lr_at()")
        return N.lr_at(self._recipe_struct, t)

    def current_lr(self):
        """The float learning rate of the last applied step as a DEVICE tensor (a view of the recipe state: no copy, no
        synchronisation); 0 before the first step."""
        self._need_recipe("current_lr()")
        return self.recipe_state.view(torch.float32)[N.RECIPE_LR_F32]

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model computes with the averaged weights: flat_param and ema are exchanged in place (rlt_swap_f32
        - no scratch bucket, no allocation; the parameters are views of the bucket) and exchanged back on exit, also when the
        block raises.  Not re-entrant, and step() raises inside it."""
        self._need_recipe("ema_weights()")
        if self.ema is None:
            raise RuntimeError("ema_weights() needs ema_decay")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is not re-entrant")
        swap = lambda: N.call("rlt_swap_f32", N.ptr(self.flat.flat_param), N.ptr(self.ema), self.flat.numel, N.stream())
        swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            swap()
            self._ema_swapped = False

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
        two counters on the device; state_dict() keeps their totals.  `lr` is the learning rate of the last applied step (the
        constant one without a schedule).  On the recipe step it works without a guard option too: the norm figures are then
        NaN / 0.0 / 0."""
        if not self.recipe:
            self._need_guard()
        words = self.opt_state.clone()
        lr = self.recipe_state.clone() if self.recipe else None
        seg = self.seg_stats.clone() if self.segment_norms else None
        if reset:
            self.opt_state[N.OPT_NORM_SUM:N.OPT_NORM_STEPS + 1].zero_()
            self.opt_state[N.OPT_SKIPPED:N.OPT_CLIPPED + 1].zero_()
        words = words.cpu()                                     # the synchronisation
        f64 = words.view(torch.float64)
        n = int(words[N.OPT_NORM_STEPS])
        out = {"grad_norm_mean": float(f64[N.OPT_NORM_SUM]) / n if n else float("nan"), "grad_norm_max": float(f64[N.OPT_NORM_MAX]),
               "finite_steps": n, "clipped_steps": int(words[N.OPT_CLIPPED]), "skipped_steps": int(words[N.OPT_SKIPPED]),
               "lr": float(lr.view(torch.float32)[N.RECIPE_LR_F32]) if self.recipe else self.lr}
        if reset:
            self.totals["clipped"] += out["clipped_steps"]
            self.totals["skipped"] += out["skipped_steps"]
        if seg is not None:
            norms = seg.view(torch.float64)[:, 0].sqrt().cpu().tolist()
            out["segment_norms"] = dict(zip(self.flat.names, norms))
        return out

    def state_dict(self):
        if not (self.guarded or self.recipe):
            return {"steps": self.steps, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        words = self.opt_state.cpu()                            # the applied step count lives on the device
        out = {"steps": int(words[N.OPT_STEP]), "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
               "clipped_steps": self.totals["clipped"] + int(words[N.OPT_CLIPPED]),
               "skipped_steps": self.totals["skipped"] + int(words[N.OPT_SKIPPED])}
        if self.recipe:
            if self._ema_swapped:
                raise RuntimeError("state_dict() inside ema_weights(): ema holds the raw parameters there")
            out.update(ema=self.ema, recipe_state=self.recipe_state.cpu())
        return out

    def load_state_dict(self, sd):
        """Restore what state_dict() of an optimizer with the same options on a bucket of the same layout returned: both moments,
        the applied-step count (the host's, or the device word), ema and the recipe state, the clipped and skipped totals.  The
        running norm figures of the open epoch start over.  The tensors are copied: `sd` may be the live state of another
        optimizer or a loaded checkpoint on any device."""
        if sd["exp_avg"].numel() != self.exp_avg.numel():
            raise ValueError(f"the state holds {sd['exp_avg'].numel()} elements, the bucket {self.exp_avg.numel()}")
        if self.recipe and ((sd.get("ema") is None) != (self.ema is None) or "recipe_state" not in sd):
            raise ValueError("the state was not written by an optimizer with these schedule / group / EMA options")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if not (self.guarded or self.recipe):
            self.steps = int(sd["steps"])
            return
        self.opt_state.zero_()
        self.opt_state[N.OPT_STEP] = int(sd["steps"])
        self.totals = {"clipped": int(sd.get("clipped_steps", 0)), "skipped": int(sd.get("skipped_steps", 0))}
        if self.recipe:
            self.recipe_state.copy_(sd["recipe_state"])
            if self.ema is not None:
                self.ema.copy_(sd["ema"])


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
