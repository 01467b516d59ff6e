"""The training-recipe flags of run.py, verify_probe.py and verify_BMT.py - learning-rate schedule, parameter groups, AdamW, averaged
weights - turned into FusedAdam's keyword arguments (rlt_hip/parallel.py, rlt_adam_step_recipe)."""
import fnmatch

from rlt_hip.parallel import LRSchedule

# --adamw 1 without --no-decay: biases (nn.Linear's, the LSTM's bias_ih_l0 ..., in_proj_bias), LayerNorm gains and biases and
# Choopy's position embedding are not decayed; a default pattern that matches nothing in the model at hand is dropped
DEFAULT_NO_DECAY = "*bias*,*norm*,position_encoding"


def add_recipe_arguments(p, ema_eval=True):
    """The recipe flags; ema_eval=False for a driver that has no evaluation with the averaged weights (no --ema-eval there)."""
    p.add_argument('--lr-schedule', type=str, default=None, choices=('constant', 'linear', 'cosine'),
                   help="learning rate over the APPLIED optimizer steps (evaluated on the device; a skipped step does not advance "
                        "it): linear warm-up, then constant, or a linear / cosine decay to --min-lr-ratio * lr at the last step")
    p.add_argument('--warmup-steps', type=int, default=0, help="warm-up length in steps")
    p.add_argument('--warmup-frac', type=float, default=0.0, help="warm-up length as a share of the run's steps (instead of --warmup-steps)")
    p.add_argument('--min-lr-ratio', type=float, default=0.0, help="floor of the decay as a share of lr")
    p.add_argument('--adamw', type=int, default=0, choices=(0, 1), help="1: decoupled weight decay (torch.optim.AdamW)")
    p.add_argument('--no-decay', type=str, default=None, metavar='PATTERNS',
                   help="comma-separated name patterns (fnmatch on the parameter names) trained with weight decay 0; default with "
                        "--adamw 1: " + DEFAULT_NO_DECAY.replace('%', '%%'))
    p.add_argument('--freeze', type=str, default=None, metavar='PATTERNS',
                   help="comma-separated name patterns whose tensors are not updated (their gradients are still computed)")
    p.add_argument('--lr-scale', type=str, default=None, metavar='PATTERN=F[,PATTERN=F...]', help="per-tensor learning-rate factors")
    p.add_argument('--ema-decay', type=float, default=0.0, help="D in (0, 1): keep an exponential moving average of the parameters")
    if ema_eval:
        p.add_argument('--ema-eval', type=int, default=0, choices=(0, 1),
                       help="1: test, report, sweep and save with the averaged weights (needs --ema-decay)")


def _patterns(spec):
    return [s.strip() for s in (spec or "").split(",") if s.strip()]


def _matching(names, patterns, flag, required=True):
    """names matched by any of `patterns`; a pattern of a flag the user gave that matches nothing raises."""
    hit = set()
    for pat in patterns:
        found = [n for n in names if fnmatch.fnmatchcase(n, pat)]
        if not found and required:
            raise ValueError(f"{flag}: pattern {pat!r} matches no parameter; the names are {list(names)}")
        hit.update(found)
    return hit


def recipe_kwargs(args, names, total_steps):
    """FusedAdam's keyword arguments for the recipe flags; empty with all of them at their defaults (the plain or the guarded
    step).  `names`: FlatModel.names; `total_steps`: epochs * steps per epoch.  The flags compose per tensor - a tensor may be
    both scaled and undecayed - so the groups are handed over as one exact-name entry per tensor that leaves the defaults;
    --freeze wins over --lr-scale, the first matching --lr-scale pattern wins."""
    get = lambda k, d=None: getattr(args, k, d)                 # (drivers build their own Namespace)
    out = {}
    kind, w_steps, w_frac = get("lr_schedule"), int(get("warmup_steps", 0) or 0), float(get("warmup_frac", 0.0) or 0.0)
    if w_steps and w_frac:
        raise ValueError("give --warmup-steps or --warmup-frac, not both")
    if kind or w_steps or w_frac:
        warm = w_steps or int(round(w_frac * total_steps))
        out["schedule"] = LRSchedule(kind or "constant", warm, total_steps, float(get("min_lr_ratio", 0.0) or 0.0))
    if get("adamw", 0):
        out["decoupled_weight_decay"] = True
    no_decay = get("no_decay")
    undecayed = _matching(names, _patterns(no_decay), "--no-decay") if no_decay is not None else \
        (_matching(names, _patterns(DEFAULT_NO_DECAY), "--no-decay", required=False) if get("adamw", 0) else set())
    frozen = _matching(names, _patterns(get("freeze")), "--freeze")
    scales = []
    for item in _patterns(get("lr_scale")):
        pat, sep, val = item.rpartition("=")
        if not sep or not pat:
            raise ValueError(f"--lr-scale: {item!r} is not PATTERN=F")
        _matching(names, [pat], "--lr-scale")
        scales.append((pat, float(val)))
    groups = []
    for n in names:
        opts = {}
        if n in frozen:
            opts["lr_scale"] = 0.0
        else:
            opts.update(next(({"lr_scale": f} for pat, f in scales if fnmatch.fnmatchcase(n, pat)), {}))
        if n in undecayed:
            opts["weight_decay"] = 0.0
        if opts:
            groups.append((n, opts))
    if groups:
        out["param_groups"] = groups
    ema = float(get("ema_decay", 0.0) or 0.0)
    if ema:
        out["ema_decay"] = ema
    if get("ema_eval", 0) and not ema:
        raise ValueError("--ema-eval 1 needs --ema-decay")
    return out
