"""Shared building blocks of the HIP model classes.

Parameters are held in `ParamTree`s that mirror the module tree (and therefore the
`state_dict()` keys, shapes, order and init distributions) of the stock torch modules the
reference builds (nn.LSTM, nn.TransformerEncoder, nn.Sequential(nn.Linear, ...)); the forward
pass never calls those modules - it runs the HIP kernels through `rlt_hip.ops`.
"""
import torch
from torch import nn

from rlt_hip import native as N
from rlt_hip import ops


class ParamTree(nn.Module):
    """Parameter-only mirror of `src`: same names, shapes, order and (cloned) initial values."""

    def __init__(self, src: nn.Module):
        super().__init__()
        for name, p in src.named_parameters(recurse=False):
            self.register_parameter(name, nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad))
        for name, child in src.named_children():
            sub = ParamTree(child)
            if next(sub.parameters(), None) is not None:
                self.add_module(name, sub)

    def forward(self, *a, **k):          # pragma: no cover - holders are never called
        raise RuntimeError("ParamTree only holds parameters")


def bilstm_params(input_size, hidden=128):
    # same construction as models/AttnCut.py:8
    return ParamTree(nn.LSTM(input_size=input_size, hidden_size=hidden, num_layers=2,
                             batch_first=True, bidirectional=True))


def encoder_params(d_model, n_head, num_layers, dropout):
    # same construction as models/AttnCut.py:9-10 (post-norm, ReLU, FF 2048, eps 1e-5)
    layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=n_head, dropout=dropout)
    return ParamTree(nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False))


def head_params(d_model):
    # nn.Sequential(nn.Linear(d_model, 1), <activation>): parameters live under key "0"
    return ParamTree(nn.Sequential(nn.Linear(d_model, 1)))


def check_input(x, ndim=3):
    if not x.is_cuda:
        raise RuntimeError("the HIP models run on the GPU only: move the model and its inputs to 'cuda' "
                           "(no CPU fallback exists)")
    if x.dim() != ndim:
        raise ValueError(f"expected a {ndim}-d input, got {tuple(x.shape)}")
    return N.f32c(x)


def check_dropout(module, p):
    """Effective dropout probability: p in train(), 0 in eval() (nn.Dropout semantics)."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout must be in [0, 1), got {p}")
    return float(p) if module.training else 0.0


def bilstm(x_pm, params, S, B):
    """2 stacked bidirectional layers, position-major in and out (one call into the library per direction of travel)."""
    return ops.bilstm(x_pm, params, S, B)


def check_attention_axis(axis):
    """'list' (the lists of a mini-batch attend to each other at every position: what the reference computes) or 'position'
    (every list attends over its own positions: the model of the papers); anything else is a ValueError.  Parameters,
    state_dict keys, shapes and initialisation do not depend on it."""
    return ops.check_attention_axis(axis)


def check_attention_mask(mask, axis):
    """'none' (every position attends to every position of its list) or 'causal' (position i attends to the positions <= i: the
    encoder's output at rank i is computed without looking below rank i); 'causal' needs axis 'position', anything else is a
    ValueError.  Like the axis, the mask changes no parameter: state_dicts load across masks.  -> the mask string."""
    ops.check_attention_mask(mask, axis)
    return mask


CUT_HEADS = ("softmax", "hazard")
HAZARD_PRIORS = ("uniform", "none")


def check_cut_head(cut_head, hazard_prior="uniform"):
    """'softmax' (Linear -> softmax over the S positions: the reference's head, the default) or 'hazard' (the logit is a stop
    logit, p_s = h_s prod_{j<s} (1 - h_j): ops.hazard_head, whose value at rank s reads ranks <= s only); hazard_prior 'uniform'
    (the fixed offset under which zero weights give the uniform cut distribution) or 'none'.  Anything else is a ValueError.
    Neither changes a parameter: state_dicts load across heads.  -> (cut_head, hazard_prior)"""
    if cut_head not in CUT_HEADS:
        raise ValueError(f"cut_head must be one of {CUT_HEADS}, got {cut_head!r}")
    if hazard_prior not in HAZARD_PRIORS:
        raise ValueError(f"hazard_prior must be one of {HAZARD_PRIORS}, got {hazard_prior!r}")
    return cut_head, hazard_prior


def cut_head(module, h, S, B):
    """The cut distribution (B,S,1) of `module` (a CutModel with a `decison_layer`) from the encoder output h (S*B,E)."""
    lin = getattr(module.decison_layer, "0")
    if module.cut_head == "softmax":
        return ops.heads(h, [lin.weight], [lin.bias], [N.HEAD_SOFTMAX], S, B)[0]
    p, stop = ops.hazard_head(h, lin.weight, lin.bias, S, B, module.hazard_offset(S, h.device))
    if module._stop_sink is not None:
        module._stop_sink.append(stop)
    return p.unsqueeze(2)


def encoder(x_pm, params, n_head, S, B, drop_p=0.0, axis="list", causal=False):
    """Stack of post-norm encoder layers with list-axis (axis='list') or within-list (axis='position') attention.  drop_p > 0
    applies the four dropouts of nn.TransformerEncoderLayer: attention probabilities, dropout1 (attention branch),
    the FFN hidden dropout and dropout2 (FFN branch).  causal=True (axis='position' only, else ValueError): every layer attends
    to the positions <= i, and since the rest of a layer is per row, row i of the stack's output depends on rows <= i of x_pm."""
    ops.check_attention_mask("causal" if causal else "none", axis)
    h = x_pm
    for layer in params.layers.children():
        h = ops.encoder_layer(h, layer, S, B, n_head, drop_p, axis=axis, causal=causal)
    return h


def pick_tasks(num_tasks):
    """Head list for the float task code of models/MtAttnCut.py:27-29."""
    if num_tasks == 3:
        return ["classi", "rerank", "decison_layer"]
    if num_tasks == 2.1:
        return ["classi", "decison_layer"]
    return ["rerank", "decison_layer"]


class _CallableHead:
    """The `rerank` parameter holder of a model (every attribute is the holder's), callable as the model's `rerank_order`."""
    __slots__ = ("_head", "_call")

    def __init__(self, head, call):
        object.__setattr__(self, "_head", head)
        object.__setattr__(self, "_call", call)

    def __getattr__(self, name):
        return getattr(self._head, name)

    def __setattr__(self, name, value):
        setattr(self._head, name, value)

    def __call__(self, x, by="rerank"):
        return self._call(x, by=by)


class CutModel(nn.Module):
    """Common base of the truncation models: `truncate` says where the model cuts each list, with no labels."""

    cut_head, hazard_prior = "softmax", "uniform"      # the models that take `cut_head=` set their own
    _stop_sink = None                                   # a list while stop_probabilities runs the forward

    def hazard_offset(self, S, device):
        """The hazard head's fixed prior offset for lists of S positions on `device` (ops.hazard_prior_offset), None under
        hazard_prior='none'.  Not a parameter and not in the state_dict: built once per (S, device) and kept."""
        if self.hazard_prior == "none":
            return None
        cache = self.__dict__.setdefault("_hazard_offsets", {})
        key = (int(S), str(device))
        if key not in cache:
            cache[key] = ops.hazard_prior_offset(S, device)
        return cache[key]

    def _eval_outputs(self, x):
        """forward(x) in eval mode under no_grad -> (the cut head's output, the stop probabilities (B,S) or None); the module's
        train / eval state is restored."""
        was_training = self.training
        self.eval()
        self._stop_sink = sink = []
        try:
            with torch.no_grad():
                out = self(x)
        finally:
            self._stop_sink = None
            self.train(was_training)
        return (out[-1] if isinstance(out, (list, tuple)) else out), (sink[-1] if sink else None)

    def stop_probabilities(self, x):
        """x: what forward takes.  Runs a cut_head='hazard' model in eval mode under no_grad and returns its stop probabilities
        (B,S): stop[b,s] = P(cut at s+1 | no cut before), 1 at the last position - what truncate(rule='above') sweeps.  Row s
        is computed from what the encoder gives for ranks <= s.  A softmax-head model has none: ValueError."""
        if self.cut_head != "hazard":
            raise ValueError(f"{type(self).__name__} with cut_head={self.cut_head!r} has no stop probabilities: build it with cut_head='hazard'")
        return self._eval_outputs(x)[1]

    def truncate(self, x, *, rule=None, tau=None):
        """x: what forward takes (BiCut with sparse_input: an ops.SparseBatch).  Runs the model in eval mode under no_grad and
        returns (k (B,) int32, p_k (B,) float32) on the device: each list's cut and the winning value (rlt_cut_report, label-free:
        first maximum + 1, or BiCut's rule on its (B,S,2) output).  The module's train / eval state is restored.
        With `rule` and `tau` set ('quantile' | 'above' | 'score' and one threshold: ops.cut_sweep) the model's output is cut by
        that rule instead - BiCut's class-0 column at stride 2 - and only k (B,) int32 is returned (rlt_cut_sweep, label-free,
        T = 1; k may be 0 under 'score').  A cut_head='hazard' model is swept on its stop probabilities under 'above' (the
        first rank whose stop probability reaches tau: a decision made at that rank); every other rule reads p."""
        if (rule is None) != (tau is None):
            raise ValueError("truncate: pass both `rule` and `tau`, or neither")
        cut, stop = self._eval_outputs(x)
        with torch.no_grad():
            if rule is not None:
                if rule == "above" and stop is not None:
                    cut = stop
                thr = torch.full((1,), float(tau), dtype=torch.float64, device=cut.device)
                k, _ = ops.cut_sweep(cut, thr, rule)
                return k.reshape(-1)
            per, _ = ops.cut_report(cut)
        return per["k"], per["p_k"]

    # why a class cannot be streamed a page of ranks at a time (Choopy overrides `stream`)
    _NO_STREAM = {"AttnCut": "its BiLSTM runs over the list in both directions, so every rank reads the ranks below it",
                  "MtAttnCut": "its BiLSTM runs both ways and its multi-task heads normalise over the whole list",
                  "MtChoopy": "its multi-task heads (softmax re-ranking, classification) normalise over the whole list",
                  "BiCut": "its BiLSTM runs over the list in both directions"}

    def stream(self, tau, batch_size, compact_every=None, compact_below=1.0):
        """Only a Choopy with attention_axis='position', attention_mask='causal', cut_head='hazard' can truncate online
        (utils/stream.py); every other model raises ValueError saying why."""
        why = self._NO_STREAM.get(type(self).__name__, "its output at a rank is not computed from the ranks above it alone")
        raise ValueError(f"{type(self).__name__} cannot stream: {why} (use Choopy with attention_axis='position', "
                         "attention_mask='causal', cut_head='hazard')")

    _TOWER_HEADS = {"TowerClass": "classi", "TowerRerank": "rerank", "TowerCut": "decison_layer"}

    def head_names(self):
        """The names of the model's outputs in the order forward returns them ('classi', 'rerank', 'decison_layer'): the towers
        of the expert models, the task code of MtAttnCut / MtChoopy; () for a model with the cut head alone."""
        if hasattr(self, "towers"):
            return tuple(self._TOWER_HEADS.get(type(t).__name__, "") for t in self.towers)
        if hasattr(self, "num_tasks"):
            return tuple(pick_tasks(self.num_tasks))
        return ()

    def __getattr__(self, name):
        # `model.rerank(x, by=...)` beside the `rerank` parameter holder of MtAttnCut / MtChoopy, whose state_dict keys are the
        # reference's: the holder, where there is one, comes back callable
        if name == "rerank":
            head = self.__dict__.get("_modules", {}).get("rerank")
            return self.rerank_order if head is None else _CallableHead(head, self.rerank_order)
        return super().__getattr__(name)

    def rerank_order(self, x, by="rerank"):
        """`model.rerank(x, by=...)`.  x: what forward takes.  Runs the model in eval mode under no_grad and returns
        (perm (B,S) int32, k (B,) int32) on the device: the order of each list by the auxiliary head `by` ('rerank' | 'classi'), descending and stable
        (ops.rerank_lists: perm[b,i] = the original index of the document at new position i), and the model's own cut as
        `truncate` gives it.  The module's train / eval state is restored.  A model, or a num_tasks, without that head is a
        ValueError: the cut head never stands in for it."""
        if by not in ("rerank", "classi"):
            raise ValueError(f"rerank: by must be 'rerank' or 'classi', got {by!r}")
        names = self.head_names()
        if by not in names:
            raise ValueError(f"{type(self).__name__}{' with num_tasks=%s' % self.num_tasks if hasattr(self, 'num_tasks') else ''} "
                             f"has no {by!r} head (its outputs: {list(names) or ['the cut distribution']})")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                out = self(x)
                if isinstance(out, tuple) and isinstance(out[-1], (list, tuple)):       # ProbeBase: (h, experts, towers)
                    out = out[-1]
                if len(out) != len(names):
                    raise ValueError(f"{type(self).__name__} returned {len(out)} outputs for the heads {list(names)}")
                perm = ops.rerank_lists(out[names.index(by)])[0]
                per, _ = ops.cut_report(out[-1])
        finally:
            self.train(was_training)
        return perm, per["k"]
