"""The recipe step's C ABI without a GPU (include/rlt_hip.h: rlt_adam_step_recipe, rlt_lr_at, rlt_swap_f32): symbols exported and
bound, every documented argument error answered with its code before any launch - host buffers stand in for device memory,
nothing is launched -, the host schedule against the restatement, the pattern -> group-table mapping of FusedAdam and the
flags -> keyword-arguments helper of the trainers."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import recipe_restate as RR

ARG, SHAPE, WORKSPACE, ALIGN = -1, -2, -3, -4
NEW = ("rlt_recipe_chunk", "rlt_recipe_grid", "rlt_lr_at", "rlt_adam_step_recipe", "rlt_swap_f32")


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def _buf(nbytes):
    raw = (ctypes.c_uint8 * (nbytes + 64))()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    return raw, base


def test_symbols_exported_bound_and_the_constants(native):
    lib = native.load()
    for name in NEW:
        assert name in native.EXPORTS and hasattr(lib, name)
    C, G = native.query("rlt_recipe_chunk"), lib.rlt_recipe_grid()
    assert C >= 1024 and C % 1024 == 0 and G >= 1        # a chunk is whole 16-byte groups of a 256-lane workgroup
    assert lib.rlt_abi_version() == 5
    assert ctypes.sizeof(native.RecipeStruct) == 64 and native.RECIPE_STATE_WORDS * 8 == 32
    assert native.OPT_STATE_WORDS * 8 == 104              # rlt_opt_state keeps its size


def test_recipe_step_argument_errors(native):
    lib = native.load()
    n = 64
    keep, base = _buf(5 * 4 * n + 256)
    p, g, m, v, ema = (base + i * 4 * n for i in range(5))
    state, rstate, groups = base + 20 * n, base + 20 * n + 104, base + 20 * n + 144
    offs = (ctypes.c_int64 * 4)(0, 8, 40, n)
    P = ctypes.c_void_p
    ok = dict(base_lr=1e-3, weight_decay=0.01, sched_kind="cosine", warmup_steps=3, total_steps=8, min_lr_ratio=0.1, ema_decay=0.9)

    def call(p_=p, g_=g, m_=m, v_=v, e_=ema, n_=n, off=offs, gr=groups, ns=3, st=state, rs=rstate, rec=True, **fields):
        r = native.recipe_struct(**{**ok, **fields})
        return lib.rlt_adam_step_recipe(*(P(x) if x else None for x in (p_, g_, m_, v_, e_)), n_, off, P(gr) if gr else None, ns,
                                        P(st) if st else None, P(rs) if rs else None, ctypes.byref(r) if rec else None, None)
    nan = float("nan")
    # null pointers, n == 0, inconsistent table arguments
    assert call(p_=0) == ARG and call(g_=0) == ARG and call(m_=0) == ARG and call(v_=0) == ARG
    assert call(st=0) == ARG and call(rs=0) == ARG and call(rec=False) == ARG and call(n_=0) == ARG
    assert call(ns=-1) == ARG and call(off=None) == ARG and call(gr=0) == ARG and call(ns=0) == ARG and call(ns=0, off=None) == ARG
    # the schedule: a decay kind with T <= W, the ratio outside [0, 1], an unknown kind, a negative warm-up
    assert call(sched_kind="cosine", total_steps=3) == ARG and call(sched_kind="linear", warmup_steps=9) == ARG
    assert call(min_lr_ratio=-0.1) == ARG and call(min_lr_ratio=1.5) == ARG and call(sched_kind=3) == ARG and call(warmup_steps=-1) == ARG
    # the average: decay outside [0, 1), ema with decay 0, decay without ema
    assert call(ema_decay=1.0) == ARG and call(ema_decay=-0.5) == ARG and call(ema_decay=0.0) == ARG and call(e_=0) == ARG
    # any NaN
    for field in ("base_lr", "beta1", "beta2", "eps", "weight_decay", "min_lr_ratio", "ema_decay"):
        assert call(**{field: nan}) == ARG, field
    # shape and alignment, as rlt_adam_step_guarded
    assert call(n_=n - 2, off=None, gr=0, ns=0) == SHAPE
    for k in ("p_", "g_", "m_", "v_", "e_"):
        assert call(**{k: {"p_": p, "g_": g, "m_": m, "v_": v, "e_": ema}[k] + 4}) == ALIGN, k
    assert call(st=state + 4) == ALIGN and call(rs=rstate + 4) == ALIGN and call(gr=groups + 4) == ALIGN
    # a segment table the host can read is checked as rlt_grad_norm checks it
    for bad in ((0, 40, 8, n), (4, 8, 40, n), (0, 8, 40, n - 4), (0, 6, 40, n), (0, 8, 40, n + 4)):
        assert call(off=(ctypes.c_int64 * 4)(*bad)) == ARG, bad
    # a constant schedule never reads total_steps
    assert native.lr_at(native.recipe_struct(base_lr=0.5, warmup_steps=4), 2) == 0.25


def test_swap_argument_errors(native):
    lib = native.load()
    keep, base = _buf(1024)
    P = ctypes.c_void_p
    call = lambda a=base, b=base + 256, n=64: lib.rlt_swap_f32(P(a) if a else None, P(b) if b else None, n, None)
    assert call(a=0) == ARG and call(b=0) == ARG and call(n=0) == ARG and call(n=62) == SHAPE
    assert call(a=base + 4) == ALIGN and call(b=base + 264) == ALIGN
    assert call(b=base) == ARG and call(b=base + 128) == ARG          # overlapping


@pytest.mark.parametrize("W", [3, 0])
def test_lr_at_is_the_restatement(native, W):
    T, base, ratio = 8, 3e-5, 0.1
    for kind in ("constant", "linear", "cosine"):
        r = native.recipe_struct(base_lr=base, sched_kind=kind, warmup_steps=W, total_steps=T, min_lr_ratio=ratio)
        for t in range(1, 11):
            got, want = native.lr_at(r, t), RR.lr_at(t, base, kind, W, T, ratio)
            if kind == "cosine":            # the host's cos against numpy's may differ in the last double bit
                g32, w32 = np.float32(got), np.float32(want)
                assert abs(float(g32) - float(w32)) <= float(np.spacing(w32)), (kind, t, got, want)
            else:
                assert got == want, (kind, t, got, want)
    assert np.isnan(native.lr_at(native.recipe_struct(base_lr=base, sched_kind="linear", warmup_steps=5, total_steps=5), 1))
    assert np.isnan(native.lr_at(native.recipe_struct(base_lr=base), 0))


def test_lr_schedule_class(native):
    from rlt_hip.parallel import LRSchedule
    s = LRSchedule("linear", 3, 8, 0.1)
    assert [s.lr_at(t, 3e-5) for t in range(1, 11)] == [RR.lr_at(t, 3e-5, "linear", 3, 8, 0.1) for t in range(1, 11)]
    assert s.lr_at(3) == 1.0 and s.lr_at(1) == 1.0 / 3.0
    for bad in (("step", 0, 8, 0.0), ("cosine", 8, 8, 0.0), ("linear", -1, 8, 0.0), ("linear", 0, 8, 1.5)):
        with pytest.raises(ValueError):
            LRSchedule(*bad)


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1 = torch.nn.LayerNorm(4)
        self.linear1 = torch.nn.Linear(4, 6)


def _module():
    m = torch.nn.Module()
    m.embed = torch.nn.Linear(3, 4)
    m.layers = torch.nn.ModuleList([_Block(), _Block()])
    return m


def test_patterns_to_group_table(native):
    from rlt_hip.parallel import FlatModel, FusedAdam, resolve_param_groups
    flat = FlatModel(_module())
    assert flat.names == ["embed.weight", "embed.bias", "layers.0.norm1.weight", "layers.0.norm1.bias", "layers.0.linear1.weight",
                          "layers.0.linear1.bias", "layers.1.norm1.weight", "layers.1.norm1.bias", "layers.1.linear1.weight",
                          "layers.1.linear1.bias"]
    groups = [("*.norm1.weight", {"weight_decay": 0.0}), ("*.bias", {"weight_decay": 0.0, "lr_scale": 2.0}),
              ("layers.0.*", {"lr_scale": 0.0}), ("*.weight", {"lr_scale": 0.5})]
    opt = FusedAdam(flat, lr=1e-3, weight_decay=0.25, param_groups=groups)        # construction needs no GPU, step() does
    want = [(0.5, 0.25), (2.0, 0.0), (1.0, 0.0), (2.0, 0.0), (0.0, 0.25), (2.0, 0.0), (1.0, 0.0), (2.0, 0.0), (0.5, 0.25), (2.0, 0.0)]
    assert opt.group_values == want                       # the first match wins: layers.0.norm1.weight is not frozen, its bias is not
    assert opt.group_table.dtype == torch.float32 and opt.group_table.tolist() == [list(w) for w in want]
    assert opt.recipe and not opt.guarded and opt.ema is None
    # unmatched names keep (1, weight_decay)
    assert resolve_param_groups(flat.names, [("embed.*", {"lr_scale": 0.0})], 0.25)[2:] == [(1.0, 0.25)] * 8
    with pytest.raises(ValueError, match="match no parameter"):
        FusedAdam(flat, param_groups=groups + [("*.norm3.*", {"weight_decay": 0.0})])
    with pytest.raises(ValueError):
        FusedAdam(flat, param_groups=[("*.bias", {"lr": 0.1})])
    with pytest.raises(ValueError):
        FusedAdam(flat, ema_decay=1.0)
    with pytest.raises(RuntimeError):
        FusedAdam(flat, ema_decay=0.5).step()             # a CPU bucket: no fallback
    plain = FusedAdam(flat, lr=1e-3)
    assert not plain.recipe and not plain.guarded
    with pytest.raises(RuntimeError):
        plain.current_lr()
    with pytest.raises(RuntimeError):
        with plain.ema_weights():
            pass
    # load_state_dict on the plain path: the host step count and both moments
    plain.load_state_dict({"steps": 7, "exp_avg": torch.ones(flat.numel), "exp_avg_sq": torch.full((flat.numel,), 2.0)})
    assert plain.steps == 7 and plain.exp_avg.eq(1).all() and plain.exp_avg_sq.eq(2).all()


def test_flags_to_kwargs_helper(native):
    import run
    from utils.recipe import DEFAULT_NO_DECAY, add_recipe_arguments, recipe_kwargs
    names = ["enc.weight_ih_l0", "enc.bias_ih_l0", "att.norm1.weight", "att.norm1.bias", "att.linear1.weight", "head.0.bias"]
    parse = lambda *argv: run.build_parser().parse_args(list(argv))
    assert recipe_kwargs(parse(), names, 100) == {}                              # the defaults: the plain or the guarded step
    assert recipe_kwargs(argparse.Namespace(), names, 100) == {}                 # a driver's own Namespace
    kw = recipe_kwargs(parse("--lr-schedule", "cosine", "--warmup-frac", "0.1", "--min-lr-ratio", "0.05"), names, 100)
    s = kw.pop("schedule")
    assert kw == {} and (s.kind, s.warmup_steps, s.total_steps, s.min_lr_ratio) == ("cosine", 10, 100, 0.05)
    s = recipe_kwargs(parse("--warmup-steps", "7"), names, 100)["schedule"]
    assert (s.kind, s.warmup_steps) == ("constant", 7)
    kw = recipe_kwargs(parse("--adamw", "1", "--ema-decay", "0.99"), names, 100)
    assert kw["decoupled_weight_decay"] is True and kw["ema_decay"] == 0.99
    assert kw["param_groups"] == [(n, {"weight_decay": 0.0}) for n in names if "bias" in n or "norm" in n]       # DEFAULT_NO_DECAY
    assert "position_encoding" in DEFAULT_NO_DECAY                               # matches nothing here and is dropped, not an error
    kw = recipe_kwargs(parse("--adamw", "1", "--no-decay", "*.bias", "--freeze", "enc.*", "--lr-scale", "att.norm1.*=0.5,att.*=0.25"), names, 100)
    assert kw["param_groups"] == [("enc.weight_ih_l0", {"lr_scale": 0.0}), ("enc.bias_ih_l0", {"lr_scale": 0.0}),
                                  ("att.norm1.weight", {"lr_scale": 0.5}), ("att.norm1.bias", {"lr_scale": 0.5, "weight_decay": 0.0}),
                                  ("att.linear1.weight", {"lr_scale": 0.25}), ("head.0.bias", {"weight_decay": 0.0})]
    for bad in (("--freeze", "nothing.*"), ("--no-decay", "*.gamma"), ("--lr-scale", "*.weight"), ("--lr-scale", "zzz=2"),
                ("--warmup-steps", "3", "--warmup-frac", "0.5"), ("--ema-eval", "1")):
        with pytest.raises(ValueError):
            recipe_kwargs(parse(*bad), names, 100)
    # the drivers share the flags, without --ema-eval
    import verify_BMT
    import verify_probe
    for mod in (verify_BMT, verify_probe):
        a = mod.build_parser().parse_args(["--adamw", "1", "--lr-schedule", "linear"])
        assert a.adamw == 1 and a.lr_schedule == "linear" and not hasattr(a, "ema_eval")
    p = argparse.ArgumentParser()
    add_recipe_arguments(p)
    assert p.parse_args(["--ema-eval", "1", "--ema-decay", "0.9"]).ema_eval == 1
