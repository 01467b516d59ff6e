"""The cut sweep (rlt_cut_sweep, ops.cut_sweep, utils/sweep.py, run.py --cut-sweep) without a GPU: the C ABI is declared, bound and
exported, the workspace query needs no device and never shrinks in B, argument errors are answered before any launch, and
the command line accepts and rejects --cut-sweep strings."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbols_declared_bound_exported(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    for name in ("rlt_cut_sweep", "rlt_cut_sweep_workspace"):
        assert name in native.EXPORTS
        assert hasattr(native.load(), name)
    for name, value in (("RLT_SWEEP_QUANTILE", 0), ("RLT_SWEEP_FIRST_BELOW", 1), ("RLT_SWEEP_FIRST_ABOVE", 2), ("RLT_SWEEP_COLS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert (native.SWEEP_QUANTILE, native.SWEEP_FIRST_BELOW, native.SWEEP_FIRST_ABOVE, native.SWEEP_COLS) == (0, 1, 2, 8)
    assert len(native.SWEEP_ROWS) == native.SWEEP_COLS
    assert native.load().rlt_abi_version() == 5


def test_workspace_query(native):
    q = lambda B, S, T: native.query("rlt_cut_sweep_workspace", B, S, T)
    assert q(0, 300, 19) == 0 and q(-1, 300, 19) == 0
    assert q(8, 0, 19) == 0 and q(8, 1025, 19) == 0 and q(8, -3, 19) == 0
    assert q(8, 300, 0) == 0 and q(8, 300, 65) == 0 and q(8, 300, -1) == 0
    for S in (1, 64, 65, 300, 1024):
        for T in (1, 19, 64):
            sizes = [q(B, S, T) for B in (1, 2, 5, 67, 1030, 4096, 1 << 20, (1 << 31) - 1)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (S, T, sizes)
            assert sizes[0] >= 8 * T * 8 and all(s % 16 == 0 for s in sizes)
    # one record of 8 T float64 per workgroup of four lists, the grid capped at 2048
    assert q(5, 300, 19) == 2 * 8 * 19 * 8
    assert q(1 << 20, 300, 19) == 2048 * 8 * 19 * 8


def test_argument_errors_before_any_launch(native):
    lib = native.load()
    buf = (ctypes.c_uint8 * (1 << 20))()
    base = ctypes.addressof(buf)
    x = ctypes.c_void_p(base)
    off = lambda n: ctypes.c_void_p(base + n)
    B, S, T = 4, 40, 19
    ws_b = native.query("rlt_cut_sweep_workspace", B, S, T)

    def call(v=x, stride=1, rule=0, thr=x, T=T, labels=x, B=B, S=S, tab=x, k=x, curve=x, ws=x, ws_b=ws_b):
        return lib.rlt_cut_sweep(v, stride, rule, thr, T, labels, B, S, -1.0, 1.0, tab, 0, k, curve, ws, ws_b, None)
    assert call(rule=3) == -1 and call(rule=-1) == -1
    assert call(stride=0) == -1 and call(stride=3) == -1
    assert call(T=0) == -1 and call(T=65, ws_b=1 << 20) == -2
    assert call(S=0) == -1 and call(S=1025, ws_b=1 << 20) == -2
    assert call(B=0) == -1 and call(B=-1) == -1
    assert call(v=None) == -1 and call(thr=None) == -1
    assert call(k=None, curve=None) == -1                   # nothing asked for
    assert call(labels=None) == -1                          # a curve without labels
    assert call(labels=None, curve=None, k=None) == -1      # label-free mode needs k
    assert call(tab=None) == -1 and call(ws=None) == -1     # the curve needs the DCG table and the workspace
    assert call(ws_b=ws_b - 1) == -3 and call(ws_b=0) == -3
    assert call(ws=off(4)) == -4
    assert call(curve=off(4)) == -4
    assert call(thr=off(4)) == -4
    assert call(tab=off(4)) == -4
    assert call(v=off(2)) == -4 and call(labels=off(2)) == -4 and call(k=off(2)) == -4


def test_python_surface_imports_without_gpu():
    import inspect
    from rlt_hip import ops
    from utils import baselines, sweep
    from models import _common
    assert callable(ops.cut_sweep) and callable(baselines.score_threshold) and callable(sweep.tune_cut_rule)
    assert all(hasattr(sweep.CutSweep, m) for m in ("update", "n_lists", "curve", "best", "at"))
    sig = inspect.signature(_common.CutModel.truncate)
    for name in ("rule", "tau"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is None
    assert [ops.sweep_rule(r) for r in ("quantile", "score", "above")] == [0, 1, 2]
    with pytest.raises(ValueError):
        ops.sweep_rule("argmax")


def test_run_parser_accepts_and_rejects_cut_sweep_strings():
    import run
    parse = run.build_parser().parse_args
    args = parse([])
    assert args.cut_sweep is None and args.sweep_out is None
    args = parse(["--cut-sweep", "quantile:0.05:0.95:19", "--sweep-out", "s.npz"])
    rule, th = args.cut_sweep
    assert rule == "quantile" and args.sweep_out == "s.npz"
    assert th.dtype == np.float64 and th.shape == (19,) and th[0] == 0.05 and th[-1] == 0.95
    assert np.array_equal(th, np.linspace(0.05, 0.95, 19))
    assert parse(["--cut-sweep", "above:0.5:0.5:1"]).cut_sweep[1].tolist() == [0.5]
    assert parse(["--cut-sweep", "score:-2:7.5:64"]).cut_sweep[1].shape == (64,)
    assert parse(["--cut-sweep", "score:auto:7"]).cut_sweep == ("score", 7)
    for bad in ("argmax:0:1:5", "quantile", "quantile:0:1", "quantile:0:1:0", "quantile:0:1:65", "quantile:1:0:5", "quantile:a:1:5",
                "quantile:0:1:2.5", "quantile:auto:5", "score:auto:0", "score:auto:65", "score:auto:x", "above:0:nan:3",
                "quantile:0:1:5:6", ""):
        with pytest.raises(SystemExit):
            parse(["--cut-sweep", bad])


def test_score_quantiles_are_host_quantiles():
    from utils.sweep import score_quantiles
    s = np.arange(101, dtype=np.float32).reshape(1, 101)
    assert np.allclose(score_quantiles(s, 3), [25.0, 50.0, 75.0])
