"""The cut report (rlt_cut_report, ops.cut_report, utils/report.py, models' truncate) without a GPU: the C ABI is declared, bound
and exported, argument errors are answered before any launch, the workspace query is monotone in B, and the float64 numpy
restatement (tests/report_restate.py) reproduces what the reference's own `Trainer.plot` and BiCut loop returned for the
committed fixtures (tests/golden/report_*.npz, tools/make_report_golden.py).

Restatement against the reference's fp32 curves: the reference rounds x = v / scale to fp32 (an absolute error of 2^-24 |x| in
the exponent, for the term and again for the normaliser), takes exp, sums S terms, divides and averages in fp32, and builds
the DCG reward as an fp32 sum of gains (error up to 2^-24 G, G = sum_j 1 / log2(j + 2), entering term and normaliser after
the division by tau).  Relative to a curve value that is at most 2^-23 (xmax + 8 + 2 G / tau), xmax the largest |x|; G = 0
for the F1 reward and the prediction curve."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import report_restate as R  # noqa: E402

FIXTURES = sorted(f for f in glob.glob(os.path.join(REPO, "tests", "golden", "report_*.npz")) if "bicut" not in f)
BICUT = os.path.join(REPO, "tests", "golden", "report_bicut_s40.npz")


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbols_declared_bound_exported(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    for name in ("rlt_cut_report", "rlt_cut_report_workspace"):
        assert name in native.EXPORTS
        assert hasattr(native.load(), name)
    assert "RLT_CUT_ARGMAX" in header and "RLT_CUT_PAIR" in header
    assert (native.CUT_ARGMAX, native.CUT_PAIR) == (0, 1)
    assert native.load().rlt_abi_version() == 5


def test_workspace_query_is_monotone_in_b(native):
    q = lambda B, S: native.query("rlt_cut_report_workspace", B, S)
    assert q(0, 300) == 0 and q(-1, 300) == 0 and q(8, 0) == 0 and q(8, 1025) == 0
    for S in (1, 40, 64, 65, 300, 1024):
        sizes = [q(B, S) for B in (1, 2, 5, 67, 1030, 4096, 1 << 20)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (S, sizes)
        assert sizes[0] >= (3 * S + 2) * 8 + 16
        assert all(s % 16 == 0 for s in sizes)
    # one record per workgroup (the grid capped at 1024), then F1@k and DCG@k per list
    assert q(1 << 20, 300) == 1024 * (3 * 300 + 2) * 8 + 16 * (1 << 20)


def test_argument_errors_before_any_launch(native):
    lib = native.load()
    buf = (ctypes.c_uint8 * (1 << 20))()
    base = ctypes.addressof(buf)
    x = ctypes.c_void_p(base)
    B, S = 4, 40
    ws_b = native.query("rlt_cut_report_workspace", B, S)

    def call(p=x, rule=0, labels=x, coef=x, B=B, S=S, metric=0, tau=0.9, sharpen=9e-4, tab=x, f1=x, hist=x, ws=x, ws_b=ws_b):
        return lib.rlt_cut_report(p, rule, labels, coef, B, S, metric, -1.0, -1.0, tau, sharpen, tab, 0, x, x, x, f1, None, None,
                                  None, None, None, None, hist, x, x if labels is not None else None, x, ws, ws_b, None)
    assert call(p=None) == -1 and call(ws=None) == -1
    assert call(S=0) == -1 and call(B=0) == -1 and call(B=-1) == -1
    assert call(rule=2) == -1 and call(metric=2) == -1
    assert call(tau=0.0) == -1 and call(sharpen=0.0) == -1 and call(sharpen=-1.0) == -1
    assert call(tab=None) == -1
    assert call(metric=1, coef=None) == -1                  # the DCG reward reads the fp32 coefficients
    assert call(labels=None, f1=x) == -1                    # a labelled output without labels
    assert call(S=1025, ws_b=1 << 20) == -2
    assert call(ws=ctypes.c_void_p(base + 4)) == -4
    assert call(hist=ctypes.c_void_p(base + 4)) == -4
    assert call(tab=ctypes.c_void_p(base + 4)) == -4
    assert call(rule=1, p=ctypes.c_void_p(base + 4)) == -4  # PAIR reads float2
    assert call(p=ctypes.c_void_p(base + 2)) == -4
    assert call(ws_b=ws_b - 1) == -3


def test_python_surface_imports_without_gpu():
    from rlt_hip import ops
    from utils import report
    import models
    from models import _common
    assert callable(ops.cut_report)
    assert all(hasattr(report.CutReport, m) for m in ("update", "per_query", "curves", "summary"))
    for name in ("AttnCut", "BiCut", "Choopy", "MtAttnCut", "MtChoopy", "MMOECut", "MOECut", "PLECut"):
        cls = getattr(models, name)
        assert issubclass(cls, _common.CutModel) and callable(cls.truncate)


def test_run_parser_offers_the_report_flags():
    import run
    args = run.build_parser().parse_args([])
    assert args.report_out is None and args.report_split == "test" and args.report_labels == 1 and args.draw == 0
    args = run.build_parser().parse_args(["--report-out", "r.npz", "--report-split", "train", "--report-labels", "0", "--draw", "1"])
    assert (args.report_out, args.report_split, args.report_labels, args.draw) == ("r.npz", "train", 0, 1)
    with pytest.raises(SystemExit):
        run.build_parser().parse_args(["--report-split", "dev"])


def test_there_are_five_fixtures():
    names = sorted(os.path.basename(f) for f in FIXTURES)
    assert names == ["report_edge_s40.npz", "report_losses_edge_s300.npz", "report_mq2007_s40.npz", "report_robust04_s300.npz"]
    for f in FIXTURES + [BICUT]:
        assert os.path.getsize(f) < 1 << 20
    for f in FIXTURES:
        assert float(np.load(f)["output"].max()) < 0.07      # the reference's fp32 exp(p / 9e-4) stays finite


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_restatement_reproduces_the_reference_curves(path):
    d = np.load(path)
    y, p, tau = d["labels"].astype(np.float64), d["output"], float(d["tau"])
    B, S = y.shape
    eps = 2.0 ** -23
    pred = R.tail_fix(R.pred_curve(p, tau * 1e-3) / B)
    xmax = float(p.max()) / (tau * 1e-3)
    assert np.all(np.abs(pred - d["pred"]) <= eps * (xmax + 8) * pred), np.abs(pred / d["pred"] - 1).max()
    G = float((1.0 / np.log2(np.arange(S) + 2.0)).sum())
    for metric, g in (("f1", 0.0), ("dcg", G)):
        r = R.reward(y, metric)
        curve = R.reward_curve(r, tau) / B
        xmax = float(np.abs(r).max()) / tau
        ref = d[f"reward_{metric}"]
        assert np.all(np.abs(curve - ref) <= eps * (xmax + 8 + 2 * g / tau) * curve), (metric, np.abs(curve / ref - 1).max())
        assert abs(curve.sum() - 1.0) < 1e-12


def test_restatement_reproduces_the_reference_bicut_cuts():
    d = np.load(BICUT)
    k = R.cut_pair(d["output2"])
    assert np.array_equal(k, d["k"])
    S = d["output2"].shape[1]
    assert k[1] == S and k[2] == 12                         # never truncates; a tie goes to class 0


def test_restatement_cut_rules_on_small_cases():
    p = np.array([[0.1, 0.4, 0.4, 0.1], [0.7, 0.1, 0.1, 0.1]], dtype=np.float32)
    assert R.cut_argmax(p).tolist() == [2, 1]
    assert R.margin_argmax(p).tolist() == [0.0, np.float32(0.7) - np.float32(0.1)]
    y = np.array([[1, 0, 1, 0]], dtype=np.float64)
    assert np.allclose(R.reward(y, "f1")[0], [2 / 3, 2 / 4, 4 / 5, 4 / 6])
    assert np.allclose(R.reward(y, "dcg")[0], np.cumsum([1, -1 / np.log2(3), 1 / 2, -1 / np.log2(5)]))
