"""Truncation baselines (rlt_truncation_curves, utils/baselines.py, run.py --baselines) without a GPU: the C ABI is declared,
bound and exported, its argument errors are answered before any launch, run.py offers the flags, and the committed notebook
fixtures agree with an independent numpy restatement."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_restate as R  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "baselines_*.npz")))


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbols_declared_bound_exported(native):
    for name in ("rlt_truncation_curves", "rlt_truncation_curves_workspace"):
        assert name in native.EXPORTS
        assert hasattr(native.load(), name)
    assert native.load().rlt_abi_version() == 5


def test_workspace_query_needs_no_gpu(native):
    q = lambda B, S: native.query("rlt_truncation_curves_workspace", B, S)
    assert q(1, 300) >= (3 * 300 + 2) * 8
    assert q(1 << 20, 300) == 1024 * (3 * 300 + 2) * 8          # one record per workgroup, the grid capped at 1024
    assert q(4096, 40) == 256 * (3 * 40 + 2) * 8               # four lists per wavefront at S <= 64
    assert q(0, 300) == 0 and q(-1, 300) == 0 and q(8, 0) == 0 and q(8, 1025) == 0
    assert q(8, 1024) > 0


def test_argument_errors_before_any_launch(native):
    lib = native.load()
    buf = (ctypes.c_uint8 * (1 << 20))()
    base = ctypes.addressof(buf)
    x = ctypes.c_void_p(base)
    B, S = 4, 40
    ws_b = native.query("rlt_truncation_curves_workspace", B, S)
    call = lambda B=B, S=S, tab=x, ws=x, ws_b=ws_b, curves=x: lib.rlt_truncation_curves(
        x, B, S, -1.0, tab, 0, curves, None, None, None, None, None, ws, ws_b, None)
    assert call(S=0) == -1
    assert call(S=1025, ws_b=1 << 20) == -2
    assert call(B=-1) == -1
    assert call(B=0) == -1                                  # as rlt_cut_metrics / rlt_task_metrics: B must be positive
    assert call(tab=None) == -1
    assert call(curves=None) == -1
    assert call(ws=None) == -1
    assert call(tab=ctypes.c_void_p(base + 4)) == -4
    assert call(ws=ctypes.c_void_p(base + 4)) == -4
    assert call(ws_b=ws_b - 1) == -3


def test_run_help_lists_the_flags():
    res = subprocess.run([sys.executable, os.path.join(REPO, "ranked-list-truncation_amd", "run.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "--baselines" in res.stdout and "--fixed-k" in res.stdout


def test_run_parser_defaults():
    import run
    args = run.build_parser().parse_args([])
    assert args.baselines == 0 and args.fixed_k == "5,10,30"
    with pytest.raises(SystemExit):
        run.build_parser().parse_args(["--baselines", "2"])


def test_the_package_module_imports_without_gpu():
    from utils import baselines
    assert callable(baselines.best_cut) and callable(baselines.greedy_k) and callable(baselines.fixed_k)


def test_there_are_three_fixtures():
    names = sorted(os.path.basename(f) for f in FIXTURES)
    assert names == ["baselines_edge_s40.npz", "baselines_mq2007_s40.npz", "baselines_robust04_s300.npz"]
    for f in FIXTURES:
        assert os.path.getsize(f) < 1 << 20


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_fixtures_agree_with_the_numpy_restatement(path):
    d = np.load(path)
    for split in ("train", "test"):
        y = d[f"{split}_labels"]
        f1, dcg = R.per_k(y)
        # F1 in the notebook's operation order: bit for bit; DCG summed in another order: 1e-12
        assert np.array_equal(f1, d[f"{split}_per_k_f1"])
        assert np.abs(dcg - d[f"{split}_per_k_dcg"]).max() < 1e-12
        np.testing.assert_allclose(f1.mean(0), d[f"{split}_curve_f1"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(dcg.mean(0), d[f"{split}_curve_dcg"], rtol=0, atol=1e-12)
    y = d["test_labels"]
    f1, dcg = R.per_k(y)
    assert abs(f1.max(1).mean() - d["best_f1"]) < 1e-12 and abs(dcg.max(1).mean() - d["best_dcg"]) < 1e-12
    for i, k in enumerate(d["fixed_k"]):
        assert abs(f1[:, k].mean() - d["fixed_f1"][i]) < 1e-12 and abs(dcg[:, k].mean() - d["fixed_dcg"][i]) < 1e-12
    kf, kd = int(d["greedy_k_f1"]), int(d["greedy_k_dcg"])
    assert kf == int(np.argmax(d["train_curve_f1"])) and kd == int(np.argmax(d["train_curve_dcg"]))
    assert abs(f1[:, kf].mean() - d["greedy_f1"]) < 1e-12 and abs(dcg[:, kd].mean() - d["greedy_dcg"]) < 1e-12
    both = np.concatenate([d["train_labels"], d["test_labels"]])
    S = both.shape[1]
    n = min(S, len(d["countp"]))
    np.testing.assert_allclose(R.irrelevant_share(both)[:n], d["countp"][:n], rtol=0, atol=1e-12)
    # the restatement's chunked sums agree with its per-list arrays
    sums, best_sums, best = R.curves(y, chunk=7)
    np.testing.assert_allclose(sums[0], f1.sum(0), atol=1e-12)
    assert np.array_equal(best[1], f1.argmax(1))


def test_edge_fixture_holds_the_exact_f1_tie():
    d = np.load(os.path.join(REPO, "tests", "golden", "baselines_edge_s40.npz"))
    curve = d["train_curve_f1"]
    assert d["train_labels"].shape[0] == 1
    ties = np.flatnonzero(curve == curve.max())
    assert len(ties) >= 2 and int(d["greedy_k_f1"]) == ties[0] == 1
