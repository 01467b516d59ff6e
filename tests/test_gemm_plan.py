"""rlt_gemm_plan - the one decision rlt_gemm / rlt_gemm_ex / rlt_gemm_bits read - against the documented rules restated in
tests/gemm_plan_restate.py: every id of the dispatch case table (tests/gemm_cases.py), a boundary grid with one value on each side
of every rule in all precision modes and operand layouts, rlt_gemm_workspace against the plan's bytes, and every environment switch
of the family at a non-default value (the switches are read once per process: one subprocess each).  No GPU: the plan is host code.

The grid is SHAPES x FEATURES x modes x layouts x workspace (given / null / short); what each shape is there for is said next to it."""
import ast
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest

import gemm_plan_restate as R
from gemm_cases import ACC, CASES, LAYOUTS, MODES, RELU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [
    (128, 128, 1023), (128, 128, 1024), (256, 256, 992), (256, 256, 1024),      # the split minimum
    (2048, 2048, 992), (2048, 2048, 1024),                                      # gemm6e from K = 1024 with A stored [M][K] (no split)
    (1920, 2176, 2048), (2048, 2048, 2048),                                     # 255 / 256 output tiles of 128 x 128
    (128, 128, 4095), (128, 128, 4096), (256, 256, 4064), (256, 256, 4096),     # 256 / 512 of K kept per slab
    (256, 9344, 8192), (1024, 2048, 8192), (128, 14464, 8192),                  # 7 / 8 / 9 slabs wanted: 9 is rounded to 8, 7 stays
    (256, 256, 32), (256, 256, 64), (256, 256, 96),                             # slabs of one, two, three K tiles
    (256, 256, 12544), (256, 256, 12576), (256, 256, 1184), (128, 128, 1030),   # a last slab of 32, of 64, a short one, a ragged one
    (128, 128, 65600),                                                          # 128 slabs wanted, 121 after rounding the slab to 32
    (256, 384, 64), (256, 320, 64), (384, 256, 64),                             # N % 256, N % 128, M % 256
    (8191, 256, 256), (8192, 256, 256), (8192, 65536, 256), (8192, 65792, 256),       # gemm6s: M from 8192, N to 65536
    (8192, 256, 128), (8192, 384, 128), (8192, 384, 256), (8192, 320, 128), (8192, 256, 192), (8223, 2048, 256),
    (4096, 4096, 64), (4352, 4096, 64), (4352, 4096, 32), (4352, 4096, 1024),   # 256 / 272 tiles of 256 x 256: the persistent forms
    (132, 136, 40), (132, 136, 38), (132, 136, 3), (129, 136, 40), (132, 130, 40), (5, 136, 40), (3, 136, 40), (132, 3, 40),   # the loaders
]
# what a call carries beside its shape: every epilogue feature gemm6e or gemm6s excludes, every cause of the guarded loaders
FEATURES = [
    dict(), dict(present=("bias",)), dict(present=("bias", "bias2"), flags=RELU), dict(flags=ACC), dict(present=("relu_mask",)),
    dict(present=("colsum",)), dict(drop=True), dict(present=("bias", "bits_out"), flags=RELU), dict(present=("bits_out",)),
    dict(present=("bits_in",)), dict(present=("bits_in", "bias")), dict(present=("bits_in",), flags=RELU), dict(present=("bits_in", "bits_out")),
    dict(lda_pad=5), dict(ldb_pad=5), dict(ldc_pad=5), dict(lda_pad=2 ** 24), dict(ldc_pad=2 ** 24),
    dict(misaligned=("A",)), dict(misaligned=("B",)), dict(misaligned=("C",)), dict(present=("bias",), misaligned=("bias",)),
    dict(present=("bias", "bias2"), misaligned=("bias2",)), dict(present=("bits_out",), flags=RELU, misaligned=("bits_out",)),
    dict(present=("bits_in",), misaligned=("bits_in",)), dict(misaligned=("bias", "bias2", "bits_out", "bits_in")),      # absent: not read
]
WORKSPACES = ("given", "null", "short")
PRECISIONS = tuple(MODES)
# every switch at a non-default value (RLT_GEMM_MODE has two)
SWITCHES = [("RLT_GEMM_MODE", "fp32"), ("RLT_GEMM_MODE", "bf16x3"), ("RLT_GEMM_NOFAST", "1"), ("RLT_GEMM_NO_BIG", "1"), ("RLT_GEMM_PERSIST", "248"),
            ("RLT_GEMM_PERSIST_NN", "1"), ("RLT_GEMM6_PERSIST", "248"), ("RLT_GEMM6_SMALL", "1"), ("RLT_GEMM6C", "0"), ("RLT_GEMM6E", "0"),
            ("RLT_GEMM6E_ALL", "1"), ("RLT_GEMM6S", "0"), ("RLT_GEMM_SPLIT_KMIN", "2048"), ("RLT_GEMM_SPLIT_TARGET", "512"),
            ("RLT_GEMM_NO_SLAB_XCD", "1")]
# the rows a switch is documented to govern, as a predicate on (key, the row's plan under the default switches): no other row may move
_split = lambda key, p: p["rc"] != 0 or (p["family"] != "gemm6s" and "bits" not in repr(dict(ast.literal_eval(key)[3]).get("present")))
GOVERNS = {
    "RLT_GEMM_MODE=fp32": lambda key, p: "'fp32'" not in key, "RLT_GEMM_MODE=bf16x3": lambda key, p: "'bf16x3'" not in key,
    "RLT_GEMM_NOFAST": lambda key, p: p["family"] in ("gemm", "gemm3") and p["fast"] == 1,
    "RLT_GEMM_NO_BIG": lambda key, p: p["family"] == "gemm3b",
    "RLT_GEMM_PERSIST": lambda key, p: p["family"] == "gemm3b" and p["ta"] == 0 and p["ns"] == 1,
    "RLT_GEMM_PERSIST_NN": lambda key, p: p["family"] == "gemm3b" and (p["ta"], p["tb"], p["ns"]) == (0, 0, 1),
    "RLT_GEMM6_PERSIST": lambda key, p: p["family"] in ("gemm6c", "gemm6e") and p["ta"] == 0 and p["ns"] == 1,
    "RLT_GEMM6_SMALL": lambda key, p: p["family"] in ("gemm6b", "gemm6c", "gemm6e"),
    "RLT_GEMM6C": lambda key, p: p["family"] in ("gemm6c", "gemm6e"),
    "RLT_GEMM6E": lambda key, p: p["family"] == "gemm6e",
    "RLT_GEMM6E_ALL": lambda key, p: p["family"] == "gemm6c" and p["ta"] == 0,
    "RLT_GEMM6S": lambda key, p: p["family"] == "gemm6s" or p["rc"] == -1,
    "RLT_GEMM_SPLIT_KMIN": _split, "RLT_GEMM_SPLIT_TARGET": _split,
    "RLT_GEMM_NO_SLAB_XCD": lambda key, p: p["slab_xcd"] == 1,
}


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("RLT_GEMM")}


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def describe(ta, tb, M, N, K, ws="given", flags=0, present=(), misaligned=(), drop=False, lda_pad=0, ldb_pad=0, ldc_pad=0):
    """a call of the grid as the dict tests/gemm_plan_restate.py reads; the workspace is sized by the default switches' rule"""
    need = R.workspace_bytes(M, N, K)
    return dict(ta=ta, tb=tb, M=M, N=N, K=K, lda=(M if ta else K) + lda_pad, ldb=(K if tb else N) + ldb_pad, ldc=N + ldc_pad, flags=flags,
                present=present, misaligned=misaligned, drop=drop, ws_bytes=None if ws == "null" else need - 4 if ws == "short" and need else need)


def grid():
    """-> (key, call, precision) over the whole grid; a column sum only where A is stored [K][M] (else: an argument error)"""
    for (M, N, K), feat, prec, (lay, (ta, tb)), ws in itertools.product(SHAPES, FEATURES, PRECISIONS, LAYOUTS.items(), WORKSPACES):
        if "colsum" in feat.get("present", ()) and not ta:
            continue
        yield repr((M, N, K, sorted(feat.items()), prec, lay, ws)), describe(ta, tb, M, N, K, ws, **feat), prec


def ask(native, call, prec):
    rc, rec = native.gemm_plan(native.gemm_call(**call), native.precision_code(prec))
    return dict(rec, rc=rc)


def compare(native, sw):
    """Every grid point: return code and record equal the restatement.  -> (the plans by key, mismatches)"""
    bad, plans = [], {}
    for key, call, prec in grid():
        rc, rec = R.plan(call, prec, sw)
        got = plans[key] = ask(native, call, prec)
        if got != dict(rec, rc=rc):
            bad.append((key, got, dict(rec, rc=rc)))
    return plans, bad


@pytest.fixture(scope="module")
def default_plans(native):
    assert not any(k.startswith("RLT_GEMM") for k in os.environ), "run with the GEMM switches unset"
    return compare(native, {})


def case_call(c, ws="given"):
    """a row of the case table as tests/test_gemm_dispatch_gpu.py launches it: leading dimensions padded to 4 and by 4 more, an operand
    or bias one float off its allocation, rlt_gemm_bits without bias2 and workspace"""
    M, N, K, up4 = c["M"], c["N"], c["K"], lambda n: (n + 3) // 4 * 4
    bits = c.get("bits")
    present = [n for n in ("bias", "bias2") if c.get(n) and not (bits and n == "bias2")] + [f"bits_{bits}"] * bool(bits) + \
              ["relu_mask"] * bool(c.get("mask")) + ["colsum"] * bool(c.get("colsum"))
    misaligned = ["A"] * c.get("a_off", 0) + ["B"] * c.get("b_off", 0) + ["bias"] * c.get("bias_off", 0)
    call = describe(c["ta"], c["tb"], M, N, K, "null" if bits else c.get("ws", ws), (RELU if c.get("relu") else 0) | (ACC if c.get("acc") else 0),
                    tuple(present), tuple(misaligned), bool(c.get("drop")))
    return dict(call, lda=up4(M if c["ta"] else K) + c.get("lda_pad", 4), ldb=up4(K if c["tb"] else N) + c.get("ldb_pad", 4), ldc=up4(N) + 4)


@pytest.mark.parametrize("name", list(CASES))
def test_case_table_id_reaches_the_kernel_it_names(native, name):
    c = CASES[name]
    got = ask(native, case_call(c), c["mode"])
    assert got["rc"] == 0 and {k: got[k] for k in c["want"]} == c["want"], (name, c["want"], got)
    rc, rec = R.plan(case_call(c), c["mode"])
    assert got == dict(rec, rc=rc), (name, got, rec)


def test_plan_equals_the_restated_rules(default_plans):
    plans, bad = default_plans
    assert len(plans) > 40000 and not bad, (len(bad), bad[:5])


def test_grid_has_a_point_on_each_side_of_every_rule(native, default_plans):
    """the default-switch grid names every family, both loader forms, both persistent answers, pinned and unpinned slabs, every
    gemm6s epilogue and panel form, every return code - and the slab counts the shapes are there for"""
    seen = default_plans[0]
    col = lambda f: {p[f] for p in seen.values()}
    assert col("family") == set(native.GEMM_FAMILIES), col("family")
    assert col("rc") == {0, -1, R.E_WORKSPACE} and col("fast") == col("persistent") == col("slab_xcd") == col("narrow") == {0, 1}
    assert col("epilogue") == {0, 1, 2, 3}
    assert {4, 7, 8, 24, 121} <= col("ns") and 9 not in col("ns"), sorted(col("ns"))
    for fam in ("gemm3b", "gemm6c", "gemm6e"):
        assert {p["persistent"] for p in seen.values() if p["family"] == fam} == {0, 1}, fam
    for fam in native.GEMM_FAMILIES[1:8]:
        assert {(p["ta"], p["tb"]) for p in seen.values() if p["family"] == fam} == set(LAYOUTS.values()), fam


def test_workspace_query_is_the_plans_split(native):
    """rlt_gemm_workspace = the bytes of the split the shape wants: a call given them gets that split, a call given less is refused"""
    for (M, N, K), (ta, tb) in itertools.product(SHAPES, LAYOUTS.values()):
        need = native.query("rlt_gemm_workspace", ta, tb, M, N, K)
        assert need == R.workspace_bytes(M, N, K), (M, N, K, need)
        for prec in PRECISIONS:
            got = ask(native, describe(ta, tb, M, N, K), prec)
            assert got["rc"] == 0 and (got["ns"] > 1) == (need > 0), (M, N, K, prec, got)
            if need:
                assert got["family"] != "gemm6s" and need >= (got["ns"] * M * N + got["ns"] * M) * 4
                assert ask(native, dict(describe(ta, tb, M, N, K), ws_bytes=need - 1), prec)["rc"] == R.E_WORKSPACE
    assert native.query("rlt_gemm_workspace", 0, 0, 0, 128, 4096) == 0 and native.query("rlt_gemm_workspace", 0, 0, 128, 128, -1) == 0


def test_plan_argument_errors(native):
    """the codes rlt_gemm / rlt_gemm_ex return for the same arguments"""
    lib, rec = native.load(), native.GemmDispatch()
    code = lambda call, prec=-1: lib.rlt_gemm_plan(ctypes.byref(call) if call is not None else None, prec, ctypes.byref(rec))
    good = dict(ta=0, tb=1, M=128, N=128, K=64)
    assert code(native.gemm_call(**good)) == 0 and code(native.gemm_call(**good), 2) == 0
    assert lib.rlt_gemm_plan(ctypes.byref(native.gemm_call(**good)), -1, None) == R.E_ARG
    assert code(None) == R.E_ARG and code(native.gemm_call(**good), 7) == R.E_ARG
    for bad in (dict(M=0), dict(N=-1), dict(K=0), dict(lda=63), dict(ldb=63), dict(ldc=127), dict(present=("colsum",))):
        assert code(native.gemm_call(**dict(good, **bad))) == R.E_ARG, bad
    assert code(native.gemm_call(**dict(good, ta=1, lda=127))) == R.E_ARG
    assert code(native.gemm_call(**dict(good, ta=1, lda=128, present=("colsum",)))) == 0
    # a workspace pointer that is NULL with a byte count is short, not absent
    call = native.gemm_call(0, 1, 128, 128, 2048)
    assert code(call) == 0 and rec.ns == 1
    call.ws_bytes = 64
    assert code(call) == R.E_WORKSPACE and rec.family == 0


_CHILD = """
import json, sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import test_gemm_plan as T
from rlt_hip import native
native.load()
plans, bad = T.compare(native, {sw!r})
base = json.load(open({base!r}))
governs = T.GOVERNS.get({name!r}) or T.GOVERNS[{name!r} + "=" + {value!r}]
moved = [key for key, p in plans.items() if base[key] != p]
print(json.dumps({{"n": len(plans), "bad": [repr(b) for b in bad[:5]], "changed": len(moved), "stray": [k for k in moved if not governs(k, base[k])][:5]}}))
"""


@pytest.fixture(scope="module")
def default_file(default_plans, tmp_path_factory):
    path = tmp_path_factory.mktemp("gemm_plan") / "default.json"
    path.write_text(json.dumps(default_plans[0]))
    return str(path)


@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{n}={v}" for n, v in SWITCHES])
def test_switch_governs_its_rows(native, default_file, name, value):
    """with the switch set, the plan equals the restatement given that switch, differs from the default plan somewhere, and only in
    rows the switch is documented to govern"""
    env = _clean_env()
    env[name] = value
    code = _CHILD.format(tests=os.path.join(REPO, "tests"), pkg=os.path.join(REPO, "ranked-list-truncation_amd"),
                         sw={name: value}, base=default_file, name=name, value=value)
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["n"] > 40000 and not out["bad"], out["bad"]
    assert out["changed"] > 0, f"{name}={value} changed no row of the plan"
    assert not out["stray"], f"{name}={value} moved rows it does not govern: {out['stray']}"
