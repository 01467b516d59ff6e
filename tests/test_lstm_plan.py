"""rlt_bilstm_rec_plan - the one decision the BiLSTM recurrence entry points read - against the rule restated in
tests/lstm_restate.py, over every precision mode (and the process default), both forward forms and the list counts at which the
rule changes; every environment switch of the family, at its non-default value, governs the rows it is documented to govern
(the switches are read once per process: one subprocess each).  No GPU: the plan is host code."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest

import lstm_restate as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 16, 17, 2047, 2048, 2049, 4096, 2 ** 20 - 1, 2 ** 20)
PRECISIONS = ("bf16x6", "fp32", "bf16x3", "default")
SWITCHES = [("RLT_LSTM6", "0"), ("RLT_LSTM6W", "0"), ("RLT_LSTM6W_BWD", "0"), ("RLT_LSTM6W_SINGLE", "0")]
GRID = list(itertools.product(BATCHES, (0, 1), PRECISIONS))


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("RLT_LSTM")}


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def compare(native, sw):
    """Every grid point: the plan equals the restatement.  -> (points, mismatches)"""
    bad = []
    for B, xin, prec in GRID:
        code = native.PRECISION_DEFAULT if prec == "default" else native.precision_code(prec)
        got = native.bilstm_rec_plan(B, xin, code)
        want = R.plan(B, xin, native.get_precision() if prec == "default" else prec, sw)
        if got != want:
            bad.append(((B, xin, prec), got, want))
    return len(GRID), bad


def plans(native):
    return {repr(k): native.bilstm_rec_plan(k[0], k[1], native.PRECISION_DEFAULT if k[2] == "default" else native.precision_code(k[2]))
            for k in GRID}


def test_plan_equals_the_restated_rule(native):
    assert not any(k.startswith("RLT_LSTM") for k in os.environ), "run with the recurrence's switches unset"
    n, bad = compare(native, {})
    assert n == 9 * 2 * 4 and not bad, bad[:5]


def test_plan_names_every_kernel_and_both_list_counts(native):
    seen = {(p["fwd"], p["fwd_lists"]) for p in plans(native).values()} | {(p["bwd"], p["bwd_lists"]) for p in plans(native).values()}
    want = {("f32", 32), ("x3", 32), ("x6", 32), ("x6w_single", 16), ("x6w_halves", 32)}
    assert seen == want, seen
    # the default switches at the boundaries the dispatch test runs on the device
    x6 = native.PRECISION_BF16X6
    assert native.bilstm_rec_plan(2048, 0, x6) == dict(fwd="x6w_single", bwd="x6w_single", fwd_lists=16, bwd_lists=16)
    assert native.bilstm_rec_plan(2049, 1, x6) == dict(fwd="x6w_halves", bwd="x6w_halves", fwd_lists=32, bwd_lists=32)
    assert native.bilstm_rec_plan(2 ** 20, 0, x6) == dict(fwd="x6", bwd="f32", fwd_lists=32, bwd_lists=32)


def test_plan_argument_errors(native):
    lib, plan = native.load(), native.BilstmRecPlan()
    ref = ctypes.byref(plan)
    assert lib.rlt_bilstm_rec_plan(64, 0, -1, None) == -1
    assert lib.rlt_bilstm_rec_plan(0, 0, -1, ref) == -1
    assert lib.rlt_bilstm_rec_plan(-5, 1, -1, ref) == -1
    assert lib.rlt_bilstm_rec_plan(64, 2, -1, ref) == -1
    assert lib.rlt_bilstm_rec_plan(64, 0, 7, ref) == -1
    assert lib.rlt_bilstm_rec_plan(64, 0, -1, ref) == 0


_CHILD = """
import json, sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import test_lstm_plan as T
from rlt_hip import native
native.load()
n, bad = T.compare(native, {sw!r})
base = json.load(open({base!r}))
changed = sum(1 for key, p in T.plans(native).items() if base[key] != p)
print(json.dumps({{"n": n, "bad": [repr(b) for b in bad[:5]], "changed": changed}}))
"""


@pytest.fixture(scope="module")
def default_plans(native, tmp_path_factory):
    path = tmp_path_factory.mktemp("lstm_plan") / "default.json"
    path.write_text(json.dumps(plans(native)))
    return str(path)


@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{n}={v}" for n, v in SWITCHES])
def test_switch_governs_its_rows(native, default_plans, name, value):
    """with the switch set, the plan equals the restatement given that switch - and differs from the default plan somewhere"""
    env = _clean_env()
    env[name] = value
    code = _CHILD.format(tests=os.path.join(REPO, "tests"), pkg=os.path.join(REPO, "ranked-list-truncation_amd"),
                         sw={name: value}, base=default_plans)
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["n"] == len(GRID) and not out["bad"], out["bad"]
    assert out["changed"] > 0, f"{name}={value} changed no row of the plan"
