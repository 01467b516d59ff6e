"""rlt_list_attention_plan - the one decision the list-attention entry points read - against the documented rules restated in
tests/attn_plan_restate.py, over every precision mode, dropout on / off, images given / not given and the list counts at which
a rule changes; the public workspace queries return the plan's bytes; every environment switch of the family, at its
non-default value, governs the rows it is documented to govern (the switches are read once per process: one subprocess each).
No GPU: the plan is host code."""
import itertools
import json
import os
import subprocess
import sys

import pytest

import attn_plan_restate as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("fp32", "bf16x3", "bf16x6")
SHAPES = ([(S, B, H, HD) for (HD, B) in R.GRID for H in (1, 2) for S in (1, 3)] + [R.NON_SMALL24])
# every switch at its non-default value (RLT_ATTN_MODE has two)
SWITCHES = [("RLT_ATTN_MODE", "fp32"), ("RLT_ATTN_MODE", "bf16x3"), ("RLT_ATTN6", "0"), ("RLT_ATTN6_IMG", "1"), ("RLT_ATTN16", "0"),
            ("RLT_A6N", "0"), ("RLT_A6N_1", "0"), ("RLT_A6N_IMG", "0"), ("RLT_A6N_F1", "0"), ("RLT_A6H", "0"), ("RLT_A6_PP", "0"),
            ("RLT_A6_DKV1", "0"), ("RLT_A6_DQ1", "0"), ("RLT_ATTN_SB", "0"), ("RLT_ATTN_SB_DQ", "1"), ("RLT_DKV_OCC", "1")]


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def compare(native, sw):
    """Every grid point: the plan equals the restatement, the public queries return the plan's layout.  -> (points, mismatches)"""
    bad, n = [], 0
    for (S, B, H, HD), prec, drop_p, have in itertools.product(SHAPES, PRECISIONS, (0.0, 0.1), (0, 1)):
        code = native.precision_code(prec)
        got = native.attention_plan(S, B, H, HD, drop_p, have, code)
        want = R.plan(S, B, H, HD, drop_p, have, prec, sw)
        n += 1
        if got != want:
            bad.append(((S, B, H, HD, prec, drop_p, have), {k: (got[k], want.get(k)) for k in got if got[k] != want.get(k)}))
        queries = (native.query("rlt_list_attention_fwd_workspace", S, B, H, HD, drop_p, code),
                   native.query("rlt_list_attention_bwd_workspace", S, B, H, HD, drop_p, code),
                   native.load().rlt_list_attention_images_retained(S, B, H, HD, code))
        if queries != (got["images_bytes"], got["ws_bytes"], got["images_retained"]):
            bad.append(((S, B, H, HD, prec, drop_p, have), {"queries": queries}))
    return n, bad


def test_plan_equals_the_restated_rules(native):
    assert not any(k.startswith("RLT_A") or k == "RLT_DKV_OCC" for k in os.environ), "run with the attention switches unset"
    n, bad = compare(native, {})
    assert n == len(SHAPES) * 12 and not bad, bad[:5]


def test_plan_names_every_default_kernel(native):
    """the grid reaches every kernel the default switches can select (the rest: test_switch_governs_its_rows)"""
    seen = set()
    for (S, B, H, HD), prec, drop_p, have in itertools.product(SHAPES, PRECISIONS, (0.0, 0.1), (0, 1)):
        p = native.attention_plan(S, B, H, HD, drop_p, have, native.precision_code(prec))
        seen |= {p["fwd"], p["fwd_fixup"], p["dkv"], p["dq"]}
    assert seen == set(native.ATTN_KERNELS) - {"x6_img", "x6_pp_img"}, seen


def test_plan_argument_errors(native):
    lib, plan = native.load(), native.AttentionPlan()
    import ctypes
    ref = ctypes.byref(plan)
    assert lib.rlt_list_attention_plan(1, 64, 1, 64, 0.0, 1, -1, None) == -1
    assert lib.rlt_list_attention_plan(0, 64, 1, 64, 0.0, 1, -1, ref) == -1
    assert lib.rlt_list_attention_plan(1, 64, 1, 64, 1.0, 1, -1, ref) == -1
    assert lib.rlt_list_attention_plan(1, 64, 1, 64, 0.0, 1, 7, ref) == -1
    assert lib.rlt_list_attention_plan(1, 64, 1, 48, 0.0, 1, -1, ref) == -2


_CHILD = """
import json, sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import test_attention_plan as T
from rlt_hip import native
native.load()
n, bad = T.compare(native, {sw!r})
base = json.load(open({base!r}))
changed = sum(1 for key, p in T.plans(native).items() if base[key] != p)
print(json.dumps({{"n": n, "bad": [repr(b) for b in bad[:5]], "changed": changed}}))
"""


def plans(native):
    out = {}
    for (S, B, H, HD), prec, drop_p, have in itertools.product(SHAPES, PRECISIONS, (0.0, 0.1), (0, 1)):
        p = native.attention_plan(S, B, H, HD, drop_p, have, native.precision_code(prec))
        out[repr((S, B, H, HD, prec, drop_p, have))] = {k: list(v) if isinstance(v, tuple) else v for k, v in p.items()}
    return out


@pytest.fixture(scope="module")
def default_plans(native, tmp_path_factory):
    path = tmp_path_factory.mktemp("attn_plan") / "default.json"
    path.write_text(json.dumps(plans(native)))
    return str(path)


@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{n}={v}" for n, v in SWITCHES])
def test_switch_governs_its_rows(native, default_plans, name, value):
    """with the switch set, the plan equals the restatement given that switch - and differs from the default plan somewhere"""
    env = {k: v for k, v in os.environ.items() if not (k.startswith("RLT_A") or k == "RLT_DKV_OCC")}
    env[name] = value
    code = _CHILD.format(tests=os.path.join(REPO, "tests"), pkg=os.path.join(REPO, "ranked-list-truncation_amd"),
                         sw={name: value}, base=default_plans)
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["n"] == len(SHAPES) * 12 and not out["bad"], out["bad"]
    assert out["changed"] > 0, f"{name}={value} changed no row of the plan"
