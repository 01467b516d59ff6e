"""rlt_probe_heads (the probing study's fused probe-head pass) without a GPU: the symbols are declared, bound and exported,
every argument error is answered before a launch, the workspace query is host arithmetic; the probe model classes mirror the
reference's state_dict (tests/golden/probe_models_s40.npz) and the stock torch modules' initialisation; the fixtures agree
with the independent float64 restatement of tests/probe_restate.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_restate as R  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
SYMS = ("rlt_probe_heads", "rlt_probe_heads_workspace")


def _gold(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_probe_symbols_declared_bound_exported(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    lib = native.load()
    for s in SYMS:
        assert s in native.EXPORTS and hasattr(lib, s), s
    assert re.search(r"#define RLT_PROBE_BCE\s+0\b", header) and re.search(r"#define RLT_PROBE_RERANK\s+1\b", header)
    assert (native.PROBE_BCE, native.PROBE_RERANK) == (0, 1)
    assert lib.rlt_abi_version() == 5


def test_probe_workspace_query_needs_no_device(native):
    q = lambda *a: native.query("rlt_probe_heads_workspace", *a)   # noqa: E731
    assert q(2, 300, 4096, 256) == 4097 * (2 * 256 + 3 * 2 + 2) * 4
    assert q(8, 1024, 1, 1024) == 2 * (8 * 1024 + 26) * 4
    for bad in ((0, 300, 4, 256), (9, 300, 4, 256), (2, 0, 4, 256), (2, 1025, 4, 256), (2, 300, 0, 256), (2, 300, 4, 0),
                (2, 300, 4, 1025)):
        assert q(*bad) == 0, bad


def test_probe_argument_errors(native):
    lib = native.load()
    S, B, E = 40, 3, 25
    wsb = native.query("rlt_probe_heads_workspace", 2, S, B, E)
    buf = (ctypes.c_uint8 * (wsb + 4096))()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    kinds = (ctypes.c_int * 2)(0, 1)
    bad_kind = (ctypes.c_int * 2)(0, 2)

    def run(x=p, w=p, b=p, k=kinds, n=2, s=S, bb=B, e=E, y=p, loss=p, dw=p, db=p, out=p, ws=p, wsn=wsb):
        return lib.rlt_probe_heads(x, w, b, k, n, s, bb, e, y, 5e-4, loss, dw, db, out, ws, wsn, None)
    for kw in ({"x": None}, {"w": None}, {"b": None}, {"k": None}, {"y": None}, {"loss": None}, {"ws": None},
               {"dw": None}, {"db": None}, {"n": 0}, {"s": 0}, {"bb": 0}, {"e": 0}, {"k": bad_kind}):
        assert run(**kw) == -1, kw
    for kw in ({"n": 9}, {"s": 1025}, {"e": 1025}):
        assert run(**kw) == -2, kw
    assert run(wsn=wsb - 1) == -3


def test_probe_models_mirror_reference_state_dict():
    import models as hm
    g = _gold("probe_models_s40")
    for name, ctor in (("TaskC", lambda: hm.TaskC()), ("TaskR", lambda: hm.TaskR()),
                       ("ProbeBase", lambda: hm.ProbeBase(seq_len=40)), ("Probe", lambda: hm.Probe())):
        sd = ctor().state_dict()
        assert list(sd.keys()) == list(g[f"keys/{name}"]), name
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g[f"shapes/{name}"]), name
    with pytest.raises(ValueError):
        hm.ProbeBase(seq_len=40, num_tasks=4)
    assert len(hm.ProbeBase(seq_len=40, num_tasks=2.1).w_gates) == 2
    assert len(hm.ProbeBase(seq_len=40, num_tasks=2.1).towers) == 3


def test_probe_models_initialise_like_the_stock_modules():
    import models as hm
    from torch import nn
    for cls in (hm.TaskC, hm.TaskR):
        for E in (3, 256):
            torch.manual_seed(11)
            a = cls(d_model=E)
            torch.manual_seed(11)
            b = nn.Linear(E, 1)
            assert torch.equal(a.linear.weight, b.weight) and torch.equal(a.linear.bias, b.bias)
    torch.manual_seed(5)
    p = hm.Probe()
    torch.manual_seed(5)
    ref = [nn.Linear(256, 1) for _ in range(6)]
    for m, r in zip((p.probe_c1, p.probe_r1, p.probe_ce1, p.probe_ce2, p.probe_re1, p.probe_re2), ref):
        assert torch.equal(m.linear.weight, r.weight)


@pytest.mark.parametrize("S", [40, 300])
def test_fixtures_agree_with_float64_restatement(S):
    import models as hm
    from oracle.weights import fill_state_dict
    g = _gold(f"probe_heads_s{S}")
    tags = sorted({k.split("/")[0] for k in g if not k.startswith("adam")})
    assert len(tags) == 4
    for tag in tags:
        B, S_, E = (int(v) for v in g[f"{tag}/shape"])
        model = (hm.TaskC if tag[0] == "c" else hm.TaskR)(d_model=E)
        fill_state_dict(model, int(g[f"{tag}/seed"]))
        x, y = R.probe_data(int(g[f"{tag}/seed"]) + 1, B, S_, E)
        w, b = model.linear.weight.detach().numpy()[0], float(model.linear.bias.detach()[0])
        loss, dw, db, out = R.head(R.BCE if tag[0] == "c" else R.RERANK, x, y, w, b)
        np.testing.assert_allclose(out, g[f"{tag}/out"], rtol=1e-5, atol=1e-7 * np.abs(out).max(), err_msg=tag)
        assert abs(loss - float(g[f"{tag}/loss"])) <= 1e-5 * max(abs(loss), 1e-3), tag
        scale = np.abs(dw).max() + 1e-30
        np.testing.assert_allclose(g[f"{tag}/dw"], dw, rtol=0, atol=1e-5 * scale, err_msg=tag)
        assert abs(float(g[f"{tag}/db"][0]) - db) <= 1e-5 * max(scale, abs(db)), tag


@pytest.mark.parametrize("script,flags", [
    ("verify_BMT.py", ["--retrieve-data", "--dataset-name", "--batch-size", "--num-workers", "--model-name", "--verify-type",
                       "--model-path", "--save-path", "--ft", "--epochs", "--lr", "--weight-decay", "--dropout",
                       "--dataset-base", "--synthetic", "--seed", "--history-json", "--tensorboard-dir", "--trunk-eval"]),
    ("verify_probe.py", ["--retrieve-data", "--dataset-name", "--batch-size", "--num-workers", "--model-name", "--criterion",
                         "--model-path", "--ft", "--save-path", "--epochs-base", "--epochs-probe", "--lr", "--weight-decay",
                         "--dropout", "--parameter-record", "--parameter-search", "--regularizer-search", "--mt-search",
                         "--search-times", "--num-tasks", "--rerank-weight", "--class-weight", "--dataset-base", "--synthetic",
                         "--seed", "--history-json", "--tensorboard-dir", "--accumulate-grads"])])
def test_probe_scripts_offer_the_reference_flags(script, flags):
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(REPO, "ranked-list-truncation_amd", script), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    for f in flags:
        assert f in res.stdout, (script, f)
