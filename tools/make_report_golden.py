#!/usr/bin/env python3
"""Generate tests/golden/report_*.npz by RUNNING THE REFERENCE'S OWN `Trainer.plot` arithmetic (run.py:242-298) and BiCut cut
branch (run.py:172-177) on the committed label sets.

CPU only; run where the reference is mounted read-only (RLT_REFERENCE, default /root/reference).  The reference's run.py cannot
be imported as a module here (it imports tensorboardX and its data loaders at the top), so it is read at run time and only the
`Trainer.plot` function definition and the BiCut branch of `Trainer.test` are executed - unbound, with a stub `self` and a stub `plt` that captures the plotted arrays -
against the reference's own utils/metrics.py `Metric_for_Loss`.  Nothing from the reference is written into this repository:
the fixtures hold labels, generated outputs and what the reference code returned for them (data).

    python tools/make_report_golden.py          # regenerates every tests/golden/report_*.npz

Each file holds: labels (B,S) uint8; output (B,S) float32, a softmax over positions whose maximum stays under 0.07 so that the
reference's fp32 exp(output / 9e-4) is finite; tau; reward_f1, reward_dcg (S,) float32 = the plotted `norm_r` with the
criterion read as f1 / as dcg; pred (S,) float32 = the plotted `norm_s` (with the figure's norm_s[-3:] = norm_s[-4]).
report_bicut_s40.npz holds instead: labels, output2 (B,S,2) float32 (tests/golden/bicut_b8_s40_in5.npz's reference output with
two rows edited to cover a tie and a list that never truncates), k (B,) int32 from the reference's loop.
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RLT_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")
TAU = 0.9


def reference_plot():
    """`Trainer.plot` of the reference's run.py as a plain function, and the list the stub `plt.plot` appends to."""
    with open(os.path.join(REF, "run.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Trainer")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "plot")
    # utils/metrics.py:3 imports numpy.lib.financial (unused, dropped by modern numpy): an empty stand-in, as tools/make_golden.py does
    sys.modules.setdefault("numpy.lib.financial", types.ModuleType("numpy.lib.financial")).irr = None
    sys.path.insert(0, REF)
    from utils.metrics import Metric_for_Loss          # the reference's own
    sys.path.pop(0)
    plotted = []
    plt = types.SimpleNamespace(plot=lambda x, y, **kw: plotted.append(y.clone()), cla=lambda: None, figure=lambda **kw: None,
                                grid=lambda **kw: None, legend=lambda **kw: None, title=lambda *a, **kw: None,
                                xlabel=lambda *a, **kw: None, savefig=lambda *a, **kw: None)
    import random
    ns = {"t": torch, "os": os, "plt": plt, "random": random, "Metric_for_Loss": Metric_for_Loss}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "run.py", "exec"), ns)
    return ns["plot"], plotted


def reference_bicut_k(output2, seq_len):
    """The k of the reference's own BiCut branch (run.py, `Trainer.test`: the body of `if self.model_name == 'bicut':`), read
    from the reference's file at run time and executed on `output2` with a stub `self`; nothing of it is kept here."""
    with open(os.path.join(REF, "run.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Trainer")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "test")
    is_bicut = lambda n: isinstance(n, ast.If) and "'bicut'" in ast.unparse(n.test)
    branch = next(n for n in ast.walk(fn) if is_bicut(n))
    ns = {"np": np, "self": types.SimpleNamespace(seq_len=seq_len), "output": torch.from_numpy(np.ascontiguousarray(output2))}
    exec(compile(ast.Module(body=branch.body, type_ignores=[]), "run.py", "exec"), ns)
    return np.asarray(ns["k_s"], dtype=np.int32)


def main():
    plot, plotted = reference_plot()
    sets = {}
    for name in ("edge_s40", "mq2007_s40", "robust04_s300"):
        d = np.load(os.path.join(OUT, f"baselines_{name}.npz"))
        sets[name] = np.concatenate([d["train_labels"], d["test_labels"]]).astype(np.float32)
    sets["losses_edge_s300"] = np.load(os.path.join(OUT, "losses_edge_s300.npz"))["y"].astype(np.float32)
    rng = np.random.default_rng(20240917)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                                   # the reference makes ./figs/ where it runs
        try:
            for name, y in sets.items():
                B, S = y.shape
                logits = rng.normal(0.0, 0.2, size=(B, S)).astype(np.float32)
                logits[0, 3] = logits[0, 17] = logits[0].max() + 0.1       # a duplicated maximum
                out = torch.softmax(torch.from_numpy(logits), dim=1)
                assert float(out.max()) < 0.07, float(out.max())
                res = {}
                for crit in ("f1", "dcg"):
                    del plotted[:]
                    stub = types.SimpleNamespace(seq_len=S, criterion=crit, model_name="attncut", div_type="js", aug_reward=1)
                    plot(stub, torch.from_numpy(y), out.clone(), 0, tau=TAU, single_sample=False)
                    res[f"reward_{crit}"], res["pred"] = plotted[0].numpy(), plotted[1].numpy()
                    assert np.isfinite(plotted[0].numpy()).all() and np.isfinite(plotted[1].numpy()).all()
                np.savez_compressed(os.path.join(OUT, f"report_{name}.npz"), labels=y.astype(np.uint8), output=out.numpy(),
                                    tau=np.float64(TAU), **res)
                print(name, y.shape)
        finally:
            os.chdir(cwd)
    d = np.load(os.path.join(OUT, "bicut_b8_s40_in5.npz"))
    out2 = d["out0"].astype(np.float32).copy()
    assert np.array_equal(reference_bicut_k(out2, out2.shape[1]), d["k_s"])
    out2[1, :, 0], out2[1, :, 1] = 0.25, 0.75            # never truncates: k = S
    out2[2, :, 0], out2[2, :, 1] = 0.4, 0.6
    out2[2, 11] = 0.5                                   # a tie: class 0, k = 12
    np.savez_compressed(os.path.join(OUT, "report_bicut_s40.npz"), labels=d["y"].astype(np.uint8), output2=out2,
                        k=reference_bicut_k(out2, out2.shape[1]))
    print("bicut", out2.shape)


if __name__ == "__main__":
    main()
