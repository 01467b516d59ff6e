#!/usr/bin/env python3
"""Generate tests/golden/baselines_*.npz by RUNNING THE REFERENCE'S Baseline/ notebooks' own functions on generated label sets.

CPU only; run in the build container, where the reference is mounted read-only (RLT_REFERENCE, default /root/reference).
The notebooks are read at run time: from their code cells only the function definitions cal_F1, cal_DCG, test_scores,
greedy_scores and countp are executed (each notebook into a namespace of its own, the module-level statements of those cells -
pickle and ground-truth loading - are not), with `dataset_prepare` replaced by one that returns the generated lists and the
dataset-path constants replaced by tags, so that the notebooks' own driver functions run on them.  Nothing from the reference
is written into this repository: the fixtures hold the labels (uint8) and what the notebook code returned for them (data).

    python tools/make_baseline_golden.py        # regenerates every tests/golden/baselines_*.npz

Each file holds, for a train and a test split of one list length S (300: robust04, 40: mq2007 - the notebooks know only
these two lengths):
    train_labels, test_labels     (n, S) uint8
    best_f1, best_dcg             Oracle.ipynb test_scores on the test split (mean over lists of the best over k = 0..S)
    fixed_k                       (3,) the k of Fixed_k.ipynb's rows (5, 10, 30);  fixed_f1, fixed_dcg: its test_scores there
    greedy_f1, greedy_dcg         Greedy_k.ipynb greedy_scores;  greedy_k_f1, greedy_k_dcg: np.argmax of the train split's mean
                                  curves as that function forms them
    train_curve_f1 / _dcg, test_curve_f1 / _dcg   (S+1,) per-k means over the split's lists (np.mean of the notebooks' arrays;
                                  Truncation_analysis.ipynb's greedy_scores for S = 300)
    countp                        (70,) Truncation_analysis.ipynb countp over train + test (k = 1..70; only k <= S is meaningful)
    train_per_k_f1 / _dcg, test_per_k_f1 / _dcg   (n, S+1) each list's [0] + [cal_F1(list, k) / cal_DCG(list, k), k = 1..S]
"""
import ast
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RLT_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")
WANTED = {"cal_F1", "cal_DCG", "test_scores", "greedy_scores", "countp"}
ROBUST, MQ = "robust04", "mq2007"          # the notebooks' ROBUST_BASE / MQ_BASE, as tags


def notebook_namespace(name, prepare):
    """The wanted function definitions of Baseline/<name>.ipynb executed into a fresh namespace; `prepare` replaces the
    notebook's dataset_prepare (its signature differs per notebook)."""
    with open(os.path.join(REF, "Baseline", name + ".ipynb")) as f:
        nb = json.load(f)
    defs = []
    for cell in nb["cells"]:
        if cell["cell_type"] != "code":
            continue
        src = "".join(cell["source"])
        try:
            tree = ast.parse(src)
        except SyntaxError:                 # notebook-only syntax in cells we do not need
            continue
        defs += [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    import math
    ns = {"math": math, "np": np, "tqdm": lambda it: it, "ROBUST_BASE": ROBUST, "MQ_BASE": MQ, "DATASET_BASE": ROBUST}
    exec(compile(ast.Module(body=defs, type_ignores=[]), f"Baseline/{name}.ipynb", "exec"), ns)
    ns["dataset_prepare"] = prepare
    return ns


def as_dict(labels):
    return {str(i): [int(v) for v in row] for i, row in enumerate(labels)}


def robust_labels(n, S, rs):
    """bench.synth_batch's labels: Bernoulli(0.55 exp(-j/45) + 0.02), at least one positive (the first) per list."""
    prob = 0.55 * np.exp(-np.arange(S) / 45.0) + 0.02
    y = (rs.uniform(size=(n, S)) < prob).astype(np.uint8)
    y[y.sum(1) == 0, 0] = 1
    return y


def mq_labels(n, S, rs):
    """mq2007-like: a few relevant documents per 40, more of them near the top, some lists without any."""
    prob = 0.35 * np.exp(-np.arange(S) / 15.0) + 0.05
    y = (rs.uniform(size=(n, S)) < prob).astype(np.uint8)
    y[rs.uniform(size=n) < 0.1] = 0
    return y


def edge_lists(S):
    rows = [np.zeros(S), np.ones(S)]
    first = np.zeros(S); first[0] = 1
    last = np.zeros(S); last[-1] = 1
    alt1 = (np.arange(S) % 2 == 0).astype(float)          # [1, 0, 1, 0, ...]
    alt0 = 1 - alt1                                        # [0, 1, 0, 1, ...]
    tie = np.zeros(S); tie[[0, 3]] = 1                     # N = 2: F1@1 = F1@4 = 2/3 exactly (first maximum k = 1)
    tie2 = np.zeros(S); tie2[[1, 2, 5]] = 1                # N = 3: F1@3 = F1@6 = 2/3 in exact arithmetic; cal_F1's rounding decides
    block = np.zeros(S); block[5:15] = 1
    tail = np.zeros(S); tail[-3:] = 1
    rows += [first, last, alt1, alt0, tie, tie2, block, tail]
    return np.stack(rows).astype(np.uint8)


def run_set(train, test, S):
    base = ROBUST if S == 300 else MQ
    tr, te = as_dict(train), as_dict(test)
    oracle_ns = notebook_namespace("Oracle", lambda name, b: te)
    fixed_ns = notebook_namespace("Fixed_k", lambda name, b: te)
    greedy_ns = notebook_namespace("Greedy_k", lambda name, b: (tr, te))
    anal_ns = notebook_namespace("Truncation_analysis", lambda name: tr)
    cal_F1, cal_DCG = greedy_ns["cal_F1"], greedy_ns["cal_DCG"]

    def per_k(lists):
        f1 = np.array([[0] + [cal_F1(lists[q], k) for k in range(1, S + 1)] for q in lists], dtype=np.float64)
        dcg = np.array([[0] + [cal_DCG(lists[q], k) for k in range(1, S + 1)] for q in lists], dtype=np.float64)
        return f1, dcg

    out = {"train_labels": train, "test_labels": test}
    out["best_f1"], out["best_dcg"] = oracle_ns["test_scores"]("x", base)
    ks = (5, 10, 30)
    out["fixed_k"] = np.array(ks)
    fx = [fixed_ns["test_scores"]("x", [k] * 2, base) for k in ks]
    out["fixed_f1"], out["fixed_dcg"] = np.array([v[0] for v in fx]), np.array([v[1] for v in fx])
    out["greedy_f1"], out["greedy_dcg"] = greedy_ns["greedy_scores"]("x", base)
    out["train_per_k_f1"], out["train_per_k_dcg"] = per_k(tr)
    out["test_per_k_f1"], out["test_per_k_dcg"] = per_k(te)
    # the mean curves exactly as greedy_scores forms them (np.mean over the notebook's per-list arrays), and its argmax
    out["train_curve_f1"], out["train_curve_dcg"] = out["train_per_k_f1"].mean(0), out["train_per_k_dcg"].mean(0)
    out["test_curve_f1"], out["test_curve_dcg"] = out["test_per_k_f1"].mean(0), out["test_per_k_dcg"].mean(0)
    if S == 300:                            # Truncation_analysis's own greedy_scores knows 300 positions only
        f1m, dcgm = anal_ns["greedy_scores"]("x")
        assert np.array_equal(f1m, out["train_curve_f1"]) and np.array_equal(dcgm, out["train_curve_dcg"])
    out["greedy_k_f1"], out["greedy_k_dcg"] = int(np.argmax(out["train_curve_f1"])), int(np.argmax(out["train_curve_dcg"]))
    # the greedy values follow from the curves at those k (a k of 0 for F1 makes the notebook divide by zero: not generated)
    assert out["greedy_k_f1"] > 0
    assert out["greedy_f1"] == sum([cal_F1(te[q], out["greedy_k_f1"]) for q in te]) / len(te)
    both = dict(tr)
    both.update({"t" + q: v for q, v in te.items()})
    out["countp"] = np.array(anal_ns["countp"](both), dtype=np.float64)
    return {k: (np.asarray(v) if not isinstance(v, np.ndarray) else v) for k, v in out.items()}


def main():
    os.makedirs(OUT, exist_ok=True)
    rs = np.random.RandomState(20241016)
    sets = {
        "baselines_robust04_s300": (robust_labels(64, 300, rs), robust_labels(32, 300, rs), 300),
        "baselines_mq2007_s40": (mq_labels(50, 40, rs), mq_labels(30, 40, rs), 40),
    }
    edge = edge_lists(40)
    sets["baselines_edge_s40"] = (edge[[6]], np.concatenate([edge, mq_labels(6, 40, rs)]), 40)   # one-list train split: the exact tie
    for name, (train, test, S) in sets.items():
        out = run_set(train, test, S)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes, train {train.shape}, test {test.shape}, greedy k "
              f"{int(out['greedy_k_f1'])}/{int(out['greedy_k_dcg'])}, best {float(out['best_f1']):.6f}/{float(out['best_dcg']):.6f}")


if __name__ == "__main__":
    sys.exit(main())
