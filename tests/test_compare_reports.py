"""The host side of the report comparison without a device: the join of compare_reports on (qid, length) with permuted rows, the
Oracle baseline, the compare_reports.py command line with its JSON file, and Trainer.compare.  PairedComparison is replaced by a
recorder that keeps what it is given (the device pass itself is tested in tests/test_compare_gpu.py).  No GPU."""
import json
import types

import numpy as np
import pytest


class Recorder:
    """Stands in for utils.compare.PairedComparison: keeps its arguments on the host."""
    made = []

    def __init__(self, base, systems, resamples=10000, seed=0, names=None, keep_stats=True):
        self.base, self.systems = base.numpy().copy(), systems.numpy().copy()
        self.resamples, self.seed, self.names = resamples, seed, list(names)
        Recorder.made.append(self)

    def summary(self, level=0.95):
        return [{"name": n, "mean_diff": float((s - self.base).mean()), "level": level} for n, s in zip(self.names, self.systems)]

    def lines(self, level=0.95):
        return [f"{r['name']}: diff {r['mean_diff']:+.4f}" for r in self.summary(level)]


@pytest.fixture
def C(monkeypatch):
    from utils import compare
    Recorder.made = []
    monkeypatch.setattr(compare, "PairedComparison", Recorder)
    return compare


QIDS = ["q7", "q1", "q1", "q3", "q9"]                  # q1 appears at two lengths: the key is (qid, length)
LENGTHS = [300, 300, 40, 40, 300]
F1_A = [0.125, 0.25, 0.375, 0.5, 0.625]
BEST_A = [0.75, 0.5, 0.875, 0.5, 1.0]


def _write(path, order, f1, best=None, dcg=None):
    cols = {"qid": np.asarray(QIDS)[order], "length": np.asarray(LENGTHS, dtype=np.int32)[order], "f1": np.asarray(f1, dtype=np.float64)[order],
            "dcg": np.asarray(dcg if dcg is not None else f1, dtype=np.float64)[order]}
    if best is not None:
        cols["best_f1"] = np.asarray(best, dtype=np.float64)[order]
    np.savez(path, **cols)


@pytest.fixture
def reports(tmp_path):
    """Three reports over the same five (qid, length) rows, each file in another row order; values are tagged by row."""
    a, b, c = (str(tmp_path / f"{n}.npz") for n in "abc")
    _write(a, [0, 1, 2, 3, 4], F1_A, BEST_A, dcg=[-1.0, -2.0, -3.0, -4.0, -5.0])
    _write(b, [4, 2, 0, 3, 1], [v + 0.0625 for v in F1_A], BEST_A, dcg=[-1.5, -2.5, -3.5, -4.5, -5.5])
    _write(c, [1, 0, 4, 2, 3], [v - 0.0625 for v in F1_A], BEST_A)
    return a, b, c


def test_rows_are_joined_on_qid_and_length_whatever_their_order(C, reports):
    a, b, c = reports
    cmp = C.compare_reports([a, b, c], metric="f1", baseline=0, resamples=77, seed=5, device="cpu")
    assert cmp is Recorder.made[0] and (cmp.resamples, cmp.seed, cmp.names) == (77, 5, [b, c])
    assert cmp.base.dtype == np.float32 and cmp.base.tolist() == F1_A                    # the first file's row order
    assert cmp.systems.tolist() == [[v + 0.0625 for v in F1_A], [v - 0.0625 for v in F1_A]]
    # another baseline: the rows still follow the first file, the systems keep the order of the remaining files
    cmp = C.compare_reports([b, a, c], metric="f1", baseline=1, device="cpu")
    first = [4, 2, 0, 3, 1]
    assert cmp.names == [b, c] and cmp.base.tolist() == [F1_A[i] for i in first]
    assert cmp.systems.tolist() == [[F1_A[i] + 0.0625 for i in first], [F1_A[i] - 0.0625 for i in first]]
    cmp = C.compare_reports([a, b], metric="dcg", baseline=0, device="cpu")
    assert cmp.base.tolist() == [-1.0, -2.0, -3.0, -4.0, -5.0] and cmp.systems.tolist() == [[-1.5, -2.5, -3.5, -4.5, -5.5]]


@pytest.mark.parametrize("name", ["Oracle", "ORACLE", "Oracle".lower()])
def test_the_best_cut_baseline_takes_the_first_files_best_column(C, reports, name):
    a, b, c = reports
    cmp = C.compare_reports([b, a], metric="f1", baseline=name, device="cpu")
    first = [4, 2, 0, 3, 1]
    assert cmp.names == [b, a] and cmp.base.tolist() == [BEST_A[i] for i in first]      # every file is a system
    assert cmp.systems.tolist() == [[F1_A[i] + 0.0625 for i in first], [F1_A[i] for i in first]]
    assert C.is_best_cut(name) and not C.is_best_cut("0") and not C.is_best_cut(0)


def test_refusals_of_the_join(C, reports, tmp_path):
    a, b, c = reports
    with pytest.raises(ValueError, match="best_dcg"):
        C.compare_reports([a, b], metric="dcg", baseline="Oracle", device="cpu")
    dup = str(tmp_path / "dup.npz")
    np.savez(dup, qid=np.asarray(["q1", "q1"]), length=np.asarray([40, 40], dtype=np.int32), f1=np.zeros(2), dcg=np.zeros(2))
    with pytest.raises(ValueError, match="duplicate"):
        C.compare_reports([dup, dup], device="cpu")
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, qid=np.asarray(QIDS), length=np.asarray(LENGTHS, dtype=np.int32), k=np.ones(5))
    with pytest.raises(ValueError, match="label-free"):
        C.compare_reports([a, bare], device="cpu")
    assert Recorder.made == []


def test_command_line_prints_one_line_per_system_and_writes_json(C, reports, tmp_path, capsys, monkeypatch):
    import compare_reports as cli
    monkeypatch.setattr(cli, "compare_reports", lambda paths, **kw: C.compare_reports(paths, device="cpu", **kw))
    a, b, c = reports
    out = str(tmp_path / "cmp.json")
    cmp = cli.main([a, b, c, "--metric", "f1", "--resamples", "33", "--seed", "4", "--level", "0.9", "--out", out])
    assert (cmp.resamples, cmp.seed, cmp.names) == (33, 4, [b, c])
    printed = capsys.readouterr().out.strip().splitlines()
    assert printed == [f"{b}: diff +0.0625", f"{c}: diff -0.0625"]
    with open(out) as f:
        doc = json.load(f)
    assert doc["metric"] == "f1" and doc["baseline"] == "0" and doc["seed"] == 4
    assert [s["name"] for s in doc["systems"]] == [b, c] and doc["systems"][0]["level"] == 0.9
    cmp = cli.main([a, b, "--baseline", "Oracle"])
    assert cmp.names == [a, b] and cmp.base.tolist() == BEST_A and len(capsys.readouterr().out.strip().splitlines()) == 2


def test_trainer_compare_takes_each_named_report_as_a_baseline(C, reports):
    import run
    a, b, c = reports
    me = types.SimpleNamespace(args=types.SimpleNamespace(criterion="f1", seed=9), device="cpu")
    lines = run.Trainer.compare(me, b[:-4], a + "," + c)                                  # the fresh report named without .npz
    assert [(m.names, m.seed, m.resamples) for m in Recorder.made] == [([b], 9, 10000), ([b], 9, 10000)]
    assert Recorder.made[0].base.tolist() == F1_A and Recorder.made[1].base.tolist() == [F1_A[i] - 0.0625 for i in [1, 0, 4, 2, 3]]
    assert lines == [f"{b}: diff +0.0625", f"{b}: diff +0.1250"]
    args = run.build_parser().parse_args([])
    assert args.compare_to is None                                                        # off by default
