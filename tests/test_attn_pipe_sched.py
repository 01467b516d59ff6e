"""The scheduler that the generators of the pipelined attention tile bodies share (tools/attn_pipe_sched.py), on problems small
enough to place by hand: the cyclic earliest-deadline-first placement, the capacity relaxation, the `no schedule:` exit, and the
independent verifier - which must reject a schedule that breaks any one of its rules.  CPU only."""
import importlib
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import attn_pipe_sched as S  # noqa: E402

COST = {"mul": 4, "exp": 8}


def small():
    """Eight gaps of 8 cycles.  By deadline: b takes gap 0; c (an exp, 8 cycles) does not fit beside it and takes gap 1; a waits for
    its release, gap 4; e1 and e2 fill gap 7, e3 wraps round to gap 8 = gap 0 beside b; d (no deadline: last) sits LAG = 2 behind c."""
    sch = S.Schedule(8, 4, COST)
    t = {"a": sch.add("a", [("a();", "mul")], 4, 5),
         "b": sch.add("b", [("b();", "mul")], 0, 2),
         "c": sch.add("c", [("c();", "exp")], 0, 3)}
    t["d"] = sch.add("d", [("d();", "exp")], 0, None, [(t["c"], 2)])
    for j in (1, 2, 3):
        t[f"e{j}"] = sch.add(f"e{j}", [(f"e({j});", "mul")], 7, 9)
    sch.solve()
    return sch, t


def test_edf_placement_on_a_cyclic_timeline():
    sch, t = small()
    assert {n: x.placed for n, x in t.items()} == {"a": [4], "b": [0], "c": [1], "d": [3], "e1": [7], "e2": [7], "e3": [8]}
    assert sch.capv == [8] * 8 and sch.used == [8, 8, 0, 8, 4, 0, 0, 8]
    assert [c for c, _k, _n, _g in sch.gaps[0]] == ["b();", "e(3);"]
    sch.verify()


def test_relaxation_raises_capacity_only_around_the_miss():
    """Three 4-cycle chunks that must all sit in gap 3: the third misses at capacity 8; every attempt adds a cycle to the gaps from six
    ahead of its window to its deadline (9, 10, 11, 0 .. 3 of the 12), until 12 cycles fit."""
    sch = S.Schedule(12, 4, COST)
    ts = [sch.add(f"m{j}", [(f"m({j});", "mul")], 3, 3) for j in range(3)]
    assert sch.run() is ts[2]
    sch.solve()
    assert [t.placed for t in ts] == [[3], [3], [3]]
    assert sch.capv == [12, 12, 12, 12, 8, 8, 8, 8, 8, 12, 12, 12]
    sch.verify()


def test_infeasible_problem_ends_with_no_schedule():
    sch = S.Schedule(8, 4, COST)
    sch.add("x", [("x();", "mul")], 5, 2)
    with pytest.raises(SystemExit) as e:
        sch.solve()
    assert str(e.value.code).startswith("no schedule: x (release 5, deadline 2)")


def _break_release(sch, t):
    t["a"].placed = [3]


def _break_lag(sch, t):
    t["d"].placed = [2]


def _break_deadline(sch, t):
    t["b"].placed = [4]


def _break_capacity(sch, t):
    t["e3"].placed = [7]


def _break_one_exp(sch, t):
    sch.capv = [16] * 8
    t["d"].placed = [9]          # gap 1 of the next round: beside c, within 16 cycles, but two exp


@pytest.mark.parametrize("breaker,what", [(_break_release, "before its release"), (_break_lag, "behind c"), (_break_deadline, "behind its deadline"),
                                          (_break_capacity, "gap 7: 12 cycles of 8"), (_break_one_exp, "gap 1: 2 exp chunks")],
                         ids=["release", "after_lag", "deadline", "capacity", "one_exp"])
def test_verifier_rejects_each_broken_rule(breaker, what):
    sch, t = small()
    breaker(sch, t)
    with pytest.raises(S.ScheduleError, match=what):
        sch.verify()


@pytest.mark.parametrize("name", ["gen_attn6n_body", "gen_attn6h_body"])
def test_importing_a_generator_runs_nothing(name, capsys):
    sys.modules.pop(name, None)
    mod = importlib.import_module(name)
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
    assert callable(mod.main) and callable(mod.schedule)
    assert not any(isinstance(v, (S.Schedule, S.Layout, S.Task)) for v in vars(mod).values())


@pytest.mark.parametrize("args", [["gen_attn6n_body.py", "fwd", "bogus"], ["gen_attn6h_body.py", "fwd", "bogus"], ["gen_attn6n_body.py", "fwd", "drop"],
                                  ["gen_attn6h_body.py", "dq", "drop"], ["gen_attn6n_body.py", "bogus"], ["gen_attn6h_body.py", "fwd", "drop", "drop"]],
                         ids=lambda a: "_".join(a))
def test_unknown_arguments_are_an_error(args):
    res = subprocess.run([sys.executable, os.path.join(TOOLS, args[0])] + args[1:], capture_output=True, text=True)
    assert res.returncode != 0 and res.stdout == ""
    assert res.stderr.startswith("usage: ") and res.stderr.count("\n") == 1
