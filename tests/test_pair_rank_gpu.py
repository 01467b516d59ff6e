"""rlt_pair_rank_loss on the device, through the raw C ABI, against the float64 restatement tests/pair_rank_restate.py (never
against the library itself).

Integer outputs (rank_out, n_pairs) are exact, and rank_out equals the `rank` of rlt_rerank_lists on NaN-free scores.  Lists
without pairs give exactly 0.  loss_per_list and loss_out lie within K 2^-24 |ref| plus one fp32 rounding of ref; dscore[b,i] within
K 2^-24 A_i plus one fp32 rounding, A_i = the restatement's sum of |lam| over the pairs of i at the same scaling.

K: the worst ratio (|got - ref| - one fp32 rounding) / (2^-24 scale) over all ids of this file, measured on an MI355X, is 1.283
for the losses and 3.099 for the gradient (profiles/pair_rank_bench.log): K_MEASURED = 3.1 in tests/pair_rank_restate.py, well
under the cap of 16; the tests assert at 4x that, K_ASSERT = 12.4.
Every test prints the worst ratio it saw (pytest -s), so a re-measurement needs no other tool.

Sizes: every list length at which the dispatch changes its packing (16 / 32 / 64 lanes per list; 4, 8 or 16 documents per lane),
list counts 1, 3, 5 and one below, at and one above the lists of a wavefront and of a workgroup for each packing, and more lists
than the grid holds at once."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import pair_rank_restate as PR

pytestmark = pytest.mark.gpu

S_EDGES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1023, 1024]
GRID_CAP = 2048
F_SENT, I_SENT = 0x7fc00123, 0x7fc00123         # a NaN pattern in front of and behind every output
GUARD = 16
OUTPUTS = ("loss_per_list", "loss_out", "dscore", "rank_out", "n_pairs")
WORST = {"loss": 0.0, "grad": 0.0}


def lists_per_wave(S):
    return 4 if S <= 64 else 2 if S <= 128 else 1


def lists_per_group(S):
    return lists_per_wave(S) * (4 if S <= 512 else 2)


def list_counts(S):
    w, g = lists_per_wave(S), lists_per_group(S)
    return sorted({1, 3, 5, w - 1, w, w + 1, g - 1, g, g + 1} - {0})


@pytest.fixture(scope="module")
def lib():
    from rlt_hip import native, ops
    native.load()
    ops.dcg_table("cuda")
    return native


class Guarded:
    """n 4-byte elements between two guard stretches, everything pre-filled with a NaN pattern."""

    def __init__(self, n):
        self.n = n
        self.t = torch.full((n + 2 * GUARD,), F_SENT, dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * GUARD)

    def read(self, dtype):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == F_SENT).all() and (a[GUARD + self.n:] == F_SENT).all(), "a guard was written"
        return a[GUARD:GUARD + self.n].view(dtype)


def call(lib, score, labels, kind, sigma=1.0, gains=None, n_grades=2, normalize=True, gscale=None, want=OUTPUTS):
    """One call through the raw C ABI -> dict of what was asked for (numpy; fp32 / int32 as the device wrote them)."""
    from rlt_hip import ops
    B, S = score.shape
    s = torch.from_numpy(np.ascontiguousarray(score, dtype=np.float32)).cuda()
    y = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32)).cuda()
    sizes = {"loss_per_list": B, "loss_out": 1, "dscore": B * S, "rank_out": B * S, "n_pairs": B}
    outs = {k: Guarded(sizes[k]) for k in want}
    o = lambda k: outs[k].ptr if k in outs else None
    garr = None
    if gains is not None:
        garr, n_grades = (ctypes.c_float * len(gains))(*gains), len(gains)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device="cuda")
    L = lib.load()
    ws_bytes = L.rlt_pair_rank_workspace(B, S)
    ws = Guarded((ws_bytes + 3) // 4 + 2)
    ws_ptr = ctypes.c_void_p((ws.ptr.value + 7) & ~7)
    table = ops.dcg_table("cuda")
    rc = L.rlt_pair_rank_loss(ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(y.data_ptr()), B, S, PR.KINDS[kind], float(sigma),
                              garr, n_grades, int(normalize), ctypes.c_void_p(table.data_ptr()),
                              None if gs is None else ctypes.c_void_p(gs.data_ptr()),
                              o("loss_per_list"), o("loss_out"), o("dscore"), o("rank_out"), o("n_pairs"),
                              ws_ptr, ws_bytes, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.read(np.int32)
    res = {}
    for k, gd in outs.items():
        a = gd.read(np.int32 if k in ("rank_out", "n_pairs") else np.float32)
        res[k] = a.reshape(B, S) if k in ("dscore", "rank_out") else a
    return res


def check(res, ref, where=""):
    """Every output present against the restatement; updates and returns the worst ratios seen."""
    if "rank_out" in res:
        assert np.array_equal(res["rank_out"], ref["rank"]), where
    if "n_pairs" in res:
        assert np.array_equal(res["n_pairs"], ref["n_pairs"]), where
    worst_l = worst_g = 0.0
    unit = 2.0 ** -24
    pairs = [(res[k].astype(np.float64), np.atleast_1d(ref[r])) for k, r in (("loss_per_list", "loss_per_list"), ("loss_out", "loss"))
             if k in res]
    for got, want in pairs:
        assert np.array_equal(np.isnan(got), np.isnan(want)), where
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok]) - PR.fp32_rounding(want[ok])
        zero = want[ok] == 0
        assert (got[ok][zero] == 0).all(), where
        if (~zero).any():
            worst_l = max(worst_l, float((err[~zero] / (unit * np.abs(want[ok][~zero]))).max()))
        assert (np.abs(got[ok] - want[ok]) <= PR.loss_bound(want[ok], PR.K_ASSERT)).all(), (where, worst_l)
    if "dscore" in res:
        got, want, A = res["dscore"].astype(np.float64), ref["dscore"], ref["A"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), where
        ok = ~np.isnan(want)
        dead = ok & (A == 0)
        assert (got[dead] == 0).all(), where                   # no pair: exactly 0
        act = ok & (A > 0)
        if act.any():
            err = np.abs(got[act] - want[act]) - PR.fp32_rounding(want[act])
            worst_g = float((err / (unit * A[act])).max())
        assert (np.abs(got[ok] - want[ok]) <= PR.grad_bound(want[ok], A[ok], PR.K_ASSERT)).all(), (where, worst_g)
    WORST["loss"], WORST["grad"] = max(WORST["loss"], worst_l), max(WORST["grad"], worst_g)
    return worst_l, worst_g


def library_rank(lib, score):
    B, S = score.shape
    s = torch.from_numpy(score).cuda()
    rank = torch.empty((B, S), dtype=torch.int32, device="cuda")
    rc = lib.load().rlt_rerank_lists(ctypes.c_void_p(s.data_ptr()), B, S, None, None, 0, None, ctypes.c_void_p(rank.data_ptr()),
                                     None, None)
    assert rc == 0
    return rank.cpu().numpy()


@pytest.mark.parametrize("name", sorted(PR.CLASSES))
@pytest.mark.parametrize("S", S_EDGES)
def test_against_the_restatement(lib, S, name):
    kw = PR.class_args(name)
    wl = wg = 0.0
    for n, B in enumerate(list_counts(S)):
        kind = ("ranknet", "lambdarank")[(n + S) & 1]
        sigma = (1.0, 2.5, 0.4)[n % 3]
        normalize = bool((n >> 1) & 1) or kind == "ranknet"
        score, labels = PR.inputs(name, B, S, sigma=sigma, seed=n)
        ref = PR.restate(score, labels, kind, sigma=sigma, normalize=normalize, **kw)
        res = call(lib, score, labels, kind, sigma=sigma, normalize=normalize, **kw)
        l, g = check(res, ref, (S, name, B, kind))
        wl, wg = max(wl, l), max(wg, g)
        assert np.array_equal(res["rank_out"], library_rank(lib, score))       # zero tolerance against rlt_rerank_lists
        if name in PR.PAIRLESS or S == 1:
            assert not res["loss_per_list"].any() and not res["dscore"].any() and not res["n_pairs"].any() and res["loss_out"][0] == 0
        if n == 0:                              # two calls give the same bits
            again = call(lib, score, labels, kind, sigma=sigma, normalize=normalize, **kw)
            for k in OUTPUTS:
                assert np.array_equal(res[k].view(np.int32), again[k].view(np.int32)), k
    print(f"\npair_rank worst ratio S={S} {name}: loss {wl:.3f} grad {wg:.3f}")


@pytest.mark.parametrize("S", [40, 300])
def test_more_lists_than_the_grid_holds(lib, S):
    """The strided loop: B beyond GRID_CAP workgroups' lists, the lists a tiling of 37 distinct ones."""
    n = 37
    B = GRID_CAP * lists_per_group(S) + 2 * lists_per_group(S) + 1
    s0, y0 = PR.inputs("graded", n, S, seed=5)
    reps = -(-B // n)
    score, labels = np.tile(s0, (reps, 1))[:B], np.tile(y0, (reps, 1))[:B]
    kw = PR.class_args("graded")
    res = call(lib, score, labels, "lambdarank", sigma=1.5, **kw)
    ref = PR.restate(s0, y0, "lambdarank", sigma=1.5, batch=B, **kw)
    first = {k: res[k][:n] for k in ("loss_per_list", "dscore", "rank_out", "n_pairs")}
    check(first, ref, (S, "strided"))
    for k in ("loss_per_list", "dscore", "rank_out", "n_pairs"):
        v = res[k].view(np.int32)
        want = np.concatenate([v[:n]] * reps)[:B]
        assert np.array_equal(v, want), k                       # every later copy of a list: the same bits
    total = sum(ref["loss_per_list"][b % n] for b in range(B)) / B
    assert abs(float(res["loss_out"][0]) - total) <= PR.loss_bound(total, PR.K_ASSERT)


@pytest.mark.parametrize("S,B", [(40, 17), (65, 5), (300, 3)])
def test_every_null_output_combination(lib, S, B):
    score, labels = PR.inputs("graded", B, S, seed=2)
    kw = PR.class_args("graded")
    for kind in ("ranknet", "lambdarank"):
        full = call(lib, score, labels, kind, sigma=1.3, **kw)
        check(full, PR.restate(score, labels, kind, sigma=1.3, **kw), (S, B, kind))
        for mask in itertools.product((False, True), repeat=len(OUTPUTS)):
            want = tuple(k for k, m in zip(OUTPUTS, mask) if m)
            if not want:
                continue
            part = call(lib, score, labels, kind, sigma=1.3, want=want, **kw)
            assert set(part) == set(want)
            for k in want:
                assert np.array_equal(part[k].view(np.int32), full[k].view(np.int32)), (kind, want, k)


@pytest.mark.parametrize("S,B", [(40, 9), (100, 5), (300, 6), (600, 3)])
def test_lists_are_independent_and_nan_scores_stay_in_their_list(lib, S, B):
    for kind, name in (("lambdarank", "graded"), ("ranknet", "randn")):
        kw = PR.class_args(name)
        score, labels = PR.inputs(name, B, S, seed=8)
        base = call(lib, score, labels, kind, **kw)
        moved = score.copy()
        moved[0] = moved[0, ::-1] * np.float32(1.5)
        other = call(lib, moved, labels, kind, **kw)
        for k in ("loss_per_list", "dscore", "rank_out", "n_pairs"):
            assert np.array_equal(base[k][1:].view(np.int32), other[k][1:].view(np.int32)), k
        assert not np.array_equal(base["dscore"][0], other["dscore"][0])
        bad = score.copy()
        victim = B // 2
        bad[victim, S // 3] = np.nan
        res = call(lib, bad, labels, kind, **kw)
        ref = PR.restate(bad, labels, kind, **kw)
        check(res, ref, (S, B, kind, "nan"))
        assert np.isnan(res["loss_per_list"][victim]) and np.isnan(res["dscore"][victim]).all() and np.isnan(res["loss_out"][0])
        assert res["n_pairs"][victim] == base["n_pairs"][victim]
        keep = np.arange(B) != victim
        for k in ("loss_per_list", "dscore", "rank_out", "n_pairs"):
            assert np.array_equal(base[k][keep].view(np.int32), res[k][keep].view(np.int32)), k


@pytest.mark.parametrize("S,B", [(40, 5), (300, 3)])
def test_gscale_scales_the_gradient_and_nothing_else(lib, S, B):
    score, labels = PR.inputs("graded", B, S, seed=4)
    kw = PR.class_args("graded")
    for kind in ("ranknet", "lambdarank"):
        one = call(lib, score, labels, kind, sigma=0.8, **kw)
        for gscale in (1.0, -3.5, 0.0):
            res = call(lib, score, labels, kind, sigma=0.8, gscale=gscale, **kw)
            for k in ("loss_per_list", "loss_out", "rank_out", "n_pairs"):
                assert np.array_equal(res[k].view(np.int32), one[k].view(np.int32)), k
            if gscale == 1.0:
                assert np.array_equal(res["dscore"].view(np.int32), one["dscore"].view(np.int32))
            elif gscale == 0.0:
                assert not res["dscore"].any()
            else:
                check(res, PR.restate(score, labels, kind, sigma=0.8, gscale=gscale, **kw), (S, B, kind, gscale))


def test_python_ops_match_the_raw_call(lib):
    from rlt_hip import ops
    B, S = 5, 40
    score, labels = PR.inputs("graded", B, S, seed=6)
    s, y = torch.from_numpy(score).cuda(), torch.from_numpy(labels).cuda()
    raw = call(lib, score, labels, "lambdarank", sigma=2.0, gains=list(PR.CUSTOM_GAINS))
    rank, n_pairs, per_list = ops.pair_rank(s, y, kind="lambdarank", sigma=2.0, gains=PR.CUSTOM_GAINS)
    assert np.array_equal(rank.cpu().numpy(), raw["rank_out"]) and np.array_equal(n_pairs.cpu().numpy(), raw["n_pairs"])
    assert np.array_equal(per_list.cpu().numpy().view(np.int32), raw["loss_per_list"].view(np.int32))
    leaf = s.clone().unsqueeze(2).requires_grad_(True)
    loss = ops.PairRankLossFn.apply(leaf, y, "lambdarank", 2.0, PR.CUSTOM_GAINS, 8, True)
    (loss * 0.25).backward()
    assert loss.detach().cpu().numpy().view(np.int32) == raw["loss_out"].view(np.int32)[0]
    assert leaf.grad.shape == leaf.shape
    scaled = call(lib, score, labels, "lambdarank", sigma=2.0, gains=list(PR.CUSTOM_GAINS), gscale=0.25)
    ref = PR.restate(score, labels, "lambdarank", sigma=2.0, gains=list(PR.CUSTOM_GAINS), gscale=0.25)
    check({"dscore": leaf.grad.reshape(B, S).cpu().numpy()}, ref, "tape")
    check(scaled, ref, "gscale")


def test_zz_report_the_worst_ratio():
    print(f"\npair_rank worst ratio over this run: loss {WORST['loss']:.3f} grad {WORST['grad']:.3f} "
          f"(K_MEASURED {PR.K_MEASURED}, asserted at {PR.K_ASSERT})")
    assert max(WORST.values()) <= PR.K_ASSERT
