"""The paired comparison pass on the device (csrc/compare.hip) through the raw C ABI, against the float64 restatement of
tests/compare_restate.py (pinned to enumeration, draw statistics and scipy in tests/test_compare_restate.py).

Qmax (largest resident Q for this M) and C (queries per chunk) are read from the plan, and the form a case names is asserted on it.
The kernels have no grid-stride trip (one wavefront per replicate and chunk), so there is no size that forces a second one.

Tolerances.  Exact operands (integers in [-512, 512] times 2^-10, every system's mean difference a multiple of 2^-10 -
compare_restate.exact_operands): every sum, the squared deviations included, is exact in float64 in any order, so the record word
for word, every replicate statistic and the three counts must EQUAL the restatement's.  Random float32 operands: a float64 sum of Q
terms is within Q * 2^-53 * sum |d| of the exact sum in any order; rand_stat and boot_stat are held to that against the
restatement; the counts are not compared there (a replicate inside that band of |T_obs| may fall on either side).
The feature has no precision mode: nothing here depends on RLT_PRECISION."""
import os

import numpy as np
import pytest
import torch

import compare_restate as R
import report_restate

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN_BITS = 0x7FF8DEADBEEF0001          # a quiet NaN: the sentinel of every pre-filled buffer
GUARD = 8                              # 8-byte words past the end of each output


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def _sentinel(n_words):
    return torch.full((n_words,), NAN_BITS, dtype=torch.int64, device="cuda")


def _run(N, base, sys, Rn, seed, ld=None, keep=True):
    """One rlt_paired_compare call on pre-filled buffers -> dict(record (M,16) int64, rand, boot (M,R) float64 or None, plan);
    asserts that nothing past the record, past M * R statistics or past the workspace was written."""
    sys = np.atleast_2d(sys)
    M, Q = sys.shape
    ld = Q if ld is None else ld
    sys_pad = np.full((M, ld), np.nan, dtype=np.float32)          # a read of the padding would show as a non-finite pair
    sys_pad[:, :Q] = sys
    b, s = torch.from_numpy(np.ascontiguousarray(base, dtype=np.float32)).cuda(), torch.from_numpy(sys_pad).cuda()
    plan = N.paired_compare_plan(Q, M, Rn)
    ws_bytes = N.query("rlt_paired_compare_workspace", Q, M, Rn)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    ws = _sentinel(ws_bytes // 8 + GUARD)
    rec = _sentinel(M * N.CMP_WORDS + GUARD)
    rs, bs = (_sentinel(M * Rn + GUARD), _sentinel(M * Rn + GUARD)) if keep else (None, None)
    N.call("rlt_paired_compare", N.ptr(b), N.ptr(s), ld, Q, M, Rn, seed, N.ptr(ws), ws_bytes, N.ptr(rec), N.ptr(rs), N.ptr(bs), N.stream())
    torch.cuda.synchronize()
    for t, used in ((ws, ws_bytes // 8), (rec, M * N.CMP_WORDS)) + (((rs, M * Rn), (bs, M * Rn)) if keep else ()):
        assert (t[used:].cpu().numpy() == NAN_BITS).all(), "written past the end"
    out = {"record": rec[:M * N.CMP_WORDS].cpu().numpy().reshape(M, N.CMP_WORDS).copy(), "plan": plan, "rand": None, "boot": None}
    if keep:
        out["rand"] = rs[:M * Rn].cpu().numpy().view(np.float64).reshape(M, Rn).copy()
        out["boot"] = bs[:M * Rn].cpu().numpy().view(np.float64).reshape(M, Rn).copy()
    return out


def _form_code(N, plan):
    return N.CMP_FORMS.index(plan["form"])


def _check_record(N, got, want, ssd_rel=0.0, counts=True):
    """The record word for word (float64 words by value and sign; ssd within ssd_rel when that is not 0)."""
    skip = () if counts else (R.RAND_GE, R.BOOT_LE0, R.BOOT_GE0)
    for m, rec in enumerate(want):
        row = got["record"][m]
        f = row.view(np.float64)
        for word in range(N.CMP_WORDS):
            if word in skip:
                continue
            if word == R.FORM:
                assert row[word] == _form_code(N, got["plan"]), (m, word)
            elif word == R.SSD and ssd_rel:
                assert abs(f[word] - rec[word]) <= ssd_rel * rec[word], (m, f[word], rec[word])
            elif word in R.F64_WORDS:
                assert f[word] == rec[word], (m, word, f[word], rec[word])
            else:
                assert row[word] == rec[word], (m, word, row[word], rec[word])


def _check_exact(N, base, sys, Rn, seed, form, ld=None, **kw):
    got = _run(N, base, sys, Rn, seed, ld=ld)
    assert got["plan"]["form"] == form
    want, rand, boot = R.compare(base, sys, Rn, seed)
    _check_record(N, got, want, **kw)
    assert np.array_equal(got["rand"], rand) and np.array_equal(got["boot"], boot)
    return got, want


# ---------------------------------------------------------------------------------------------------------------- resident form
@pytest.mark.parametrize("Q", [1, 31, 32, 33, 63, 64, 65, 300])
def test_resident_exact_operands(N, Q):
    for M in (1, 3, 8):
        base, sys = R.exact_operands(Q, M, 1000 * M + Q)
        for Rn in (0, 1, 63, 64, 65, 257):
            _check_exact(N, base, sys, Rn, seed=77 + Rn, form="resident", ld=Q + 5 if Rn % 2 else None)


def test_resident_without_the_statistic_arrays(N):
    base, sys = R.exact_operands(300, 3, 5)
    got = _run(N, base, sys, 257, 9, keep=False)
    want, _, _ = R.compare(base, sys, 257, 9)
    _check_record(N, got, want)


def test_resident_limit_and_many_replicates_per_wavefront(N):
    """Q = Qmax (all 160 KB of LDS) at M = 8, and R large enough for 16 replicates per wavefront at a small Q."""
    qmax = N.paired_compare_plan(1, 8, 1)["resident_max_q"]
    base, sys = R.exact_operands(qmax, 8, 3)
    got, _ = _check_exact(N, base, sys, 33, seed=5, form="resident")
    assert got["plan"]["lds_bytes"] == 160 * 1024
    base, sys = R.exact_operands(33, 2, 4)
    Rn = 16 * 16 * 1024 + 3
    assert N.paired_compare_plan(33, 2, Rn)["replicates_per_wave"] == 16
    _check_exact(N, base, sys, Rn, seed=6, form="resident")


# ---------------------------------------------------------------------------------------------------------------- chunked form
@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("size", ["Qmax+1", "C-1", "C", "C+1", "2C+5"])
def test_chunked_exact_operands(N, size, M):
    p = N.paired_compare_plan(1, M, 1)
    qmax, C = p["resident_max_q"], p["chunk"]
    Q = {"Qmax+1": qmax + 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+5": 2 * C + 5}[size]
    base, sys = R.exact_operands(Q, M, Q + M)
    for Rn in (1, 65):
        got, _ = _check_exact(N, base, sys, Rn, seed=31 + Rn, form="chunked", ld=Q + 3 if Rn == 65 else None)
        assert got["plan"]["chunks"] == (Q + C - 1) // C


# ---------------------------------------------------------------------------------------------------------------- further cases
@pytest.mark.parametrize("form", ["resident", "chunked"])
def test_query_tagged_operands(N, form):
    """d[q] = (q + 1) * 2^-15, distinct per query: a wrong sign position or gather index cannot cancel."""
    Q = 300 if form == "resident" else N.paired_compare_plan(1, 1, 1)["resident_max_q"] + 1
    base = np.zeros(Q, dtype=np.float32)
    sys = ((np.arange(Q) + 1) / 32768.0).astype(np.float32)[None, :]
    got = _run(N, base, sys, 65, 12)
    assert got["plan"]["form"] == form
    want, rand, boot = R.compare(base, sys, 65, 12)
    _check_record(N, got, want, ssd_rel=Q * U + 1e-15)
    assert np.array_equal(got["rand"], rand) and np.array_equal(got["boot"], boot)
    # the replicates are not one value repeated; two of 65 may coincide (the sums are multiples of 2^-15 with a spread of a few
    # thousand of them, so a pair meets with a probability of some tenths), more than half of them cannot
    assert len(set(rand[0].tolist())) > 32 and len(set(boot[0].tolist())) > 32


def test_ties(N):
    Q, Rn = 3, 257
    zero = np.zeros(Q, dtype=np.float32)
    got, want = _check_exact(N, zero, zero[None, :], Rn, seed=3, form="resident")
    assert got["record"][0][R.RAND_GE] == Rn and got["record"][0][R.TIES] == Q and got["record"][0][R.WINS] == 0
    assert got["record"][0][R.BOOT_LE0] == Rn and got["record"][0][R.BOOT_GE0] == Rn
    got, want = _check_exact(N, zero, np.full((1, Q), 0.25, dtype=np.float32), Rn, seed=3, form="resident")
    s = R.signs(3, np.arange(Rn), Q)
    all_equal = int((np.abs(s.sum(axis=1)) == Q).sum())
    assert 20 < all_equal < 120                                   # about R / 4 of the replicates at Q = 3
    assert got["record"][0][R.WINS] == Q and got["record"][0][R.RAND_GE] == all_equal


@pytest.mark.parametrize("form", ["resident", "chunked"])
def test_non_finite_inputs_are_counted(N, form):
    Q = 300 if form == "resident" else N.paired_compare_plan(1, 2, 1)["resident_max_q"] + 7
    base, sys = R.exact_operands(Q, 2, 8)
    base[5] = np.nan
    sys[0, 17] = np.inf
    sys[1, Q - 1] = -np.inf
    sys[1, 5] = np.nan
    got = _run(N, base, sys, 65, 4)
    assert got["plan"]["form"] == form
    want, rand, boot = R.compare(base, sys, 65, 4)
    assert [int(got["record"][m][R.NONFINITE]) for m in range(2)] == [2, 2]
    _check_record(N, got, want, ssd_rel=Q * U + 1e-15)
    assert np.array_equal(got["rand"], rand) and np.array_equal(got["boot"], boot) and np.isfinite(got["rand"]).all()


@pytest.mark.parametrize("form", ["resident", "chunked"])
def test_random_float32_operands_and_two_calls(N, form):
    M = 3
    p = N.paired_compare_plan(1, M, 1)
    Q = 300 if form == "resident" else 2 * p["chunk"] + 5
    rng = np.random.RandomState(21)
    base = rng.rand(Q).astype(np.float32)
    sys = (base[None, :] + 0.3 * rng.randn(M, Q)).astype(np.float32)
    Rn = 257 if form == "resident" else 33
    got = _run(N, base, sys, Rn, 99)
    assert got["plan"]["form"] == form
    want, rand, boot = R.compare(base, sys, Rn, 99)
    d, _ = R.differences(base, sys)
    for m in range(M):
        bound = Q * U * np.abs(d[m]).sum()
        err_r, err_b = np.abs(got["rand"][m] - rand[m]).max(), np.abs(got["boot"][m] - boot[m]).max()
        print(f"{form} m={m}: bound {bound:.3e} rand {err_r:.3e} boot {err_b:.3e}")
        assert err_r <= bound and err_b <= bound
        f = got["record"][m].view(np.float64)
        assert abs(f[R.T_OBS] - want[m][R.T_OBS]) <= bound and abs(f[R.SUM_D] - want[m][R.SUM_D]) <= bound
        assert abs(f[R.SSD] - want[m][R.SSD]) <= 4 * Q * U * want[m][R.SSD]
        assert [got["record"][m][w] for w in (R.N_, R.WINS, R.TIES, R.LOSSES, R.NONFINITE)] == \
               [want[m][w] for w in (R.N_, R.WINS, R.TIES, R.LOSSES, R.NONFINITE)]
    again = _run(N, base, sys, Rn, 99)
    for k in ("record", "rand", "boot"):
        assert got[k].tobytes() == again[k].tobytes(), k
    other = _run(N, base, sys, Rn, 100)
    assert not np.array_equal(other["rand"], got["rand"])          # the seed matters


def test_ops_and_paired_comparison_on_the_golden_report(N):
    """F1 columns of the 96 robust04 lists: the model's cut as the baseline; the Oracle cut, Fixed-5 and Fixed-30 as systems."""
    from rlt_hip import ops
    from utils.compare import PairedComparison
    z = np.load(os.path.join(GOLDEN, "report_robust04_s300.npz"))
    f1 = report_restate.reward(z["labels"], "f1")
    k = report_restate.cut_argmax(z["output"])
    base = f1[np.arange(96), k - 1].astype(np.float32)
    sys = np.stack([f1.max(axis=1), f1[:, 4], f1[:, 29]]).astype(np.float32)
    Rn, seed = 2000, 11
    want, rand, boot = R.compare(base, sys, Rn, seed)
    out = ops.paired_compare(torch.from_numpy(base).cuda(), torch.from_numpy(sys).cuda(), Rn, seed)
    assert out["record"].shape == (3, N.CMP_WORDS) and out["rand_stat"].shape == (3, Rn) and out["record"].is_cuda
    d, _ = R.differences(base, sys)
    bound = max(96 * U * np.abs(d[m]).sum() for m in range(3))
    assert np.abs(out["rand_stat"].cpu().numpy() - rand).max() <= bound and np.abs(out["boot_stat"].cpu().numpy() - boot).max() <= bound
    cmp = PairedComparison(torch.from_numpy(base).cuda(), torch.from_numpy(sys).cuda(), resamples=Rn, seed=seed,
                           names=["Oracle", "Fixed-5", "Fixed-30"])
    p_want = [R.randomization_p(want[m][R.RAND_GE], Rn) for m in range(3)]
    holm_want = R.holm(p_want)
    assert cmp.holm_p() == pytest.approx(holm_want, abs=0) and np.argsort(cmp.holm_p()).tolist() == np.argsort(holm_want).tolist()
    for m in range(3):
        assert cmp.randomization_p(m) == p_want[m]
        lo, hi = cmp.bootstrap_interval(m, 0.95)
        wlo, whi = R.percentile_interval(boot[m], 96, 0.95)
        assert abs(lo - wlo) <= bound / 96 and abs(hi - whi) <= bound / 96 and lo <= cmp.means(m)[2] <= hi
        assert cmp.sign_test(m) == pytest.approx(R.sign_test_p(want[m][R.WINS], want[m][R.LOSSES]), rel=1e-12)
        t, df = cmp.t_test(m)
        wt, wdf = R.t_statistic(d[m])
        assert df == wdf == 95 and t == pytest.approx(wt, rel=1e-12)
    assert cmp.means(0)[2] > 0 and cmp.randomization_p(0) == 1 / (Rn + 1)          # the Oracle cut beats every model on every list
    assert len(cmp.lines()) == 3 and cmp.summary()[0]["form"] == "resident"
    bad = torch.from_numpy(base).cuda().clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError, match="NaN or Inf"):
        PairedComparison(bad, torch.from_numpy(sys).cuda(), resamples=10, seed=1).means(0)
