"""rlt_reward_eval on the device (raw C ABI through ctypes) at the edges of its layouts: S over the four / two / one-list forms,
S % 4 != 0 and the rounds of 64; B over partial wavefronts and workgroups; T over no cut, one lane, a full row of lanes; both
reward sources; F_beta, gain with own discounts, nDCG; allow_empty 0 and 1.

What is compared with what.  The reward row is compared BIT FOR BIT with rlt_reward_spec_matrix's r_out.  Integer outputs (best,
best_k, better, best_hist, counts) are compared with zero tolerance against tests/reward_eval_restate.py applied to THAT device
r_out, so no fp32-ulp tie can excuse a mismatch.  The float64 sums are bounded by (B - 1) * 2^-53 * sum |r|, the bound of any
summation order.  With exact operands (integer gains, power-of-two discounts) every output equals the float64 restatement."""
import os

import numpy as np
import pytest
import torch

import reward_any_restate as R
import reward_eval_restate as E

pytestmark = pytest.mark.gpu

S_EDGES = [1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 300, 301, 1023, 1024]
B_EDGES = [1, 2, 3, 5, 255, 256, 257]
T_EDGES = [0, 1, 2, 63, 64]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTPUTS = ("r_at", "better", "best", "best_k", "curve", "best_hist", "sums")


@pytest.fixture(scope="module")
def lib():
    from rlt_hip import native
    native.load()
    return native


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _guarded(n, dtype, pad=16, fill=None):
    sentinel = float("nan") if dtype.is_floating_point else -7
    t = torch.full((n + pad,), sentinel, dtype=dtype, device="cuda")
    if fill is not None:
        t[:n] = torch.as_tensor(fill, dtype=dtype, device="cuda").reshape(-1)
    return t


def _intact(t, n):
    tail = t[n:]
    return bool(torch.isnan(tail).all()) if t.dtype.is_floating_point else bool((tail == -7).all())


def _ulps(a, b):
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _pairs(S):
    """(the library's RewardSpec, the restatement's Spec): F_beta, gain with own discounts, nDCG."""
    from utils.rewards import RewardSpec
    disc = (1.0 / (1.0 + np.arange(S))).astype(np.float32)
    return [(RewardSpec.fbeta(2.0), R.fbeta(2.0)), (RewardSpec.gain((-1.0, 1.0, 3.0), discount=disc), R.gain((-1.0, 1.0, 3.0), disc)),
            (RewardSpec.ndcg(), R.ndcg()), (RewardSpec.fbeta(1.0), R.fbeta(1.0))]


def _labels(B, S, seed, grades=3):
    rng = np.random.default_rng(seed)
    y = ((rng.random((B, S)) < 0.35) * rng.integers(1, grades, (B, S))).astype(np.float32)
    if B > 1:
        y[1] = 0.0                                  # no relevant document: F_beta 0 everywhere, ideal 0, negative gain rows
    if B > 2:
        y[2] = grades - 1
    return y


def _cuts(B, S, T, seed):
    """(B,T) int32 in -1..S+1: the ends clamp; column 0 holds the out-of-range ones in its first rows."""
    k = np.random.default_rng(seed).integers(-1, S + 2, (B, max(T, 1))).astype(np.int32)[:, :T]
    if T:
        k[0, 0] = -1
        if B * T > 1:
            k[-1, -1] = S + 1
    return k


def _sum_bound(x):
    """The bound of any summation order on the MEAN of the columns of x: (n - 1) * 2^-53 * sum |x| / n."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return (len(x) - 1) * 2.0 ** -53 * x.sum(0) / len(x)


def spec_matrix(y, spec):
    from rlt_hip import ops
    out = ops.reward_spec_matrix(_dev(y), spec, 1.0, False)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_eval(lib, S, labels=None, spec=None, r=None, k=None, allow_empty=1, want=OUTPUTS, accumulate=0, init=None):
    """One call of rlt_reward_eval on guarded outputs -> dict of numpy results (None where the output was NULL) and `intact`:
    every sentinel behind every output is untouched.  init: {name: array} the split outputs start from (accumulate)."""
    from rlt_hip import ops
    N = lib
    rows = labels if labels is not None else r
    B = rows.shape[0]
    T = 0 if k is None else k.shape[1]
    rt = _dev(rows)
    kt = None if not T else _dev(k, torch.int32)
    struct = keep = table = None
    if spec is not None:
        struct, keep = spec.native(S, rt.device)
        table = ops.dcg_table(rt.device) if struct.family == N.REWARD_GAIN and struct.discount is None else None
    sizes = {"r_at": (B * T, torch.float32), "better": (B * T, torch.int32), "best": (B, torch.float32), "best_k": (B, torch.int32),
             "curve": (S + 1, torch.float64), "best_hist": (S + 1, torch.float64), "sums": (3 + 3 * T, torch.float64)}
    bufs = {n: (_guarded(*sizes[n], fill=None if init is None else init.get(n)) if n in want and sizes[n][0] else None) for n in OUTPUTS}
    ws_bytes = N.query("rlt_reward_eval_workspace", B, S, T)
    ws = N.workspace(ws_bytes, rt.device)
    g = lambda n: N.ptr(bufs[n])
    N.call("rlt_reward_eval", N.ptr(rt) if labels is not None else None, None if struct is None else N.ctypes.byref(struct),
           N.ptr(rt) if labels is None else None, B, S, N.ptr(kt), T, int(allow_empty), N.ptr(table), int(accumulate),
           g("r_at"), g("better"), g("best"), g("best_k"), g("curve"), g("best_hist"), g("sums"), N.ptr(ws), ws_bytes, N.stream())
    torch.cuda.synchronize()
    out = {"intact": all(_intact(t, sizes[n][0]) for n, t in bufs.items() if t is not None)}
    for n, t in bufs.items():
        out[n] = None if t is None else t[:sizes[n][0]].cpu().numpy()
    for n in ("r_at", "better"):
        if out[n] is not None:
            out[n] = out[n].reshape(B, T)
    return out


def check_against(got, ref, r_dev, B, S, T, tag):
    """Zero tolerance on the integer outputs and on the reward values, the float64 sums within the bound of any order."""
    assert got["intact"], tag
    assert np.array_equal(_bits(got["best"]), _bits(ref["best"])), tag
    assert np.array_equal(got["best_k"], ref["best_k"]), tag
    assert np.array_equal(got["best_hist"], ref["best_hist"]), tag
    assert got["sums"][0] == B, tag
    absr = np.abs(r_dev.astype(np.float64))
    eps = (B - 1) * 2.0 ** -53
    assert np.all(np.abs(got["curve"] - ref["curve"]) <= eps * np.concatenate([[0.0], absr.sum(0)])), tag
    assert got["curve"][0] == 0.0, tag
    assert abs(got["sums"][1] - ref["sums"][1]) <= eps * np.abs(ref["best"].astype(np.float64)).sum(), tag
    if T:
        assert np.array_equal(_bits(got["r_at"]), _bits(ref["r_at"])), tag
        assert np.array_equal(got["better"], ref["better"]), tag
        assert got["sums"][2] == ref["sums"][2], tag
        assert np.array_equal(got["sums"][4::3], ref["sums"][4::3]) and np.array_equal(got["sums"][5::3], ref["sums"][5::3]), tag
        assert np.all(np.abs(got["sums"][3::3] - ref["sums"][3::3]) <= eps * np.abs(ref["r_at"].astype(np.float64)).sum(0)), tag


# ---- checks 1, 2, 4, 5, 8 (guards), 9: the grid of shapes, sources, specs ------------------------------------------------------
@pytest.mark.parametrize("S", S_EDGES)
def test_shapes_sources_and_specs(lib, S):
    pairs = _pairs(S)[:3]
    cache = {}
    n = S_EDGES.index(S)                            # the rotation starts elsewhere at every S
    for B in B_EDGES:
        y = _labels(B, S, 7 * S + B)
        for T in T_EDGES:
            # every (B, T) at every S; the spec, allow_empty and the source rotate so that each combination meets each edge
            i = n % 3
            allow_empty = (n // 3) % 2
            source = "matrix" if (n // 6) % 2 else "spec"
            n += 1
            spec, want = pairs[i]
            if (B, i) not in cache:
                r_dev = spec_matrix(y, spec)
                assert _ulps(r_dev, R.reward(y, want)).max() <= 1                    # check 5: one fp32 ulp from float64
                cache[(B, i)] = r_dev
            r_dev = cache[(B, i)]
            k = _cuts(B, S, T, S + B + T) if T else None
            kw = dict(labels=y, spec=spec) if source == "spec" else dict(r=r_dev)
            got = run_eval(lib, S, k=k, allow_empty=allow_empty, want=OUTPUTS if T else OUTPUTS[2:], **kw)
            ref = E.evaluate(r_dev, k, bool(allow_empty))
            check_against(got, ref, r_dev, B, S, T, (S, B, T, i, allow_empty, source))
            if T:                                                                    # check 9: the clamped ends
                assert got["r_at"][0, 0] == 0.0 and not np.signbit(got["r_at"][0, 0])
                assert B * T == 1 or _bits(got["r_at"][-1, -1]) == _bits(r_dev[-1, S - 1])
                assert got["sums"][2] >= min(2, B * T)
            ref64 = E.evaluate(R.reward(y, want), k, bool(allow_empty))              # check 5: values against float64
            assert _ulps(got["best"], ref64["best"]).max() <= 1
            if T:
                assert _ulps(got["r_at"], ref64["r_at"]).max() <= 1


# ---- check 1: the whole row through r_at, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_EDGES)
def test_reward_row_is_bit_identical_to_the_training_entry_point(lib, S):
    B = 5
    y = _labels(B, S, 3 * S)
    for i, (spec, _want) in enumerate(_pairs(S)[:3]):
        r_dev = spec_matrix(y, spec)
        for source in ("spec", "matrix"):
            kw = dict(labels=y, spec=spec) if source == "spec" else dict(r=r_dev)
            row = np.empty((B, S + 1), dtype=np.float32)
            for lo in range(0, S + 1, 64):
                cuts = np.arange(lo, min(lo + 64, S + 1), dtype=np.int32)
                got = run_eval(lib, S, k=np.tile(cuts, (B, 1)), want=("r_at",), **kw)
                assert got["intact"]
                row[:, cuts] = got["r_at"]
            assert np.array_equal(_bits(row[:, 1:]), _bits(r_dev)), (S, i, source)
            assert np.all(row[:, 0] == 0.0) and not np.signbit(row[:, 0]).any()     # cut 0: +0.0


# ---- checks 3 and 7: exact operands ------------------------------------------------------------------------------------------------
def _exact_case(B, S, seed):
    """Integer gains, power-of-two discounts, 3 grades (as tests/test_reward_any_gpu.py): every sum is exact in float64 and in
    fp32.  Gain 0 for grade 1 makes runs of equal rewards: rows tie at their maximum."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, (B, S)).astype(np.float32)
    lead = min(S, 2)
    y[0, :lead] = 2.0
    y[0, lead:] = 0.0
    y[0, lead:lead + max(1, S // 3)] = 1.0
    if B > 1:
        y[1] = 1.0                                  # all rewards 0: k = 0 wins with allow_empty, k = 1 without
    if B > 2:
        y[2] = 0.0                                  # all-negative row
    disc = (2.0 ** -(np.arange(S) % 7)).astype(np.float32)
    return y, disc


@pytest.mark.parametrize("S", S_EDGES)
def test_exact_operands_equal_the_float64_restatement(lib, S):
    from utils.rewards import RewardSpec
    for n, B in enumerate(B_EDGES):
        T = T_EDGES[1 + n % 4]
        y, disc = _exact_case(B, S, 100 * S + B)
        spec, want = RewardSpec.gain((-1.0, 0.0, 2.0), discount=disc), R.gain((-1.0, 0.0, 2.0), disc)
        r64 = R.reward64(y, want)
        assert np.array_equal(r64, r64.astype(np.float32).astype(np.float64))      # exact operands indeed
        k = _cuts(B, S, T, B + S)
        for allow_empty in (0, 1):
            ref = E.evaluate(r64, k, bool(allow_empty))
            got = run_eval(lib, S, labels=y, spec=spec, k=k, allow_empty=allow_empty)
            assert got["intact"]
            for name in OUTPUTS:
                assert np.array_equal(np.asarray(got[name], dtype=np.float64), np.asarray(ref[name], dtype=np.float64)), (S, B, T, name)
            if B > 2:
                assert got["best_k"][1] == (0 if allow_empty else 1) and got["best_k"][2] == (0 if allow_empty else 1)
            again = run_eval(lib, S, labels=y, spec=spec, k=k, allow_empty=allow_empty)             # two calls: the same bits
            for name in OUTPUTS:
                assert got[name].tobytes() == again[name].tobytes(), (S, B, T, name)
        # accumulate: two batches added = the sum of two overwriting calls
        if B >= 2:
            h = B // 2
            parts = [run_eval(lib, S, labels=y[s], spec=spec, k=k[s]) for s in (slice(0, h), slice(h, B))]
            first = run_eval(lib, S, labels=y[:h], spec=spec, k=k[:h], want=OUTPUTS[4:])
            both = run_eval(lib, S, labels=y[h:], spec=spec, k=k[h:], want=OUTPUTS[4:], accumulate=1,
                            init={n_: first[n_] for n_ in OUTPUTS[4:]})
            assert both["intact"]
            for name in OUTPUTS[4:]:
                assert np.array_equal(both[name], parts[0][name] + parts[1][name]), (S, B, T, name)


# ---- check 8: every NULL-output combination ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,T", [(65, 5, 2), (300, 3, 63), (4, 257, 1)])
def test_every_null_output_combination(lib, S, B, T):
    spec, _ = _pairs(S)[2]
    y, k = _labels(B, S, S + B), _cuts(B, S, T, S)
    full = run_eval(lib, S, labels=y, spec=spec, k=k)
    assert full["intact"]
    for mask in range(1, 1 << len(OUTPUTS)):
        want = tuple(n for i, n in enumerate(OUTPUTS) if mask >> i & 1)
        got = run_eval(lib, S, labels=y, spec=spec, k=k, want=want)
        assert got["intact"], want
        for n in OUTPUTS:
            if n in want:
                assert got[n].tobytes() == full[n].tobytes(), (want, n)
            else:
                assert got[n] is None


# ---- check 9: clamped cuts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 64, 300, 1023])
def test_clamped_cuts(lib, S):
    B = 5
    y = _labels(B, S, S)
    spec, _ = _pairs(S)[0]
    k = np.tile(np.array([-1, 0, S, S + 1, -(2 ** 31), 2 ** 31 - 1], dtype=np.int32), (B, 1))
    got = run_eval(lib, S, labels=y, spec=spec, k=k)
    assert got["intact"] and got["sums"][2] == 4 * B
    assert np.array_equal(_bits(got["r_at"][:, 0]), _bits(got["r_at"][:, 1])) and np.all(got["r_at"][:, :2] == 0.0)
    for c in (3, 5):
        assert np.array_equal(_bits(got["r_at"][:, c]), _bits(got["r_at"][:, 2]))
        assert np.array_equal(got["better"][:, c], got["better"][:, 2])
    assert np.array_equal(got["better"][:, 4], got["better"][:, 1])


# ---- check 6: F_1 on 0/1 labels against rlt_truncation_curves -----------------------------------------------------------------------
@pytest.mark.parametrize("S", [40, 129, 300])
def test_fbeta_one_against_truncation_curves(lib, S):
    """best_k == best_f1_k and best within one fp32 ulp of best_f1.  A list whose largest F1 is reached at several cuts in exact
    arithmetic is the one place the two can part: cal_F1's three roundings may break the tie by a float64 ulp (tests/
    test_reward_eval_restate.py); there best_k must be the FIRST exact maximiser and best_f1_k one of them."""
    from rlt_hip import ops
    B = 23
    y = (np.random.default_rng(S).random((B, S)) < 0.3).astype(np.float32)
    y[0] = 0.0
    y[1] = 1.0
    spec, _ = _pairs(S)[3]
    got = run_eval(lib, S, labels=y, spec=spec, allow_empty=1, want=("best", "best_k"))
    _c, _s, (bf, bfk, _bd, _bdk) = ops.truncation_curves(_dev(y), per_list=True)
    torch.cuda.synchronize()
    bf, bfk = bf.cpu().numpy(), bfk.cpu().numpy()
    exact = E.exact_f1_maximisers(y)
    unique = np.array([len(m) == 1 for m in exact])
    print(f"\nS = {S}: {int((~unique).sum())} of {B} lists tie exactly at their best F1; "
          f"{int((got['best_k'] != bfk).sum())} differ from best_f1_k")
    assert unique.sum() >= B - 2                    # the identity below is asserted on nearly every list
    assert [int(v) for v in got["best_k"]] == [m[0] for m in exact]
    assert np.array_equal(got["best_k"][unique], bfk[unique])
    assert all(int(v) in m for v, m in zip(bfk, exact))
    assert _ulps(got["best"], bf).max() <= 1


# ---- check 10: the Python layer -----------------------------------------------------------------------------------------------------
def test_reward_curves_over_three_batches(lib):
    from utils.baselines import RewardCurves, best_cut_reward, fixed_k_reward, greedy_k_reward
    S = 40
    spec, want = _pairs(S)[2]
    y = _labels(67, S, 1)
    rc = RewardCurves(S, spec)
    for part in (y[:5], y[5:40], y[40:]):
        rc.update(part)
    torch.cuda.synchronize()
    ref = E.spec_evaluate(y, want)
    assert rc.n_lists == 67
    r = E.row(R.reward(y, want))
    tol = _sum_bound(r)
    assert np.all(np.abs(rc.curve().cpu().numpy() - ref["curve"] / 67) <= tol)
    assert np.array_equal(rc.best_hist().cpu().numpy(), ref["best_hist"])
    assert abs(rc.best_cut() - ref["sums"][1] / 67) <= _sum_bound(ref["best"])
    assert rc.best_k() == int(np.argmax(ref["curve"])) and abs(rc.fixed_k(10) - ref["curve"][10] / 67) <= tol[10]
    assert abs(best_cut_reward(y, spec) - rc.best_cut()) <= _sum_bound(ref["best"])
    assert abs(fixed_k_reward(y, 10, spec) - rc.fixed_k(10)) <= tol[10]
    val, k = greedy_k_reward(y[:30], y[30:], spec)
    rval, rk = E.greedy_k(R.reward(y[:30], want), R.reward(y[30:], want))
    assert k == rk and abs(val - rval) <= (_sum_bound(E.row(R.reward(y[30:], want)))[k] if k else 0.0)
    no_empty = RewardCurves(S, "ndcg", allow_empty=False).update(y)
    ref1 = E.spec_evaluate(y, want, None, False)
    assert abs(no_empty.best_cut() - ref1["sums"][1] / 67) <= _sum_bound(ref1["best"]) and no_empty.best_k() >= 1


def test_cut_report_with_a_reward(lib):
    from utils.report import CutReport
    z = np.load(os.path.join(GOLDEN, "report_edge_s40.npz"))
    y, p = z["labels"].astype(np.float32), z["output"].astype(np.float32)
    B, S = y.shape
    spec, want = _pairs(S)[2]
    plain = CutReport(S).update(_dev(p), _dev(y))
    rep = CutReport(S, reward=spec).update(_dev(p)[:7], _dev(y)[:7]).update(_dev(p)[7:], _dev(y)[7:])
    q, q0 = rep.per_query(), plain.per_query()
    new = {"reward", "best_reward", "best_reward_k", "better_reward"}
    assert set(q) == set(q0) | new and not (set(q0) & new)                  # without reward=: no new keys
    assert not (set(plain.summary()) & {"reward", "best_reward", "reward_spec", "regret_reward"})
    for name in q0:
        assert q[name].tobytes() == q0[name].tobytes(), name
    ref = E.spec_evaluate(y, want, q["k"].reshape(B, 1), allow_empty=False)
    assert np.array_equal(_bits(q["reward"]), _bits(ref["r_at"][:, 0])) and np.array_equal(q["better_reward"], ref["better"][:, 0])
    assert np.array_equal(_bits(q["best_reward"]), _bits(ref["best"])) and np.array_equal(q["best_reward_k"], ref["best_k"])
    s = rep.summary()
    assert s["reward_spec"] == str(spec) and abs(s["reward"] - ref["sums"][3] / B) <= _sum_bound(ref["r_at"])[0]
    assert abs(s["best_reward"] - ref["sums"][1] / B) <= _sum_bound(ref["best"]) and s["best_cut_share_reward"] == ref["sums"][4] / B
    assert s["better_reward"] == ref["sums"][5] / B                         # a sum of integers: exact


def test_tune_cut_rule_on_a_reward(lib):
    from rlt_hip import ops
    from utils.sweep import tune_cut_rule
    z = np.load(os.path.join(GOLDEN, "report_edge_s40.npz"))
    y, p = z["labels"].astype(np.float32), np.abs(z["output"].astype(np.float32))
    B, S = y.shape
    spec, want = _pairs(S)[0]
    th = np.linspace(0.1, 0.9, 5)
    plain = tune_cut_rule([(_dev(p), _dev(y))], [(_dev(p), _dev(y))], "quantile", th)
    res = tune_cut_rule([(_dev(p[:9]), _dev(y[:9])), (_dev(p[9:]), _dev(y[9:]))], [(_dev(p), _dev(y))], "quantile", th, reward=spec)
    assert "reward" not in plain["test"] and "reward" not in plain["train_curve"]
    for name in ("k", "f1", "dcg", "fbeta"):                                # the F1 / DCG / F_beta columns are still produced
        assert np.allclose(res["test_curve"][name], plain["test_curve"][name], rtol=1e-15, atol=0)
    k, _ = ops.cut_sweep(_dev(p), _dev(th, torch.float64), "quantile")
    ref = E.spec_evaluate(y, want, k.cpu().numpy(), allow_empty=True)
    means = ref["sums"][3::3] / B
    tol = _sum_bound(ref["r_at"])
    assert np.all(np.abs(res["train_curve"]["reward"] - means) <= tol)
    assert res["metric"] == "reward" and res["index"] == int(np.argmax(res["train_curve"]["reward"]))
    assert abs(res["test"]["reward"] - means[res["index"]]) <= tol[res["index"]]


def test_compare_reports_on_the_reward(lib, tmp_path):
    from utils.compare import compare_reports
    from utils.report import CutReport
    z = np.load(os.path.join(GOLDEN, "report_edge_s40.npz"))
    y, p = z["labels"].astype(np.float32), z["output"].astype(np.float32)
    B, S = y.shape
    spec, want = _pairs(S)[2]
    paths, cols = [], []
    for i, out in enumerate((p, np.roll(p, 5, axis=1))):
        rep = CutReport(S, reward=spec).update(_dev(out), _dev(y))
        q = rep.per_query()
        path = str(tmp_path / f"run{i}.npz")
        np.savez(path, qid=np.asarray([f"q{j}" for j in range(B)]), length=np.full(B, S, dtype=np.int32),
                 reward_spec=np.asarray(rep.reward_text()), **q)
        paths.append(path)
        cols.append(E.spec_evaluate(y, want, q["k"].reshape(B, 1), False)["r_at"][:, 0].astype(np.float64))
    cmp = compare_reports(paths, metric="reward", resamples=200, seed=1)
    row = cmp.summary()[0]
    assert row["n"] == B and abs(row["mean_base"] - cols[0].mean()) <= 1e-12 and abs(row["mean_sys"] - cols[1].mean()) <= 1e-12
    assert row["wins"] == int((cols[1] > cols[0]).sum()) and row["losses"] == int((cols[1] < cols[0]).sum())
    top = compare_reports(paths, metric="reward", baseline="Oracle", resamples=0, keep_stats=False).summary()
    assert len(top) == 2 and all(r["mean_diff"] <= 0 for r in top)


# ---- run.py --eval-reward end to end: baselines, report, comparison, sweep, history ------------------------------------------------
def test_run_with_eval_reward_end_to_end(lib, tmp_path):
    """One epoch of Choopy on a synthetic set under --criterion ndcg; then the checkpoint goes through --baselines, --report-out,
    --compare-to, --cut-sweep (quantile: a model-based rule) and --history-json with --eval-reward criterion.  The figures are
    checked against the restatement on the split's own labels; a report written without the flag has none of the new keys and
    the same bytes in every other array."""
    import json
    import run
    from dataloader.synth import write_synthetic_robust04
    base, save = str(tmp_path / "data"), str(tmp_path / "ckpt")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=48, n_test=44, seed=11, seq_len=300)
    common = ["--model-name", "choopy", "--dataset-base", base, "--use-conf", "0", "--batch-size", "64", "--seed", "3", "--dropout", "0.1",
              "--save-path", save, "--criterion", "ndcg", "--tensorboard-dir", ""]
    run.main(common + ["--epochs", "1", "--model-persist", "1"])
    ckpt = os.path.join(save, "choopy.pkl")
    argv = common + ["--epochs", "0", "--ft", "1", "--model-path", ckpt]
    second, plain = (str(tmp_path / n) for n in ("b.npz", "plain.npz"))
    sweep_out, hist = str(tmp_path / "sweep.json"), str(tmp_path / "history.json")
    flag = ["--eval-reward", "criterion"]
    run.main(argv + flag + ["--report-out", second, "--baselines", "1", "--fixed-k", "5,30",
                            "--cut-sweep", "quantile:0.1:0.9:5", "--sweep-out", sweep_out, "--history-json", hist])
    run.main(argv + ["--report-out", plain])
    trainer = run.Trainer(run.build_parser().parse_args(argv + flag))
    (L, (_x, y_te, _q)), = sorted(trainer.data.buckets["test"].items())
    y_te, y_tr = np.asarray(y_te, dtype=np.float32), np.asarray(trainer.data.gety_train(), dtype=np.float32)
    B, want = len(y_te), R.ndcg()
    # the report: reward columns against the restatement at the report's own cuts
    d, p0 = np.load(second), np.load(plain)
    new = {"reward", "best_reward", "best_reward_k", "better_reward", "reward_spec"}
    assert set(d.files) == set(p0.files) | new and not (set(p0.files) & new)
    for key in p0.files:
        if key != "summary":
            assert d[key].tobytes() == p0[key].tobytes(), key
    assert not (set(json.loads(str(p0["summary"]))[str(L)]) & {"reward", "best_reward", "reward_spec", "regret_reward"})
    assert str(d["reward_spec"]) == "ndcg:-1.0"
    ref = E.spec_evaluate(y_te, want, d["k"].reshape(B, 1), allow_empty=False)
    assert np.array_equal(_bits(d["reward"]), _bits(ref["r_at"][:, 0])) and np.array_equal(d["better_reward"], ref["better"][:, 0])
    assert np.array_equal(_bits(d["best_reward"]), _bits(ref["best"])) and np.array_equal(d["best_reward_k"], ref["best_k"])
    h = json.load(open(hist))
    assert h["eval_reward"]["spec"] == "ndcg:-1.0"
    assert abs(h["eval_reward"]["report"][str(L)]["reward"] - ref["sums"][3] / B) <= _sum_bound(ref["r_at"])[0]
    # the baselines in the reward
    base_r = h["baselines"][str(L)]["reward"]
    full = E.spec_evaluate(y_te, want)
    tol = _sum_bound(E.row(R.reward(y_te, want)))
    assert abs(base_r["Oracle"] - full["sums"][1] / B) <= _sum_bound(full["best"])
    for k in (5, 30):
        assert abs(base_r["fixed_k"][str(k)] - full["curve"][k] / B) <= tol[k]
    gval, gk = E.greedy_k(R.reward(y_tr, want), R.reward(y_te, want))
    assert base_r["greedy_k"]["k"] == gk and abs(base_r["greedy_k"]["reward"] - gval) <= (tol[gk] if gk else 0.0)
    assert {"f1", "dcg"} <= set(h["baselines"][str(L)]["Oracle"])                      # the F1 / DCG rows are still there
    # the sweep: tau* on the mean reward, the argmax record carries the reward too
    sw = h["eval_reward"]["cut_sweep"][str(L)]
    curves = json.load(open(sweep_out))["curves"]
    assert sw["metric"] == "reward" and sw["index"] == int(np.argmax(curves[f"train_reward_{L}"]))
    assert sw["test"]["reward"] == curves[f"test_reward_{L}"][sw["index"]]
    assert abs(sw["argmax"]["reward"] - ref["sums"][3] / B) <= _sum_bound(ref["r_at"])[0] and "f1" in sw["argmax"]
    # the comparison runs on the reward column (a report against itself: every pair ties) and refuses a report without it
    lines = trainer.compare(second, second)
    assert len(lines) == 1 and f"W/T/L 0/{B}/0" in lines[0]
    with pytest.raises(ValueError, match="no 'reward' column"):
        trainer.compare(second, plain)
