"""Every dispatch branch of the scan / row-wise kernels around the hot path (csrc/loss.hip, heads.hip, norm.hip) against float64,
through the raw C ABI (rlt_hip.native) so that dp = NULL, loss_out = NULL, k_in, accumulate_dx, r = NULL are reachable.
`pytest -m gpu`.  Parametrised by BRANCH, the instantiation is named in the test id:

    general-C*      reward_loss_kernel<C> (one list per wavefront, C = positions per lane), scalar (S % 4 != 0) and 16-byte
                    staging (S % 4 == 0) paths; reached at S % 4 == 0, S <= 384 only without dp or through rlt_reward_matrix_ex
    h-LL16-R* / h-LL32-R*   reward_loss_h_kernel (four / two lists per wavefront, R rounds of 4 LL positions)
    V*-nch*         the heads / LayerNorm kernels: V floats per lane and load, nch = E / (64 V) loads per row

The reference is tests/loss_restate.py (float64 numpy, pinned to the reference's fixtures by tests/test_loss_restate.py) and
torch float64 for the heads and LayerNorm.  Tolerances are the ones tools/gpu_probe.py holds the same quantities to: batch
loss 2e-5 of max(1, |ref|) (per-list terms: the same form), dL/dp 1e-4 of max |ref|, cut positions identical, F1 / DCG 1e-12
(of max(1, |ref|)), fused loss == separate loss 1e-6, reward matrix 2e-5 of max(1, max |r_ref|) per row.

Conditions on the inputs, asserted on the restatement before a launch: the reference takes exp(r / tau) without subtracting the
maximum, so every case keeps max r / tau <= 80 (finite in the reference's own fp32); the all-relevant list breaks that under
DCG for S >~ 512 and is then replaced by a random list - that one row, never a case."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_restate as R

pytestmark = pytest.mark.gpu

KINDS = {"expect": R.EXPECT, "ce": R.CE, "kl": R.KL, "js": R.JS}
METRICS = [("f1", -1.0), ("dcg", -1.0), ("dcg", -0.5)]
TAUS = (0.85, 0.95, 1.0)
SENTINEL = 12345.0
C_SET = (1, 2, 3, 4, 5, 6, 8, 12, 16)


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rlt_hip import native
    native.load()
    return native


@pytest.fixture(scope="module")
def table(N):
    nbytes = N.query("rlt_dcg_table_bytes")
    t = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    N.call("rlt_dcg_table_init", N.ptr(t), nbytes, N.stream())
    torch.cuda.synchronize()
    return t


def general_c(S):
    return next(c for c in C_SET if c >= -(-S // 64))


def h_form(S, metric):
    """the instantiation dispatch_reward_m picks for S % 4 == 0, S <= 384 with p and dp present"""
    r16 = -(-S // 64)
    if (r16 & 1) and r16 <= (5 if metric == "f1" else 3):
        return f"LL16-R{r16}"
    return f"LL32-R{max(1, -(-S // 128))}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")          # (a copy: the shared inputs are read-only)


def padded(n, dtype, fill=SENTINEL, pad=64):
    """an n-element output followed by `pad` sentinel elements: a store beyond the array shows"""
    return torch.full((n + pad,), fill, dtype=dtype, device="cuda")


def unpad(t, n, what):
    h = t.cpu().numpy()
    assert (h[n:] == h.dtype.type(SENTINEL)).all(), f"{what}: written beyond its {n} elements"
    return h[:n]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@functools.lru_cache(maxsize=None)
def coef(S):
    return dev(np.array([math.log(j + 2, 2) for j in range(S)], dtype=np.float32))       # utils/metrics.py:7, fp32


@functools.lru_cache(maxsize=None)
def lists(B, S, lane_c, seed=0):
    """labels Bernoulli(0.2), rows 0-3: all zero, all one, a single positive first / last; p = softmax(3 randn) with one uniform
    row (the first position wins), one row whose maximum sits at j and j + 1, j + 1 = lane_c * lane (two lanes tie, the lower
    index wins) and one row with its maximum at S - 1.  -> (y, p, {row: expected k})"""
    g = np.random.default_rng(1000003 * B + 1009 * S + seed)
    y = (g.random((B, S)) < 0.2).astype(np.float32)
    for row, fill in ((0, "zero"), (1, "one"), (2, "first"), (3, "last")):
        if row < B:
            y[row] = 1.0 if fill == "one" else 0.0
            if fill == "first":
                y[row, 0] = 1.0
            if fill == "last":
                y[row, -1] = 1.0
    z = 3.0 * g.standard_normal((B, S))
    p = np.exp(z - z.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    # (B < 7: the last rows, the maximum-at-the-end row first - a one-list batch of no relevant document and a uniform p would
    # have q == p and a JS gradient of exactly zero, nothing to compare against)
    rows = [6, 5, 4] if B >= 7 else list(range(B))[::-1][:3]
    want = {}
    if rows:
        p[rows[0], S - 1] = 2.0 * p[rows[0]].max()
        want[rows[0]] = S
    if len(rows) > 1 and (S - 1) // lane_c >= 1:
        j1 = lane_c * (((S - 1) // lane_c + 1) // 2)
        p[rows[1], j1 - 1] = p[rows[1], j1] = 2.0 * p[rows[1]].max()
        want[rows[1]] = j1                      # index j1 - 1, k = index + 1
    if len(rows) > 2:
        p[rows[2]] = np.float32(1.0 / S)
        want[rows[2]] = 1
    y.setflags(write=False)
    p.setflags(write=False)
    return y, p, want


def finite_labels(y, metric, penalty, tau):
    """max r / tau <= 80 on the restatement; under DCG the all-relevant list (row 1) is the one row that may be replaced"""
    if metric == "dcg":
        over = np.nonzero(R.reward(y, metric, penalty).max(1) / tau > 80)[0]
        if len(over):
            assert list(over) == [1], over
            y = y.copy()
            y[1] = (np.random.default_rng(y.shape[1]).random(y.shape[1]) < 0.2).astype(np.float32)
    assert R.reward(y, metric, penalty).max() / tau <= 80
    return y


def run_loss(N, table, p, y, metric, penalty, kind, tau, fused, with_dp=True, with_loss_out=True, mpen=-1.0):
    B, S = y.shape
    pd, yd = dev(p), dev(y)
    cf = coef(S) if metric == "dcg" else None
    per, loss = padded(B, torch.float32), padded(1, torch.float32)
    dp = padded(B * S, torch.float32) if with_dp else None
    out = {}
    m = N.METRIC_F1 if metric == "f1" else N.METRIC_DCG
    if fused:
        k, f1, dcg, sums = padded(B, torch.int32, 12345), padded(B, torch.float64), padded(B, torch.float64), padded(2, torch.float64)
        ws_bytes = N.query("rlt_loss_metrics_workspace", B)
        ws = N.byte_buffer(ws_bytes, "cuda")
        N.call("rlt_loss_metrics", N.ptr(pd), N.ptr(yd), N.ptr(cf), B, S, m, penalty, kind, tau, mpen, N.ptr(per), N.ptr(loss),
               N.ptr(dp), N.ptr(k), N.ptr(f1), N.ptr(dcg), N.ptr(sums), N.ptr(table), N.ptr(ws), ws_bytes, N.stream())
        torch.cuda.synchronize()
        out.update(k=unpad(k, B, "k"), f1=unpad(f1, B, "f1"), dcg=unpad(dcg, B, "dcg"), sums=unpad(sums, 2, "sums"))
    else:
        N.call("rlt_reward_loss_ex", N.ptr(pd), N.ptr(yd), N.ptr(cf), B, S, m, penalty, kind, tau, N.ptr(per),
               N.ptr(loss) if with_loss_out else None, N.ptr(dp), N.stream())
        torch.cuda.synchronize()
    out["per"] = unpad(per, B, "loss_per_list")
    out["loss"] = float(unpad(loss, 1, "loss_out")[0]) if (fused or with_loss_out) else None
    if not fused and not with_loss_out:
        assert loss.cpu()[0] == SENTINEL
    out["dp"] = unpad(dp, B * S, "dp").reshape(B, S) if with_dp else None
    return out


class Tally:
    """collects every figure of a test against its bound; the test prints the worst of each kind, then asserts none is over"""

    def __init__(self):
        self.worst, self.bad = {}, []

    def add(self, what, case, err, tol):
        if not (err <= tol):
            self.bad.append((what, case, err, tol))
        if what not in self.worst or not (err <= self.worst[what][0]):
            self.worst[what] = (err, tol, case)

    def done(self):
        for what, (err, tol, case) in self.worst.items():
            print(f"  worst {what:18s} {err:.3e} (bound {tol:.1e}) at {case}")
        assert not self.bad, f"{len(self.bad)} figures over their bound: {self.bad[:6]}"


def check_loss(t, case, out, ref, y, p, want_k, mpen):
    per_ref, loss_ref, dp_ref, _, _ = ref
    if out["loss"] is not None:
        t.add("loss", case, abs(out["loss"] - loss_ref) / max(1.0, abs(loss_ref)), 2e-5)
    t.add("loss per list", case, float((np.abs(out["per"] - per_ref) / np.maximum(1.0, np.abs(per_ref))).max()), 2e-5)
    if out["dp"] is not None:
        t.add("dp", case, rel(out["dp"], dp_ref), 1e-4)
    if "k" in out:
        k_ref = R.cut_positions(p)
        for row, k in want_k.items():
            assert k_ref[row] == k, (row, k_ref[row], k)
        t.add("k", case, float((out["k"] != k_ref).sum()), 0)
        f1_ref, dcg_ref = R.f1_at(y, k_ref), R.dcg_at(y, k_ref, mpen)
        t.add("F1@k", case, float(np.abs(out["f1"] - f1_ref).max()), 1e-12)
        t.add("DCG@k", case, float((np.abs(out["dcg"] - dcg_ref) / np.maximum(1.0, np.abs(dcg_ref))).max()), 1e-12)
        B = len(y)
        t.add("mean F1", case, abs(out["sums"][0] / B - f1_ref.mean()), 1e-12)
        t.add("mean DCG", case, abs(out["sums"][1] / B - dcg_ref.mean()) / max(1.0, abs(dcg_ref.mean())), 1e-12)


def sweep(N, table, t, B, S, lane_c, combos, with_dp=True, entries=("plain", "fused"), tag=""):
    """combos: (metric, penalty, kind name); tau and the fused pass's metric penalty are spread over them"""
    y0, p, want_k = lists(B, S, lane_c)
    for i, (metric, penalty, kname) in enumerate(combos):
        tau, mpen = TAUS[(i + S) % 3], (-1.0, -2.0)[i % 2]
        y = finite_labels(y0, metric, penalty, tau)
        ref = R.reward_loss(p, y, metric, KINDS[kname], tau, penalty)
        outs = {}
        for entry in entries:
            case = f"{tag}{entry} {metric}{penalty:g} {kname} tau{tau} B{B} S{S}"
            # the loss-only form also without loss_out: the per-list terms are then the only output
            no_out = entry == "plain" and not with_dp and kname == "kl"
            outs[entry] = run_loss(N, table, p, y, metric, penalty, KINDS[kname], tau, entry == "fused", with_dp,
                                   with_loss_out=not no_out, mpen=mpen)
            check_loss(t, case, outs[entry], ref, y, p, want_k, mpen)
        if len(outs) == 2 and outs["plain"]["loss"] is not None:
            a, b = outs["plain"]["loss"], outs["fused"]["loss"]
            t.add("fused == separate", f"{metric}{penalty:g} {kname} S{S}", abs(a - b) / max(1.0, abs(a)), 1e-6)


ALL_COMBOS = [(m, pen, k) for (m, pen) in METRICS for k in KINDS]

SCALAR_S = (1, 2, 3, 63, 65, 127, 129, 191, 193, 255, 257, 319, 321, 383, 385, 511, 513, 767, 769, 1023)


@pytest.mark.parametrize("S", SCALAR_S, ids=lambda S: f"general-C{general_c(S)}-scalar-S{S}")
def test_general_pass_scalar_path(N, table, S):
    """reward_loss_kernel<C, false | true>, S % 4 != 0: 4 loss kinds x {F1, DCG penalty -1, -0.5}, rlt_reward_loss_ex and
    rlt_loss_metrics (metric penalty -1 / -2), B = 17."""
    t = Tally()
    sweep(N, table, t, 17, S, general_c(S), ALL_COMBOS)
    t.done()


VECTOR_S = [(S, False) for S in (4, 64, 128, 192, 256, 320, 384)] + [(S, True) for S in (512, 768, 1024)]


@pytest.mark.parametrize("S,with_dp", VECTOR_S, ids=lambda v: (f"general-C{general_c(v)}-vector-S{v}" if not isinstance(v, bool)
                                                                else ("dp" if v else "dpNULL")))
def test_general_pass_vector_path(N, table, S, with_dp):
    """reward_loss_kernel<C>, S % 4 == 0 (16-byte staging and write-back).  S <= 384 reaches it through the documented dp == NULL
    form (loss only; for KL also without loss_out), S > 384 with dp."""
    t = Tally()
    sweep(N, table, t, 17, S, general_c(S), ALL_COMBOS, with_dp=with_dp)
    t.done()


def reference_arithmetic_error(y, penalty):
    """What the REFERENCE's arithmetic gives for the DCG reward against float64 on the same labels, per row, as a fraction of
    max(1, max |r|): float32 1 / log2(j + 2) gains under a sequential float32 running sum (utils/metrics.py:93-101)."""
    S = y.shape[1]
    c32 = np.array([math.log(j + 2, 2) for j in range(S)], dtype=np.float32)
    gain = np.where(y == 1.0, np.float32(1.0) / c32, (np.float32(1.0) / c32) * np.float32(penalty)).astype(np.float32)
    r32 = np.cumsum(gain, axis=1, dtype=np.float32)
    r64 = R.reward(y, "dcg", penalty)
    return np.abs(r32 - r64).max(1) / np.maximum(1.0, np.abs(r64).max(1))


@pytest.mark.parametrize("outs", ["r", "q", "rq"])
@pytest.mark.parametrize("S", [64, 65, 256, 257, 768, 1024], ids=lambda S: f"general-C{general_c(S)}-{'vector' if S % 4 == 0 else 'scalar'}-S{S}")
def test_reward_matrix(N, S, outs):
    """rlt_reward_matrix_ex (p == NULL) with r_out, q_out or both.  r: 2e-5 of max(1, max |r_ref|) per row (|r| reaches 130
    under DCG at S = 1024).  q = exp(r / tau) / Z carries the error of r twice (numerator and normaliser) over tau plus the
    1-ulp exp2 / rcp: |dq| <= (2 * 2e-5 max(1, max |r|) / tau + 4e-6) q, element by element, plus max(1, 1 / Z) times the
    smallest fp32 normal: v_exp_f32 returns zero below it, and the normaliser scales that loss by 1 / Z.
    Measured on an MI355X: r within 1.9e-7 of float64 (the reference's own arithmetic - float32 1 / log2(j + 2) under a
    sequential float32 running sum, printed per case - is 1.1e-6 away at S = 1024), so the 2e-5 stands as it is."""
    t = Tally()
    B = 17
    y0, _, _ = lists(B, S, general_c(S))
    for i, (metric, penalty) in enumerate(METRICS):
        tau = TAUS[(i + S) % 3]
        y = finite_labels(y0, metric, penalty, tau)
        r_ref = R.reward(y, metric, penalty)
        q_ref = R.reward_distribution(r_ref, tau)
        r_out = padded(B * S, torch.float32) if "r" in outs else None
        q_out = padded(B * S, torch.float32) if "q" in outs else None
        yd = dev(y)
        N.call("rlt_reward_matrix_ex", N.ptr(yd), N.ptr(coef(S)) if metric == "dcg" else None, B, S,
               N.METRIC_F1 if metric == "f1" else N.METRIC_DCG, penalty, tau, N.ptr(r_out), N.ptr(q_out), N.stream())
        torch.cuda.synchronize()
        case = f"{metric}{penalty:g} tau{tau} S{S} {outs}"
        scale = np.maximum(1.0, np.abs(r_ref).max(1, keepdims=True))
        if r_out is not None:
            r = unpad(r_out, B * S, "r_out").reshape(B, S)
            t.add("r", case, float((np.abs(r - r_ref) / scale).max()), 2e-5)
            if metric == "dcg":
                print(f"  {case}: reference arithmetic vs float64 {reference_arithmetic_error(y, penalty).max():.3e}")
        if q_out is not None:
            q = unpad(q_out, B * S, "q_out").reshape(B, S)
            z_ref = np.exp(r_ref / tau).sum(1, keepdims=True)
            bound = (2 * 2e-5 * scale / tau + 4e-6) * q_ref + 1.17549435e-38 * np.maximum(1.0, 1.0 / z_ref)
            t.add("q / bound", case, float((np.abs(q - q_ref) / bound).max()), 1.0)
            t.add("sum q", case, float(np.abs(q.astype(np.float64).sum(1) - 1.0).max()), 1e-5)
    t.done()


H_S = (60, 64, 68, 188, 192, 196, 316, 320, 324, 380, 384)
H_COMBOS = [(m, -1.0, k) for m in ("f1", "dcg") for k in KINDS]


@pytest.mark.parametrize("S", H_S, ids=lambda S: f"h-f1-{h_form(S, 'f1')}-dcg-{h_form(S, 'dcg')}-S{S}")
def test_lists_per_wavefront_family(N, table, S):
    """reward_loss_h_kernel<R, METRICS, F1, LL>: the full-round lengths 64 / 192 / 320 of the four-lists form (LL = 16, R = 1 /
    3 / 5), one step either side of them, and the two-lists form's rounds (LL = 32, R = 1 / 2 / 3; DCG at five rounds of 64
    falls to LL = 32, R = 3).  F1 and DCG, plain and fused, B = 17 (odd: the last wavefront works part of its groups).  The
    tie row's two maxima sit in neighbouring lanes (j + 1 a multiple of 4)."""
    t = Tally()
    sweep(N, table, t, 17, S, 4, H_COMBOS)
    t.done()


@pytest.mark.parametrize("S", [300, 64], ids=lambda S: f"h-f1-{h_form(S, 'f1')}-dcg-{h_form(S, 'dcg')}-S{S}")
@pytest.mark.parametrize("B", [1, 3, 4, 5, 15, 16])
def test_lists_per_wavefront_family_partial_groups(N, table, B, S):
    """B below, at and one past a wavefront's 2 / 4 lists and a workgroup's 8 / 16: idle groups shadow a live list, stores masked"""
    t = Tally()
    sweep(N, table, t, B, S, 4, [("f1", -1.0, "js"), ("dcg", -1.0, "ce"), ("f1", -1.0, "expect"), ("dcg", -1.0, "kl")])
    t.done()


@pytest.mark.parametrize("B,S,form", [(8197, 5, "general-C1"), (16389, 68, "h-LL32-R1"), (32771, 4, "h-LL16-R1")],
                         ids=lambda v: str(v))
def test_grid_striding_against_the_restatement(N, table, B, S, form):
    """More lists than one sweep of the grid (2048 workgroups of 4 / 8 / 16 lists) covers, 5 past it: the stride itself against
    float64 - 'fused == separate' on the device would agree with itself under a wrong stride."""
    assert (form == "general-C1") == (S % 4 != 0) and (S % 4 != 0 or form == "h-" + h_form(S, "f1") == "h-" + h_form(S, "dcg"))
    t = Tally()
    sweep(N, table, t, B, S, 4 if S % 4 == 0 else 1, [("f1", -1.0, "js"), ("dcg", -1.0, "kl")], tag=form + " ")
    t.done()


# ---------------------------------------------------------------------------------------------- cut and task metrics
GRID_BS = [(B, S) for B in (1, 5, 259) for S in (1, 63, 64, 65, 300, 1024)]


@pytest.mark.parametrize("B,S", GRID_BS, ids=lambda v: str(v))
def test_cut_metrics(N, B, S):
    """rlt_cut_metrics_ex: the argmax path (first maximum) and the k_in path (rows with k = 1 and k = S), penalty -1 / 0.25,
    and the one-workgroup sum kernel (B = 259 > its 256 threads)."""
    t = Tally()
    y, p, want_k = lists(B, S, 1)
    g = np.random.default_rng(B * 4099 + S)
    k_in = g.integers(1, S + 1, size=B).astype(np.int32)
    k_in[0] = 1
    k_in[-1] = S
    yd, pd, kd = dev(y), dev(p), dev(k_in)
    for penalty in (-1.0, 0.25):
        for path in ("argmax", "k_in"):
            k, f1, dcg, sums = padded(B, torch.int32, 12345), padded(B, torch.float64), padded(B, torch.float64), padded(2, torch.float64)
            N.call("rlt_cut_metrics_ex", N.ptr(pd) if path == "argmax" else None, N.ptr(yd), N.ptr(kd) if path == "k_in" else None,
                   B, S, penalty, N.ptr(k), N.ptr(f1), N.ptr(dcg), N.ptr(sums), N.stream())
            torch.cuda.synchronize()
            k_ref = R.cut_positions(p) if path == "argmax" else k_in.astype(np.int64)
            if path == "argmax":
                for row, kk in want_k.items():
                    assert k_ref[row] == kk
            case = f"{path} pen{penalty:g} B{B} S{S}"
            f1_ref, dcg_ref = R.f1_at(y, k_ref), R.dcg_at(y, k_ref, penalty)
            t.add("k", case, float((unpad(k, B, "k") != k_ref).sum()), 0)
            t.add("F1@k", case, float(np.abs(unpad(f1, B, "f1") - f1_ref).max()), 1e-12)
            t.add("DCG@k", case, float((np.abs(unpad(dcg, B, "dcg") - dcg_ref) / np.maximum(1.0, np.abs(dcg_ref))).max()), 1e-12)
            s = unpad(sums, 2, "sums")
            t.add("mean F1", case, abs(s[0] / B - f1_ref.mean()), 1e-12)
            t.add("mean DCG", case, abs(s[1] / B - dcg_ref.mean()) / max(1.0, abs(dcg_ref.mean())), 1e-12)
    t.done()


@pytest.mark.parametrize("B,S", GRID_BS, ids=lambda v: str(v))
def test_task_metrics(N, B, S):
    """rlt_task_metrics: continuous predictions and predictions quantised to 4 levels (heavy ties), one all-equal row; the
    all-relevant and the all-irrelevant list have AUC -1 and stay out of sums[1] / sums[2].  DCG 1e-9, AUC 1e-12."""
    t = Tally()
    y, p, _ = lists(B, S, 1)
    cont = (p / p.max(1, keepdims=True)).astype(np.float32)
    for name, pred in (("continuous", cont), ("4 levels", (np.round(cont * 3) / 3).astype(np.float32))):
        pred = pred.copy()
        pred[B // 2] = 0.25                                   # all equal: rank = index, every pair tied
        dcg, auc, sums = padded(B, torch.float64), padded(B, torch.float64), padded(3, torch.float64)
        yd, pd = dev(y), dev(pred)
        N.call("rlt_task_metrics", N.ptr(yd), N.ptr(pd), B, S, N.ptr(dcg), N.ptr(auc), N.ptr(sums), N.stream())
        torch.cuda.synchronize()
        dcg_ref, auc_ref = R.task_dcg(y, pred), R.task_auc(y, pred)
        one_class = (y.sum(1) == 0) | (y.sum(1) == S)
        assert one_class[0] and (B < 2 or one_class[1]) and (auc_ref[one_class] == -1.0).all() and (auc_ref[~one_class] >= 0).all()
        case = f"{name} B{B} S{S}"
        d, a, s = unpad(dcg, B, "dcg"), unpad(auc, B, "auc"), unpad(sums, 3, "sums")
        t.add("task DCG", case, float(np.abs(d - dcg_ref).max()), 1e-9)
        t.add("AUC", case, float(np.abs(a - auc_ref).max()), 1e-12)
        t.add("skipped lists", case, float(((a == -1.0) != one_class).sum()), 0)
        t.add("mean task DCG", case, abs(s[0] / B - dcg_ref.mean()), 1e-9)
        t.add("valid lists", case, abs(s[2] - float((~one_class).sum())), 0)
        if (~one_class).any():
            t.add("mean AUC", case, abs(s[1] / s[2] - auc_ref[~one_class].mean()), 1e-12)
        else:
            t.add("sum AUC", case, abs(s[1]), 0)
    t.done()


# ---------------------------------------------------------------------------------------------- multi-task terms
@pytest.mark.parametrize("B,S", [(1, 1), (1, 255), (1, 257), (5, 300), (7001, 300)], ids=lambda v: str(v))
def test_mt_terms(N, B, S):
    """rlt_mt_terms / rlt_mt_terms_bwd: n = B S from one element to 2,100,300 (past the 1024 workgroups x 2048 elements one
    sweep of mt_partial_kernel covers); rerank only, class only, both; an empty class (all labels 1: hinge and both gradients
    0), an inactive hinge (margin -10), class probabilities of exactly 0.0 and 1.0 (the -100 clamp, torch's backward), gscale
    NULL and 0.5.  terms 1e-5 absolute (the two gradient constants also 1e-6 of themselves), d_rerank 1e-7, d_class 1e-4."""
    t = Tally()
    g = np.random.default_rng(B * 7919 + S)
    n = B * S
    y0 = (g.random((B, S)) < 0.2).astype(np.float32)
    s = g.standard_normal((B, S)).astype(np.float32)
    c = (1.0 / (1.0 + np.exp(-2.0 * g.standard_normal((B, S))))).astype(np.float32)
    c_edge = c.copy()
    c_edge.ravel()[::3] = np.array([0.0, 1.0], dtype=np.float32)[np.arange(len(c_edge.ravel()[::3])) % 2]
    ws_bytes = N.query("rlt_mt_terms_workspace", B, S)
    ws = N.byte_buffer(ws_bytes, "cuda")
    half = dev(np.array([0.5], dtype=np.float32))
    scenarios = [("plain", y0, c, 1.0), ("empty class", np.ones_like(y0), c, 5e-4), ("inactive", y0, c, -10.0), ("clamp", y0, c_edge, 0.3)]
    for name, y, cls, margin in scenarios:
        yd, sd, cd = dev(y), dev(s), dev(cls)
        for mode in ("rerank", "class", "both"):
            rr, cc = (s if mode != "class" else None), (cls if mode != "rerank" else None)
            terms = padded(4, torch.float32)
            N.call("rlt_mt_terms", N.ptr(sd) if rr is not None else None, N.ptr(cd) if cc is not None else None, N.ptr(yd), B, S,
                   margin, N.ptr(terms), N.ptr(ws), ws_bytes, N.stream())
            torch.cuda.synchronize()
            got, ref = unpad(terms, 4, "terms"), R.mt_terms(rr, cc, y, margin)
            case = f"{name} {mode} n{n}"
            t.add("terms", case, float(np.abs(got - ref).max()), 1e-5)
            t.add("dhinge constants", case, float((np.abs(got[2:] - ref[2:]) / np.maximum(np.abs(ref[2:]), 1e-30)).max()), 1e-6)
            if name in ("empty class", "inactive") or n == 1:
                assert ref[0] == 0 and ref[2] == 0 and ref[3] == 0 and got[0] == 0 and got[2] == 0 and got[3] == 0, (case, got)
            elif rr is not None and name == "plain":
                assert ref[0] > 0, case                     # (margin 1: the hinge is active)
            for gs_name, gs_t, gs in (("NULL", None, 1.0), ("0.5", half, 0.5)):
                d_rr = padded(n, torch.float32) if rr is not None else None
                d_cl = padded(n, torch.float32) if cc is not None else None
                N.call("rlt_mt_terms_bwd", N.ptr(cd) if cc is not None else None, N.ptr(yd), N.ptr(terms), B, S, 0.4, 0.6, N.ptr(gs_t),
                       N.ptr(d_rr), N.ptr(d_cl), N.stream())
                torch.cuda.synchronize()
                r_ref, c_ref = R.mt_terms_bwd(cc, y, ref, 0.4, 0.6, gs)
                if rr is not None:
                    t.add("d_rerank", f"{case} gscale {gs_name}", float(np.abs(unpad(d_rr, n, "d_rerank").reshape(B, S) - r_ref).max()), 1e-7)
                if cc is not None:
                    t.add("d_class", f"{case} gscale {gs_name}", rel(unpad(d_cl, n, "d_class").reshape(B, S), c_ref), 1e-4)
    t.done()


@pytest.mark.parametrize("n", range(1, 9))
def test_weighted_sum_is_the_fp32_sum_in_order(N, n):
    g = np.random.default_rng(n)
    xs = g.standard_normal(n).astype(np.float32)
    w = g.standard_normal(n).astype(np.float32)
    xt = [dev(xs[i:i + 1]) for i in range(n)]
    out = padded(1, torch.float32)
    N.call("rlt_weighted_sum", N.pointer_array(xt), (N.c_float * n)(*[float(v) for v in w]), n, N.ptr(out), N.stream())
    torch.cuda.synchronize()
    acc = np.float32(0.0)
    for i in range(n):
        acc = np.float32(acc + np.float32(w[i] * xs[i]))
    assert unpad(out, 1, "out")[0] == acc


@pytest.mark.parametrize("n", [1, 255, 1025, 4096 * 1024 + 3])
def test_scale_and_relu_bwd_are_exact(N, n):
    """rlt_scale (x *= *scale) and rlt_relu_bwd (dX = 0 where not Y > 0), the largest n past one sweep of their grid"""
    g = np.random.default_rng(n)
    x = g.standard_normal(n).astype(np.float32)
    yv = g.standard_normal(n).astype(np.float32)
    yv[::7] = 0.0
    yv[3::11] = -0.0
    f = np.array([0.3], dtype=np.float32)
    xd = padded(n, torch.float32)
    xd[:n] = dev(x)
    fd, yd = dev(f), dev(yv)
    N.call("rlt_scale", N.ptr(xd), N.ptr(fd), n, N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(unpad(xd, n, "x"), x * f[0])
    xd[:n] = dev(x)
    N.call("rlt_relu_bwd", N.ptr(xd), N.ptr(yd), n, N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(unpad(xd, n, "dX"), np.where(yv > 0, x, np.float32(0.0)))


# ---------------------------------------------------------------------------------------------- heads, LayerNorm
def vn(E):
    V = 4 if E % 256 == 0 else (2 if E % 128 == 0 else 1)
    return f"V{V}-nch{E // (64 * V)}-E{E}"


@pytest.mark.parametrize("E", [64, 192, 128, 384, 256, 512, 768, 1024], ids=vn)
def test_heads(N, E):
    """rlt_heads_fwd / rlt_heads_bwd against torch float64: every V / nch, S below the workgroup's 4 wavefronts and at the LDS
    limit 1024, one to three heads of every kind, dx overwritten and accumulated onto a pre-filled dx.  fwd 1e-5, dx / dw 2e-5
    of the largest reference value, db 2e-5 absolute (a softmax head's bias gradient is analytically zero)."""
    t = Tally()
    for (S, B) in ((1, 1), (3, 5), (63, 2), (65, 2), (300, 3), (1024, 1)):
        for kinds in ([0], [1, 0], [2, 1, 0], [0, 0, 0]):
            nh = len(kinds)
            gen = torch.Generator().manual_seed(E * 100003 + S * 101 + nh)
            x = torch.randn(S * B, E, generator=gen)                                   # position-major rows s * B + b
            w, b = torch.randn(nh, E, generator=gen) / math.sqrt(E), torch.randn(nh, generator=gen)
            dout, dx0 = torch.randn(nh, B, S, generator=gen), torch.randn(S * B, E, generator=gen)
            xr, wr, br = [v.clone().double().requires_grad_(True) for v in (x, w, b)]
            xb = xr.reshape(S, B, E).permute(1, 0, 2)
            heads = []
            for i, k in enumerate(kinds):
                z = xb @ wr[i] + br[i]
                heads.append(torch.softmax(z, 1) if k == 0 else (torch.sigmoid(z) if k == 1 else z))
            yr = torch.stack(heads)
            yr.backward(dout.double())
            case = f"S{S} B{B} E{E} {kinds}"
            karr = (N.c_int * nh)(*kinds)
            xd, wd, bd, doutd = x.cuda(), w.cuda(), b.cuda(), dout.cuda()
            out = padded(nh * B * S, torch.float32)
            N.call("rlt_heads_fwd", N.ptr(xd), N.ptr(wd), N.ptr(bd), karr, nh, S, B, E, N.ptr(out), N.stream())
            torch.cuda.synchronize()
            t.add("fwd", case, rel(unpad(out, nh * B * S, "out").reshape(nh, B, S), yr.detach().numpy()), 1e-5)
            ws_bytes = N.query("rlt_heads_bwd_workspace", nh, S, B, E)
            ws = N.byte_buffer(ws_bytes, "cuda")
            for acc in (0, 1):
                dx = padded(S * B * E, torch.float32)
                dx[:S * B * E] = dx0.cuda().reshape(-1)
                dw, db = padded(nh * E, torch.float32), padded(nh, torch.float32)
                N.call("rlt_heads_bwd", N.ptr(xd), N.ptr(wd), karr, nh, N.ptr(out), N.ptr(doutd), S, B, E, N.ptr(dx), acc,
                       N.ptr(dw), N.ptr(db), N.ptr(ws), ws_bytes, N.stream())
                torch.cuda.synchronize()
                want_dx = xr.grad.numpy() + (dx0.double().numpy() if acc else 0.0)
                t.add(f"dx accumulate={acc}", case, rel(unpad(dx, S * B * E, "dx").reshape(S * B, E), want_dx), 2e-5)
                t.add("dw", case, rel(unpad(dw, nh * E, "dw").reshape(nh, E), wr.grad.numpy()), 2e-5)
                t.add("db", case, float(np.abs(unpad(db, nh, "db") - br.grad.numpy()).max()), 2e-5)
    t.done()


@pytest.mark.parametrize("E,Ts", [(192, (1, 3, 5, 333)), (384, (1, 3, 5, 333)), (768, (1, 3, 5, 333)), (1024, (1, 3, 5, 333)), (64, (8195,))],
                         ids=lambda v: vn(v) if isinstance(v, int) else "T" + "_".join(map(str, v)))
def test_add_layernorm(N, E, Ts):
    """rlt_add_layernorm_fwd / _bwd against torch float64: every V / nch the sections above leave out, T below a workgroup's 4
    rows, T = 8195 past one sweep of the 2048-workgroup grid, r == NULL, dgamma / dbeta overwritten and accumulated onto
    pre-filled values.  fwd 5e-6, gradients 2e-5 (of the largest reference value)."""
    t = Tally()
    F = torch.nn.functional
    for T in Ts:
        for with_r in (True, False):
            gen = torch.Generator().manual_seed(E * 7 + T + with_r)
            x, r, dy = (torch.randn(T, E, generator=gen) for _ in range(3))
            gam, bet, g0, b0 = (torch.randn(E, generator=gen) for _ in range(4))
            xr, gr, br = [v.clone().double().requires_grad_(True) for v in (x, gam, bet)]
            yr = F.layer_norm(xr + r.double() if with_r else xr, (E,), gr, br, 1e-5)
            yr.backward(dy.double())
            case = f"T{T} E{E} r={'yes' if with_r else 'NULL'}"
            xd, rd, gd, bd, dyd = x.cuda(), (r.cuda() if with_r else None), gam.cuda(), bet.cuda(), dy.cuda()
            y, stats = padded(T * E, torch.float32), padded(2 * T, torch.float32)
            N.call("rlt_add_layernorm_fwd", N.ptr(xd), N.ptr(rd), N.ptr(gd), N.ptr(bd), T, E, 1e-5, 0.0, 0, N.ptr(y), N.ptr(stats), N.stream())
            torch.cuda.synchronize()
            t.add("fwd", case, rel(unpad(y, T * E, "y").reshape(T, E), yr.detach().numpy()), 5e-6)
            unpad(stats, 2 * T, "stats")
            ws_bytes = N.query("rlt_add_layernorm_bwd_workspace", T, E)
            ws = N.byte_buffer(ws_bytes, "cuda")
            for acc in (0, 1):
                dz, dg, db = padded(T * E, torch.float32), padded(E, torch.float32), padded(E, torch.float32)
                dg[:E], db[:E] = g0.cuda(), b0.cuda()
                N.call("rlt_add_layernorm_bwd", N.ptr(xd), N.ptr(rd), N.ptr(gd), N.ptr(stats), N.ptr(dyd), T, E, 0.0, 0, N.ptr(dz), None,
                       N.ptr(dg), N.ptr(db), acc, N.ptr(ws), ws_bytes, N.stream())
                torch.cuda.synchronize()
                t.add("dz", case, rel(unpad(dz, T * E, "dz").reshape(T, E), xr.grad.numpy()), 2e-5)
                t.add(f"dgamma accumulate={acc}", case, rel(unpad(dg, E, "dgamma"), gr.grad.numpy() + (g0.double().numpy() if acc else 0.0)), 2e-5)
                t.add(f"dbeta accumulate={acc}", case, rel(unpad(db, E, "dbeta"), br.grad.numpy() + (b0.double().numpy() if acc else 0.0)), 2e-5)
    t.done()
