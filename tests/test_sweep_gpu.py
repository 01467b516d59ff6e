"""The cut sweep on the MI355X (rlt_cut_sweep through the raw ABI, ops.cut_sweep, utils/sweep.py, utils/baselines.py and the models'
truncate) against the float64 numpy restatement (tests/sweep_restate.py) and ops.cut_metrics.

Conditions:
  * k equals the restatement exactly.  Only for QUANTILE, pairs (list, tau) with min_j |C_j - tau C_S| <= 2^-40 C_S (C_S > 0) are
    left out - another summation order may flip them - and at most 0.1 % of a case's pairs may be (asserted; on these inputs none
    is: the float64 sums of the fp32 softmax values are exact in any order).  The planted all-zero and NaN rows are NOT left out.
  * rows 0, 6, 7 of the curve (sums of integers) are exact;
  * F1 per list - the curve of a B = 1 call - is bit-equal to ops.cut_metrics(None, y, k_in=k[:, t]) wherever k >= 1;
  * rows 1, 3, 4, 5 within B 2^-52 sum|value| of the restatement: each value carries at most a few roundings of 2^-53 on either
    side and the B-term sums in another order (B - 1) 2^-53 sum|value| each;
  * row 2 (DCG) within (S + B) 2^-52 sum|term|: the prefix of at most S terms in another order, the table's 1 / log2 against
    numpy's division, and the B-term sum;
  * the two FIRST rules compare the inputs themselves: no exclusions.
Every device call of the shape sweep goes through the raw ABI with NaN sentinels in and around the outputs."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_restate as W  # noqa: E402

SHAPES = [(1, 1), (7, 5), (64, 67), (65, 67), (300, 67), (300, 1030), (1024, 5)]
CASES = [(S, B, 19) for S, B in SHAPES] + [(S, B, T) for S, B in ((65, 67), (1024, 5)) for T in (1, 64)]
GUARD = 64
I32_NAN = int(np.array([np.nan], dtype=np.float32).view(np.int32)[0])


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.array(a, dtype=dtype)).cuda()       # a copy: the shared inputs are read-only


def _taus(T):
    return np.array([0.5]) if T == 1 else np.linspace(0.05, 0.95, T)


@functools.lru_cache(maxsize=None)
def _inputs(S, B):
    """Softmaxes of N(0,1) logits, Bernoulli(0.15) labels; planted: no relevant document, only relevant documents, an all-zero
    v row, a row with a NaN.  Read-only, shared by the tests."""
    rng = np.random.default_rng(1000 * S + B)
    logits = rng.normal(0.0, 1.0, size=(B, S)).astype(np.float32)
    p = np.exp(logits - logits.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    y = (rng.random((B, S)) < 0.15).astype(np.float32)
    y[0] = 0.0
    if B > 1:
        y[1] = 1.0
    if B > 2:
        p[2] = 0.0
    if B > 3:
        p[3, S // 2] = np.nan
    # descending scores with exact duplicates (quantised to quarters), and a stop probability
    score = -np.sort(-np.round(rng.normal(3.0, 2.5, size=(B, S)) * 4) / 4, axis=1).astype(np.float32)
    stop = rng.random((B, S)).astype(np.float32)
    for a in (p, y, score, stop):
        a.setflags(write=False)
    return p, y, score, stop


def _score_taus(score, T):
    """T thresholds for FIRST_BELOW: one above every score (k = 0), one below every score (k = S), a duplicated value."""
    vals, counts = np.unique(score, return_counts=True)
    dup = float(vals[np.argmax(counts)])
    th = np.linspace(float(score.min()), float(score.max()), T)
    th[0], th[-1] = float(score.max()) + 1.0, float(score.min()) - 1.0
    if T > 2:
        th[T // 2] = dup
    return th


@functools.lru_cache(maxsize=None)
def _reference_k(S, B, T, rule):
    p, _y, score, stop = _inputs(S, B)
    if rule == W.QUANTILE:
        v, taus = p, _taus(T)
    elif rule == W.FIRST_BELOW:
        v, taus = score, _score_taus(score, T)
    else:
        v, taus = stop, _taus(T)
    k = W.cuts(v, taus, rule)
    near = np.zeros(k.shape, dtype=bool)
    if rule == W.QUANTILE:
        C = W.prefix(v)
        with np.errstate(invalid="ignore"):
            near = W.near_ties(v, taus) & (C[:, -1:] > 0)
    k.setflags(write=False)
    return v, taus, k, near


def _raw(v, stride, rule, taus, y, B, S, penalty=-1.0, beta=1.0, curve_in=None, want_k=True):
    """rlt_cut_sweep through the raw ABI with NaN sentinels in and around k and the curve; asserts that nothing outside the outputs
    was written.  Returns (k (B,T) int32 numpy or None, curve (8,T) float64 numpy or None)."""
    from rlt_hip import native as N, ops
    T = len(taus)
    thr = _t(taus, np.float64)
    kbuf = torch.full((GUARD + B * T + GUARD,), float("nan"), dtype=torch.float32, device="cuda").view(torch.int32) if want_k else None
    cbuf = None
    if y is not None:
        cbuf = torch.full((GUARD + 8 * T + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        if curve_in is not None:
            cbuf[GUARD:GUARD + 8 * T] = torch.as_tensor(curve_in).reshape(-1).cuda()
    ws_bytes = N.query("rlt_cut_sweep_workspace", B, S, T) if y is not None else 0
    ws = torch.full((ws_bytes // 8 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    N.call("rlt_cut_sweep", N.ptr(v), stride, rule, N.ptr(thr), T, N.ptr(y), B, S, float(penalty), float(beta),
           N.ptr(ops.dcg_table(v.device)) if y is not None else None, int(curve_in is not None),
           N.ptr(kbuf[GUARD:]) if want_k else None, N.ptr(cbuf[GUARD:]) if cbuf is not None else None,
           N.ptr(ws) if y is not None else None, ws_bytes, N.stream())
    torch.cuda.synchronize()
    k = curve = None
    if want_k:
        kh = kbuf.cpu().numpy()
        assert np.all(kh[:GUARD] == I32_NAN) and np.all(kh[GUARD + B * T:] == I32_NAN)
        k = kh[GUARD:GUARD + B * T].reshape(B, T).copy()
        assert k.min() >= 0 and k.max() <= S
    if cbuf is not None:
        ch = cbuf.cpu().numpy()
        assert np.all(np.isnan(ch[:GUARD])) and np.all(np.isnan(ch[GUARD + 8 * T:]))
        curve = ch[GUARD:GUARD + 8 * T].reshape(8, T).copy()
        assert np.all(np.isfinite(curve))
        assert np.all(np.isnan(ws.cpu().numpy()[ws_bytes // 8:]))
    return k, curve


def _check_curve(curve, y, k, S, B, penalty=-1.0, beta=1.0, label=""):
    """Checks 2, 4 and 5 against the restatement evaluated at the same k."""
    ref = W.curve(y, k, penalty, beta)
    for row in (0, 6, 7):
        assert np.array_equal(curve[row], ref[row]), (label, row)
    pl = W.per_list(y, k, penalty, beta)
    for row, name in ((1, "f1"), (3, "precision"), (4, "recall"), (5, "fbeta")):
        scale = np.abs(pl[name]).sum(axis=0)
        err = np.abs(curve[row] - ref[row])
        print(label, name, "max err / (2^-52 sum|value|):", float((err / np.where(scale > 0, scale, 1)).max() * 2.0 ** 52), "bound", B)
        assert np.all(err <= B * 2.0 ** -52 * scale), (label, name)
    scale = W.dcg_abs_terms(y, k, penalty)
    err = np.abs(curve[2] - ref[2])
    print(label, "dcg max err / (2^-52 sum|term|):", float((err / np.where(scale > 0, scale, 1)).max() * 2.0 ** 52), "bound", S + B)
    assert np.all(err <= (S + B) * 2.0 ** -52 * scale), (label, "dcg")


@pytest.mark.parametrize("S,B,T", CASES)
def test_quantile_against_the_restatement(S, B, T):
    _p, y, _score, _stop = _inputs(S, B)
    v, taus, k_ref, near = _reference_k(S, B, T, W.QUANTILE)
    vt, yt = _t(v), _t(y)
    k, curve = _raw(vt, 1, W.QUANTILE, taus, yt, B, S)
    assert near.sum() <= 0.001 * near.size, (int(near.sum()), near.size)      # check 1: a condition, not a measurement
    assert np.array_equal(k[~near], k_ref[~near])
    assert np.all(k >= 1)
    if B > 2:
        assert np.all(k[2] == 1)                            # the all-zero row
    if B > 3:
        assert np.all(k[3] == 1)                            # the row with a NaN: its total is NaN
    _check_curve(curve, y, k, S, B, label=f"S{S} B{B} T{T}")
    # check 7: determinism
    k2, curve2 = _raw(vt, 1, W.QUANTILE, taus, yt, B, S)
    assert np.array_equal(k, k2) and np.array_equal(curve.view(np.int64), curve2.view(np.int64))
    # check 9: label-free mode, and labels with only the cuts asked for
    k3, none = _raw(vt, 1, W.QUANTILE, taus, None, B, S)
    assert none is None and np.array_equal(k, k3)
    # only the curve
    none, curve3 = _raw(vt, 1, W.QUANTILE, taus, yt, B, S, want_k=False)
    assert none is None and np.array_equal(curve.view(np.int64), curve3.view(np.int64))
    # check 8: the class-0 column of a (B,S,2) array at stride 2
    v2 = np.stack([v, np.full_like(v, 7.0)], axis=2)
    k4, curve4 = _raw(_t(v2), 2, W.QUANTILE, taus, yt, B, S)
    assert np.array_equal(k, k4) and np.array_equal(curve.view(np.int64), curve4.view(np.int64))
    # check 6: two batches accumulated against the one call over their concatenation
    if B >= 2:
        h = B // 3 + 1
        _k, part = _raw(_t(v[:h]), 1, W.QUANTILE, taus, _t(y[:h]), h, S)
        _k, both = _raw(_t(v[h:]), 1, W.QUANTILE, taus, _t(y[h:]), B - h, S, curve_in=part)
        for row in (0, 6, 7):
            assert np.array_equal(both[row], curve[row]), row
        _check_curve(both, y, k, S, B, label=f"S{S} B{B} T{T} accumulated")
    # another penalty and beta
    if T == 19:
        k5, curve5 = _raw(vt, 1, W.QUANTILE, taus, yt, B, S, penalty=-0.25, beta=2.0)
        assert np.array_equal(k, k5)
        _check_curve(curve5, y, k, S, B, penalty=-0.25, beta=2.0, label=f"S{S} B{B} T{T} penalty -0.25 beta 2")


@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("rule", [W.FIRST_BELOW, W.FIRST_ABOVE], ids=["first_below", "first_above"])
def test_first_rules_against_the_restatement(rule, S, B):
    _p, y, _score, _stop = _inputs(S, B)
    v, taus, k_ref, _near = _reference_k(S, B, 19, rule)
    k, curve = _raw(_t(v), 1, rule, taus, _t(y), B, S)
    assert np.array_equal(k, k_ref)                         # no exclusions
    if rule == W.FIRST_BELOW:
        assert np.all(k[:, 0] == 0) and np.all(k[:, -1] == S)       # above every score, below every score
        assert np.all(curve[:7, 0] == 0.0) and curve[7, 0] == B     # k = 0: every metric is 0
        assert curve[6, -1] == B
    else:
        assert np.all(k >= 1)
    _check_curve(curve, y, k, S, B, label=f"rule {rule} S{S} B{B}")
    k2, _none = _raw(_t(v), 1, rule, taus, None, B, S)
    assert np.array_equal(k, k2)


def test_nan_values_and_thresholds_compare_false():
    v = np.array([[0.9, np.nan, 0.8, 0.1]], dtype=np.float32)
    y = np.array([[1, 0, 1, 0]], dtype=np.float32)
    taus = np.array([0.5, np.nan, 0.05])
    for rule in (W.QUANTILE, W.FIRST_BELOW, W.FIRST_ABOVE):
        k, _c = _raw(_t(v), 1, rule, taus, _t(y), 1, 4)
        assert np.array_equal(k, W.cuts(v, taus, rule)), rule
    k, _c = _raw(_t(v), 1, W.FIRST_BELOW, taus, _t(y), 1, 4)
    assert k.tolist() == [[1, 0, 1]]
    k, _c = _raw(_t(v), 1, W.FIRST_ABOVE, taus, _t(y), 1, 4)
    assert k.tolist() == [[1, 4, 1]]


@pytest.mark.parametrize("S,B", [(300, 1), (65, 67)])
def test_f1_per_list_is_bit_equal_to_cut_metrics(S, B):
    """Check 3: a B = 1 call's curve row 1 IS the list's F1; per list of the B = 67 shape, B = 1 calls on its rows."""
    from rlt_hip import ops
    S0, B0, rows = (300, 67, slice(5, 6)) if B == 1 else (S, B, slice(0, B))
    p, y, score, _stop = _inputs(S0, B0)
    y = y[rows]
    for rule, v, taus in ((W.QUANTILE, p[rows], _taus(19)), (W.FIRST_BELOW, score[rows], _score_taus(score, 19))):
        yt = _t(y)
        k, _c = _raw(_t(v), 1, rule, taus, yt, B, S)
        f1 = np.stack([_raw(_t(v[b:b + 1]), 1, rule, taus, _t(y[b:b + 1]), 1, S)[1][1] for b in range(B)])       # (B,T)
        cols = [t for t in range(len(taus)) if np.all(k[:, t] >= 1)]
        assert len(cols) == 19 if rule == W.QUANTILE else len(cols) >= 1
        for t in cols:
            _k, ref, _d, _s = ops.cut_metrics(None, yt, k_in=_t(k[:, t], np.int32))
            torch.cuda.synchronize()
            assert np.array_equal(f1[:, t].view(np.int64), ref.cpu().numpy().view(np.int64)), (rule, t)


def test_ops_and_cutsweep_match_the_raw_call():
    from rlt_hip import ops
    from utils.sweep import CutSweep
    S, B, T = 300, 67, 19
    p, y, _score, stop = _inputs(S, B)
    taus = _taus(T)
    k_raw, c_raw = _raw(_t(p), 1, W.QUANTILE, taus, _t(y), B, S)
    k, c = ops.cut_sweep(_t(p).reshape(B, S, 1), _t(taus, np.float64), "quantile", _t(y))
    assert k.dtype == torch.int32 and c.dtype == torch.float64 and tuple(k.shape) == (B, T) and tuple(c.shape) == (8, T)
    assert np.array_equal(k.cpu().numpy(), k_raw) and np.array_equal(c.cpu().numpy().view(np.int64), c_raw.view(np.int64))
    k_free, none = ops.cut_sweep(_t(p), _t(taus, np.float64), "quantile")
    assert none is None and np.array_equal(k_free.cpu().numpy(), k_raw)
    # streaming in three ragged batches; BiCut-shaped values at stride 2
    pair = np.stack([stop, 1.0 - stop], axis=2).astype(np.float32)
    k_above, c_above = _raw(_t(stop), 1, W.FIRST_ABOVE, taus, _t(y), B, S)
    sw = CutSweep(S, "above", taus)
    for lo, hi in ((0, 30), (30, 31), (31, B)):
        sw.update(_t(pair[lo:hi]), _t(y[lo:hi]))
    sw.update(_t(pair[:0]), _t(y[:0]))
    assert sw.n_lists == B
    sums = sw.sums()
    for row in (0, 6, 7):
        assert np.array_equal(sums[row], c_above[row])
    _check_curve(sums, y, k_above, S, B, label="CutSweep above")
    cv = sw.curve()
    assert np.array_equal(cv["k"], c_above[0] / B) and np.array_equal(cv["thresholds"], taus) and cv["n"] == B
    tau, i, val = sw.best("f1")
    assert i == int(np.argmax(cv["f1"])) and tau == taus[i] and val == cv["f1"][i]
    at = sw.at(taus[4])
    assert at["index"] == 4 and at["dcg"] == cv["dcg"][4] and at["uncut"] == cv["uncut"][4]
    with pytest.raises(ValueError):
        sw.at(0.123)
    with pytest.raises(ValueError):
        ops.cut_sweep(_t(p), _t(taus, np.float64), "quantile", None, curve=c)


def test_truncate_with_and_without_a_rule():
    """Check 10: the default truncate is what it was (rlt_cut_report's k and p_k); with a rule it is the sweep's k on the model's
    own output."""
    from models import AttnCut
    from rlt_hip import ops
    torch.manual_seed(5)
    B, S = 5, 40
    x = torch.randn(B, S, 3, device="cuda")
    model = AttnCut(input_size=3).cuda().train()
    k, p_k = model.truncate(x)
    assert model.training
    model.eval()
    with torch.no_grad():
        out = model(x)
    per, _ = ops.cut_report(out)
    p = out.reshape(B, S).cpu().numpy()
    assert torch.equal(k, per["k"]) and torch.equal(p_k, per["p_k"])
    assert np.array_equal(k.cpu().numpy(), np.argmax(p, axis=1) + 1)
    assert np.array_equal(p_k.cpu().numpy(), p.max(axis=1))
    model.train()
    kq = model.truncate(x, rule="quantile", tau=0.5)
    assert model.training and kq.dtype == torch.int32 and tuple(kq.shape) == (B,)
    k_sweep, _ = ops.cut_sweep(out, torch.tensor([0.5], dtype=torch.float64, device="cuda"), "quantile")
    assert torch.equal(kq, k_sweep.reshape(-1))
    ref = W.cuts(p, [0.5], W.QUANTILE)[:, 0]
    near = W.near_ties(p, [0.5])[:, 0]
    assert np.array_equal(kq.cpu().numpy()[~near], ref[~near]) and near.sum() == 0
    with pytest.raises(ValueError):
        model.truncate(x, rule="quantile")
    with pytest.raises(TypeError):
        model.truncate(x, "quantile", 0.5)                  # keyword-only


def _synthetic_scores(tmp_path):
    from dataloader.synth import write_synthetic_robust04
    root = write_synthetic_robust04(str(tmp_path), "robust04", "bm25", n_train=23, n_test=11, seq_len=100, seed=7)
    gt = pickle.load(open(os.path.join(root, "gt.pkl"), "rb"))
    out = []
    for split in ("train", "test"):
        raw = pickle.load(open(os.path.join(root, f"bm25_{split}.pkl"), "rb"))
        scores = np.array([list(raw[q].values()) for q in raw], dtype=np.float32)
        labels = np.array([[1.0 if d in set(gt[q]) else 0.0 for d in raw[q]] for q in raw], dtype=np.float32)
        out += [scores, labels]
    return out


def test_tuning_on_a_synthetic_set(tmp_path):
    """Check 11: tune_cut_rule and score_threshold against the restatement run on the host."""
    from utils.baselines import score_threshold
    from utils.sweep import score_quantiles, tune_cut_rule
    s_tr, y_tr, s_te, y_te = _synthetic_scores(tmp_path)
    taus = score_quantiles(s_tr, 15)
    ref = {}
    for name, s, y in (("train", s_tr, y_tr), ("test", s_te, y_te)):
        ref[name] = W.curve(y, W.cuts(s, taus, W.FIRST_BELOW)) / len(y)
    # the host's choice is not a near-tie between two thresholds: the device's rounding cannot move it
    for row in (1, 2):
        top = np.sort(ref["train"][row])[::-1]
        assert top[0] - top[1] > 1e-9
    i_f1, i_dcg = int(np.argmax(ref["train"][1])), int(np.argmax(ref["train"][2]))
    f1, dcg, th_f1, th_dcg = score_threshold(s_tr, y_tr, s_te, y_te, taus)
    assert (th_f1, th_dcg) == (taus[i_f1], taus[i_dcg])
    assert abs(f1 - ref["test"][1][i_f1]) <= 1e-13 and abs(dcg - ref["test"][2][i_dcg]) <= 1e-12
    batches = lambda s, y: [(_t(s[i:i + 5]), _t(y[i:i + 5])) for i in range(0, len(y), 5)]
    res = tune_cut_rule(batches(s_tr, y_tr), batches(s_te, y_te), "score", taus, metric="dcg")
    assert res["index"] == i_dcg and res["tau"] == taus[i_dcg]
    assert abs(res["test"]["dcg"] - ref["test"][2][i_dcg]) <= 1e-12 and abs(res["train"]["dcg"] - ref["train"][2][i_dcg]) <= 1e-12
    assert np.allclose(res["test_curve"]["k"], ref["test"][0], rtol=0, atol=0)
    assert np.allclose(res["test_curve"]["recall"], ref["test"][4], rtol=1e-13, atol=1e-15)
