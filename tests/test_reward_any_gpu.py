"""rlt_reward_spec_matrix and rlt_reward_any_loss on the device against the float64 restatement (tests/reward_any_restate.py), at
the edges of the layouts rather than at the workload: S over the lists-per-wavefront forms and their round counts, B over the
tails of the groups and of the grid stride, both reward sources, the four kinds, dp given and NULL.

The bound on the loss and on dp is not a constant: each test measures, at its own B, S, p, kind and tau, how far the EXISTING
rlt_reward_loss_ex is from tests/loss_restate.py for the F1 and the DCG reward (distance = max abs as a fraction of the array's
largest magnitude) and grants the new entry point 4 times the larger of the two, with a floor of S * 2^-24 - the factor the
report test grants.  The measured figures are printed (run with -s) and tabulated in DESIGN.md section 7."""
import os

import numpy as np
import pytest
import torch

import loss_restate as L
import reward_any_restate as R

pytestmark = pytest.mark.gpu

S_EDGES = [1, 3, 4, 63, 64, 65, 128, 129, 192, 300, 321, 1024]
B_EDGES = [1, 2, 3, 5, 67]
TAU = {R.EXPECT: 1.0, R.CE: 0.95, R.KL: 1.0, R.JS: 0.85}
KIND_NAMES = {R.EXPECT: "expect", R.CE: "ce", R.KL: "kl", R.JS: "js"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from rlt_hip import native
    native.load()
    return native


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _guarded(n, dtype=torch.float32, pad=16):
    """An output of n elements followed by `pad` sentinels (NaN, or -7 for integers)."""
    t = torch.full((n + pad,), float("nan") if dtype.is_floating_point else -7, dtype=dtype, device="cuda")
    return t


def _intact(t, n):
    tail = t[n:]
    return bool(torch.isnan(tail).all()) if t.dtype.is_floating_point else bool((tail == -7).all())


def _pair(kind, *a, **kw):
    """(the library's RewardSpec, the restatement's Spec) of one reward."""
    from utils.rewards import RewardSpec
    return getattr(RewardSpec, kind)(*a, **kw), getattr(R, kind)(*a, **kw)


def _labels(B, S, seed, grades=3):
    rng = np.random.default_rng(seed)
    y = ((rng.random((B, S)) < 0.35) * rng.integers(1, grades, (B, S))).astype(np.float32)
    if B > 1:
        y[1] = 0.0                                  # no relevant document: F_beta 0 everywhere, ideal 0
    if B > 2:
        y[2] = grades - 1
    return y


def _p(B, S, seed):
    """Strictly positive fp32 rows (a softmax over S + 1 logits with the last dropped), with exact ties at the maximum."""
    rng = np.random.default_rng(seed)
    e = np.exp(rng.normal(size=(B, S + 1)) * 1.5)
    p = (e / e.sum(1, keepdims=True))[:, :S].astype(np.float32)
    for b in range(0, B, 2):                        # every other row: the maximum again at later positions
        j = int(np.argmax(p[b]))
        p[b, j::max(1, S // 5)] = p[b, j]
    if B > 3:
        p[3] = p[3, 0]                              # all equal: k = 1
    return p


def spec_matrix(labels, spec, tau=1.0, want_q=True):
    from rlt_hip import ops
    out = ops.reward_spec_matrix(_dev(labels), spec, tau, want_q)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) if want_q else out.cpu().numpy()


def any_loss(lib, p, kind, tau, labels=None, spec=None, r=None, want_dp=True, want=("per", "loss", "k", "r_k", "r_best", "best_k", "sums")):
    """One call of rlt_reward_any_loss on guarded outputs -> dict of numpy results (None where the output was NULL) and
    `intact`: every sentinel behind every output is untouched."""
    from rlt_hip import ops
    N = lib
    B, S = p.shape
    pt = _dev(p)
    yt = None if labels is None else _dev(labels)
    rt = None if r is None else _dev(r)
    struct = keep = table = None
    if spec is not None:
        struct, keep = spec.native(S, pt.device)
        table = ops.dcg_table(pt.device) if struct.family == N.REWARD_GAIN and struct.discount is None else None
    sizes = {"per": (B, torch.float32), "loss": (1, torch.float32), "k": (B, torch.int32), "r_k": (B, torch.float32),
             "r_best": (B, torch.float32), "best_k": (B, torch.int32), "sums": (4, torch.float64), "dp": (B * S, torch.float32)}
    bufs = {name: (_guarded(*sizes[name]) if (name in want or (name == "dp" and want_dp)) else None) for name in sizes}
    ws_bytes = N.query("rlt_reward_any_workspace", B)
    ws = N.workspace(ws_bytes, pt.device)
    g = lambda name: N.ptr(bufs[name])
    N.call("rlt_reward_any_loss", N.ptr(pt), N.ptr(yt), None if struct is None else N.ctypes.byref(struct), N.ptr(rt), B, S, kind,
           float(tau), g("per"), g("loss"), g("dp"), g("k"), g("r_k"), g("r_best"), g("best_k"), g("sums"), N.ptr(table), N.ptr(ws),
           ws_bytes, N.stream())
    torch.cuda.synchronize()
    out = {"intact": all(_intact(t, sizes[n][0]) for n, t in bufs.items() if t is not None)}
    for n, t in bufs.items():
        out[n] = None if t is None else t[:sizes[n][0]].cpu().numpy()
    if out["dp"] is not None:
        out["dp"] = out["dp"].reshape(B, S)
    if out["loss"] is not None:
        out["loss"] = out["loss"][0]
    return out


def parent_loss(lib, p, y, metric, kind, tau):
    """The existing rlt_reward_loss_ex (F1 / DCG reward, penalty -1): (per_list, loss, dp)."""
    from rlt_hip import ops
    N = lib
    B, S = p.shape
    pt, yt = _dev(p), _dev(y)
    coef = ops.dcg_coef(S, pt.device) if metric == N.METRIC_DCG else None
    per, loss, dp = torch.empty(B, device="cuda"), torch.empty(1, device="cuda"), torch.empty(B, S, device="cuda")
    N.call("rlt_reward_loss_ex", N.ptr(pt), N.ptr(yt), N.ptr(coef), B, S, metric, -1.0, kind, float(tau), N.ptr(per), N.ptr(loss),
           N.ptr(dp), N.stream())
    torch.cuda.synchronize()
    return per.cpu().numpy(), loss.cpu().numpy()[0], dp.cpu().numpy()


def yardstick(lib, p, y01, kind, tau):
    """{'loss', 'per', 'dp'}: the larger of the F1 and the DCG distance of the existing entry point from loss_restate."""
    out = {"loss": 0.0, "per": 0.0, "dp": 0.0}
    for name, code in (("f1", lib.METRIC_F1), ("dcg", lib.METRIC_DCG)):
        per, loss, dp = parent_loss(lib, p, y01, code, kind, tau)
        rper, rloss, rdp, _r, _q = L.reward_loss(p, y01, name, kind, tau)
        out["loss"] = max(out["loss"], R.distance(loss, rloss))
        out["per"] = max(out["per"], R.distance(per, rper))
        out["dp"] = max(out["dp"], R.distance(dp, rdp))
    return out


def bound_of(yard, S):
    return {k: max(4.0 * v, S * 2.0 ** -24) for k, v in yard.items()}


def _ulps(a, b):
    """Distance in fp32 units in the last place between two finite fp32 arrays."""
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- exact operands: zero tolerance ----------------------------------------------------------------------------------------
def _exact_case(B, S, seed):
    """Integer gains, power-of-two discounts, 3 grades: every sum is exact in float64 and in fp32, so the reward has ONE value.
    Gain 0 for grade 1 makes runs of equal rewards: rows are built to tie at their maximum."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, (B, S)).astype(np.float32)
    lead = min(S, 2)
    y[0, :lead] = 2.0                               # row 0: the best reward after `lead` documents, tied along a run of grade 1
    y[0, lead:] = 0.0
    y[0, lead:lead + max(1, S // 3)] = 1.0
    if B > 1:
        y[1] = 1.0                                  # all rewards equal (0): best_k = 1
    disc = (2.0 ** -(np.arange(S) % 7)).astype(np.float32)
    return y, disc


@pytest.mark.parametrize("S", S_EDGES)
def test_exact_operands_bit_for_bit(lib, S):
    for B in B_EDGES:
        y, disc = _exact_case(B, S, 100 * S + B)
        spec, want = _pair("gain", (-1.0, 0.0, 2.0), discount=disc)
        p = _p(B, S, S + B)
        r64 = R.reward64(y, want)
        ref = R.loss(p, r64.astype(np.float32), R.JS, 0.85)
        assert np.array_equal(r64, r64.astype(np.float32).astype(np.float64))          # exact operands indeed
        r, _q = spec_matrix(y, spec, 0.85)
        assert np.array_equal(r.view(np.int32), r64.astype(np.float32).view(np.int32)), (B, S)
        for source in ("spec", "matrix"):
            kw = dict(labels=y, spec=spec) if source == "spec" else dict(r=r)
            got = any_loss(lib, p, R.JS, 0.85, **kw)
            assert got["intact"]
            assert np.array_equal(got["k"], ref["k"]), (B, S, source)
            assert np.array_equal(got["best_k"], ref["best_k"]), (B, S, source)
            assert np.array_equal(got["r_k"].view(np.int32), ref["r_k"].astype(np.float32).view(np.int32)), (B, S, source)
            assert np.array_equal(got["r_best"].view(np.int32), ref["r_best"].astype(np.float32).view(np.int32)), (B, S, source)
            assert got["sums"][2] == ref["sums"][2] and got["sums"][3] == B, (B, S, source)
            assert got["sums"][0] == ref["sums"][0] and got["sums"][1] == ref["sums"][1], (B, S, source)   # exact sums too


# ---- rounded rewards: one fp32 ulp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_EDGES)
def test_rounded_rewards_within_one_ulp(lib, S):
    pairs = [_pair("fbeta", 0.5), _pair("fbeta", 1.0), _pair("fbeta", 2.0), _pair("ndcg"), _pair("ndcg", -0.5),
             _pair("gain", (-1.0, 1.0, 3.0), normalize=True), _pair("gain", (-1.0, 1.0, 3.0)),
             _pair("gain", (0.0, 2.0, 2.0, -1.0, 5.0, 0.5, 0.25, 1.0), normalize=True)]
    for B in B_EDGES:
        y = _labels(B, S, 7 * S + B)
        y8 = np.random.default_rng(S + B).integers(0, 9, (B, S)).astype(np.float32) - 0.4     # grades by rounding and clamping
        for i, (spec, want) in enumerate(pairs):
            labels = y8 if i == len(pairs) - 1 else y
            r, q = spec_matrix(labels, spec, 0.95)
            ref = R.reward(labels, want)
            assert np.isfinite(r).all()
            assert _ulps(r, ref).max() <= 1, (B, S, str(want.family), i, int(_ulps(r, ref).max()))
            if B > 1 and i < 6:
                assert np.all(r[1] == 0.0)          # the all-zero-label list: F_beta 0; normalised gain: ideal 0
            qref = R.distribution(r, 0.95)          # q of the reward the device formed
            assert R.distance(q, qref) <= 2.0 ** -23, (B, S, i)


# ---- loss and dp against the restatement, bound measured on the existing entry point ----------------------------------------------
def _loss_cases(S):
    return [("fbeta:2", _pair("fbeta", 2.0)), ("ndcg", _pair("ndcg")), ("gain:-1,1,3", _pair("gain", (-1.0, 1.0, 3.0)))]


@pytest.mark.parametrize("S", S_EDGES)
def test_loss_and_dp_against_restatement(lib, S):
    rows = []
    for B in B_EDGES:
        y = _labels(B, S, 11 * S + B)
        y01 = np.minimum(y, 1.0)
        p = _p(B, S, 13 * S + B)
        for kind in R.KINDS:
            tau = TAU[kind]
            yard = yardstick(lib, p, y01, kind, tau)
            bound = bound_of(yard, S)
            worst = {"loss": 0.0, "per": 0.0, "dp": 0.0, "src": 0.0}
            for name, (spec, want) in _loss_cases(S):
                ref = R.spec_loss(p, y, want, kind, tau)
                r_dev = spec_matrix(y, spec, tau, want_q=False)
                ref_r = R.reward(y, want)
                assert _ulps(r_dev, ref_r).max() <= 1
                got_s = any_loss(lib, p, kind, tau, labels=y, spec=spec)
                got_m = any_loss(lib, p, kind, tau, r=r_dev)
                got_n = any_loss(lib, p, kind, tau, labels=y, spec=spec, want_dp=False)
                # the restatement works from the fp32 reward the device formed (equal to its own but for a last-bit tie)
                ref = R.loss(p, r_dev, kind, tau) if not np.array_equal(r_dev, ref_r) else ref
                for got in (got_s, got_m):
                    assert got["intact"]
                    d = {"loss": R.distance(got["loss"], ref["loss"]), "per": R.distance(got["per"], ref["per_list"]),
                         "dp": R.distance(got["dp"], ref["dp"])}
                    for k in d:
                        worst[k] = max(worst[k], d[k])
                        assert d[k] <= bound[k], (B, S, KIND_NAMES[kind], name, k, d[k], bound[k], yard[k])
                    assert np.array_equal(got["k"], ref["k"]) and np.array_equal(got["best_k"], ref["best_k"])
                    assert np.array_equal(got["r_k"], ref["r_k"].astype(np.float32))
                    assert np.array_equal(got["r_best"], ref["r_best"].astype(np.float32))
                    assert got["sums"][2] == ref["sums"][2] and got["sums"][3] == B
                    assert abs(got["sums"][0] - ref["sums"][0]) <= 1e-12 * max(1.0, abs(ref["sums"][0]))
                    assert abs(got["sums"][1] - ref["sums"][1]) <= 1e-12 * max(1.0, abs(ref["sums"][1]))
                # the two sources agree within the same bound; cuts and counts are identical
                src = max(R.distance(got_s["loss"], got_m["loss"]), R.distance(got_s["per"], got_m["per"]), R.distance(got_s["dp"], got_m["dp"]))
                worst["src"] = max(worst["src"], src)
                assert R.distance(got_s["loss"], got_m["loss"]) <= bound["loss"]
                assert R.distance(got_s["per"], got_m["per"]) <= bound["per"]
                assert R.distance(got_s["dp"], got_m["dp"]) <= bound["dp"]
                assert np.array_equal(got_s["k"], got_m["k"]) and np.array_equal(got_s["best_k"], got_m["best_k"])
                assert got_s["sums"][2] == got_m["sums"][2]
                # dp NULL: the same loss, bit for bit, and nothing written where dp would be
                assert got_n["intact"] and got_n["dp"] is None
                assert got_n["loss"].tobytes() == got_s["loss"].tobytes() and got_n["per"].tobytes() == got_s["per"].tobytes()
            rows.append((B, KIND_NAMES[kind], yard, worst, bound))
    print(f"\nS = {S}: distance from the float64 restatement (max abs / largest magnitude); yardstick = rlt_reward_loss_ex, F1 | DCG")
    print("   B kind   | yard loss  yard per   yard dp   | new loss   new per    new dp    | two sources | bound dp")
    for B, kn, yard, worst, bound in rows:
        print(f"{B:4d} {kn:6s} | {yard['loss']:.2e}  {yard['per']:.2e}  {yard['dp']:.2e}  | {worst['loss']:.2e}  {worst['per']:.2e}  "
              f"{worst['dp']:.2e}  | {worst['src']:.2e}    | {bound['dp']:.2e}")


# ---- write extents, NULL outputs, determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 64, 300, 321])
def test_write_extents_and_null_outputs(lib, S):
    spec, _ = _pair("ndcg")
    for B in (1, 5, 67):
        y, p = _labels(B, S, S + B), _p(B, S, S - B + 500)
        full = any_loss(lib, p, R.KL, 1.0, labels=y, spec=spec)
        assert full["intact"]
        for leave in ("per", "loss", "k", "r_k", "r_best", "best_k", "sums"):
            want = tuple(n for n in ("per", "loss", "k", "r_k", "r_best", "best_k", "sums") if n != leave)
            got = any_loss(lib, p, R.KL, 1.0, labels=y, spec=spec, want=want)
            assert got["intact"] and got[leave] is None
            for n in want + ("dp",):
                assert np.asarray(got[n]).tobytes() == np.asarray(full[n]).tobytes(), (B, S, leave, n)
        none = any_loss(lib, p, R.KL, 1.0, labels=y, spec=spec, want=("loss",), want_dp=False)
        assert none["intact"] and none["loss"].tobytes() == full["loss"].tobytes()
        # the matrices: guarded r and q, either alone
        N = lib
        from rlt_hip import ops
        yt = _dev(y)
        struct, keep = spec.native(S, yt.device)
        for want_r, want_q in ((True, True), (True, False), (False, True)):
            r, q = (_guarded(B * S) if want_r else None), (_guarded(B * S) if want_q else None)
            N.call("rlt_reward_spec_matrix", N.ptr(yt), B, S, N.ctypes.byref(struct), 1.0, N.ptr(ops.dcg_table(yt.device)), N.ptr(r),
                   N.ptr(q), N.stream())
            torch.cuda.synchronize()
            for t in (r, q):
                assert t is None or (_intact(t, B * S) and bool(torch.isfinite(t[:B * S]).all()))


@pytest.mark.parametrize("S", [4, 65, 300, 1024])
def test_two_calls_are_bit_identical(lib, S):
    B = 67
    y, p = _labels(B, S, S), _p(B, S, S + 1)
    for spec in (_pair("fbeta", 2.0)[0], _pair("gain", (-1.0, 1.0, 3.0), normalize=True)[0]):
        for kind in R.KINDS:
            a = any_loss(lib, p, kind, TAU[kind], labels=y, spec=spec)
            b = any_loss(lib, p, kind, TAU[kind], labels=y, spec=spec)
            for n in ("per", "loss", "dp", "k", "r_k", "r_best", "best_k", "sums"):
                assert np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes(), (S, kind, n)


# ---- through the classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["choopy_b6_s40", "choopy_b5_s300"])
def test_divloss_fbeta_one_is_divloss_f1(lib, fixture):
    """DivLoss(metric=RewardSpec.fbeta(1.0)) against DivLoss(metric='f1') on the same p and labels: loss and input gradient."""
    from utils import losses
    from utils.rewards import RewardSpec
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    p, y = z["out0"].astype(np.float32), z["y"].astype(np.float32)
    B, S = y.shape
    assert (p > 0).all()
    for div_type, kind in (("js", R.JS), ("kl", R.KL)):
        bound = bound_of(yardstick(lib, p, y, kind, 0.85), S)
        res = []
        for metric in ("f1", RewardSpec.fbeta(1.0), "fbeta:1"):
            pt = _dev(p).reshape(B, S, 1).requires_grad_(True)
            loss = losses.DivLoss(metric=metric, div_type=div_type, augmented=True)(pt, _dev(y))
            loss.backward()
            torch.cuda.synchronize()
            res.append((loss.item(), pt.grad.cpu().numpy().reshape(B, S)))
        for loss, grad in res[1:]:
            d_loss, d_grad = R.distance(loss, res[0][0]), R.distance(grad, res[0][1])
            print(f"\n{fixture} {div_type}: |loss| {d_loss:.2e} (bound {bound['loss']:.2e})  |grad| {d_grad:.2e} (bound {bound['dp']:.2e})")
            assert d_loss <= bound["loss"] and d_grad <= bound["dp"]
        assert res[1][0] == res[2][0] and np.array_equal(res[1][1], res[2][1])      # the string and the object are one reward


def test_classes_accept_a_spec_and_report_reward_statistics(lib):
    from utils import losses
    from utils.metrics import Metric
    from utils.rewards import RewardSpec
    z = np.load(os.path.join(GOLDEN, "choopy_b6_s40.npz"))
    p, y = z["out0"].astype(np.float32), z["y"].astype(np.float32)
    B, S = y.shape
    for crit, kind, tau in ((losses.ChoopyLoss(metric="fbeta:2"), R.EXPECT, 1.0), (losses.AttnCutLoss(metric=RewardSpec.ndcg()), R.CE, 0.95),
                            (losses.DivLoss(metric="gain:-1,1,3:norm", div_type="kl"), R.KL, 0.85)):
        want = R.parse(crit.metric) if isinstance(crit.metric, str) else R.ndcg()
        ref = R.spec_loss(p, y, want, kind, tau)
        pt = _dev(p).reshape(B, S, 1)
        loss, k, f1, dcg = Metric.step(crit, pt, _dev(y))
        assert R.distance(loss.item(), ref["loss"]) <= S * 2.0 ** -24
        assert np.array_equal(k.cpu().numpy(), ref["k"])
        assert abs(float(f1) - L.f1_at(y, ref["k"]).mean()) <= 1e-12 and abs(float(dcg) - L.dcg_at(y, ref["k"]).mean()) <= 1e-12
        sums = crit.last_reward_sums.cpu().numpy()
        assert sums[2] == ref["sums"][2] and sums[3] == B and abs(sums[0] - ref["sums"][0]) <= 1e-12


# ---- one training step -----------------------------------------------------------------------------------------------------------------
def test_reward_matrix_loss_trains_one_step(lib):
    import models
    from utils import losses
    z = np.load(os.path.join(GOLDEN, "choopy_b6_s40.npz"))
    x, y = _dev(z["x"]), z["y"].astype(np.float32)
    B, S = y.shape
    torch.manual_seed(0)
    model = models.Choopy(seq_len=S, dropout=0.0).cuda()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    r = _dev(R.reward(y, R.fbeta(2.0)))             # any (B,S) matrix: here F_2 from the restatement
    crit = losses.RewardMatrixLoss(kind="js", tau=0.85)
    before = [q.detach().clone() for q in model.parameters()]
    out = model(x)
    loss, k, stats = crit.forward_with_stats(out, r)
    ref = R.loss(out.detach().cpu().numpy().reshape(B, S), r.cpu().numpy(), R.JS, 0.85)
    assert R.distance(loss.item(), ref["loss"]) <= S * 2.0 ** -24 and np.array_equal(k.cpu().numpy(), ref["k"])
    assert stats["sums"].cpu().numpy()[2] == ref["sums"][2]
    loss2 = crit(model(x), r)
    loss2.backward()
    grads = [q.grad for q in model.parameters() if q.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    assert np.isfinite(loss2.item())
