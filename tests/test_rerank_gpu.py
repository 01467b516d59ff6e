"""rlt_rerank_lists on the device against tests/rerank_restate.py (np.argsort(-v, kind="stable")), tolerance ZERO on every output:
they are integers and moved bits, so fp32 is compared as its uint32 view.  Every list length at which the dispatch changes its
packing (16, 32 or 64 lanes per list; 4, 8 or 16 keys per lane), list counts around one workgroup's lists for each packing and
past the grid cap, NaN / inf / signed zeros at the lane boundaries; then the Python layer: ops.rerank_lists, model.rerank,
utils.rerank.RerankedEval and run.py --rerank-eval."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import rerank_restate as RR

pytestmark = pytest.mark.gpu

S_EDGES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1023, 1024]
WAVES = 4                                       # wavefronts per workgroup of the kernel
GRID_CAP = 2048                                 # workgroups; more lists than they hold at once take the strided loop
I_SENT, F_SENT = 0x7fffffff, 0x7fc00123         # what the outputs hold before the call


def lists_per_wave(S):
    return 4 if S <= 64 else 2 if S <= 128 else 1


def list_counts(S):
    per_group = lists_per_wave(S) * WAVES
    return sorted({1, 3, 5, per_group - 1, per_group, per_group + 1})


@pytest.fixture(scope="module")
def lib():
    from rlt_hip import native
    native.load()
    return native


class Guarded:
    """A (B,S) 4-byte output between two guard rows, everything pre-filled with a sentinel."""

    def __init__(self, B, S, sentinel):
        self.B, self.S, self.sentinel = B, S, sentinel
        self.t = torch.full(((B + 2) * S,), sentinel, dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.S)

    def read(self):
        """-> the (B,S) int32 body; the guard rows must be untouched."""
        a = self.t.cpu().numpy()
        S, B = self.S, self.B
        assert (a[:S] == self.sentinel).all() and (a[(B + 1) * S:] == self.sentinel).all(), "a guard row was written"
        return a[S:(B + 1) * S].reshape(B, S)


def companions(B, S, n):
    """n arrays whose element [b,j] holds the int32 b * 1024 + j (+ t << 28) as its bits: a row read from a neighbouring list or
    a lost element shows."""
    base = (np.arange(B, dtype=np.int64)[:, None] * 1024 + np.arange(S)[None, :])
    return [((base + (t << 28)) & 0x7fffffff).astype(np.int32) for t in range(n)]


def call(lib, v, n=0, perm=True, rank=True, sorted_pred=True, src_np=None):
    """One call through the raw C ABI -> dict of the (B,S) int32 views of what was asked for ('perm', 'rank', 'sorted', 'dst')."""
    B, S = v.shape
    pred = torch.from_numpy(v.view(np.int32).copy()).cuda()
    src_np = companions(B, S, n) if src_np is None else src_np
    src = [torch.from_numpy(a.copy()).cuda() for a in src_np]
    dst = [Guarded(B, S, F_SENT) for _ in range(n)]
    outs = {"perm": Guarded(B, S, I_SENT) if perm else None, "rank": Guarded(B, S, I_SENT) if rank else None,
            "sorted": Guarded(B, S, F_SENT) if sorted_pred else None}
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*ps) if ps else None
    o = lambda name: outs[name].ptr if outs[name] is not None else None
    rc = lib.load().rlt_rerank_lists(ctypes.c_void_p(pred.data_ptr()), B, S, arr([t.data_ptr() for t in src]),
                                     arr([g.ptr.value for g in dst]), n, o("perm"), o("rank"), o("sorted"), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = {k: g.read() for k, g in outs.items() if g is not None}
    res["dst"] = [g.read() for g in dst]
    return res


def check(res, v, src_np):
    """Every output that is present equals the restatement bit for bit (so every element was overwritten)."""
    B, S = v.shape
    p = RR.perm(v)
    p64 = p.astype(np.int64)
    if "perm" in res:
        assert np.array_equal(res["perm"], p)
    if "rank" in res:
        assert np.array_equal(res["rank"], RR.inverse(p))
    if "perm" in res and "rank" in res:
        ar = np.tile(np.arange(S, dtype=np.int32), (B, 1))
        assert np.array_equal(np.take_along_axis(res["rank"], res["perm"].astype(np.int64), axis=1), ar)
        assert np.array_equal(np.take_along_axis(res["perm"], res["rank"].astype(np.int64), axis=1), ar)
    if "sorted" in res:
        assert np.array_equal(res["sorted"], np.take_along_axis(v.view(np.int32), p64, axis=1))
    assert len(res["dst"]) == len(src_np)
    for got, a in zip(res["dst"], src_np):
        assert np.array_equal(got, np.take_along_axis(a, p64, axis=1))


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("S", S_EDGES)
def test_order_and_moved_bits(lib, S, kind):
    for i, B in enumerate(list_counts(S)):
        v = RR.inputs(kind, B, S, seed=i)
        n = (0, 1, 4)[(i + S) % 3]
        src = companions(B, S, n)
        first = call(lib, v, n, src_np=src)
        check(first, v, src)
        if kind in ("equal", "descending", "zeros"):
            assert np.array_equal(first["perm"], np.tile(np.arange(S, dtype=np.int32), (B, 1)))
        if kind == "ascending":
            assert np.array_equal(first["perm"], np.tile(np.arange(S, dtype=np.int32)[::-1], (B, 1)))
        if i == 0:                              # two calls give the same bits
            second = call(lib, v, n, src_np=src)
            for name in ("perm", "rank", "sorted"):
                assert np.array_equal(first[name], second[name])
            assert all(np.array_equal(a, b) for a, b in zip(first["dst"], second["dst"]))


@pytest.mark.parametrize("S", [33, 100, 300])
def test_more_lists_than_the_grid_holds(lib, S):
    B = GRID_CAP * WAVES * lists_per_wave(S) + 2 * lists_per_wave(S) + 1
    v = RR.inputs("specials", B, S, seed=3)
    v[1::2] = RR.inputs("ties", B, S, seed=4)[1::2]
    src = companions(B, S, 1)
    check(call(lib, v, 1, src_np=src), v, src)


@pytest.mark.parametrize("S,B", [(65, 5), (300, 5), (16, 17)])
def test_every_null_output_combination(lib, S, B):
    v = RR.inputs("specials", B, S, seed=9)
    for n in (0, 1, 4):
        src = companions(B, S, n)
        for perm, rank, srt in itertools.product((False, True), repeat=3):
            if n == 0 and not (perm or rank or srt):
                p = ctypes.c_void_p(torch.zeros(B * S, device="cuda").data_ptr())
                assert lib.load().rlt_rerank_lists(p, B, S, None, None, 0, None, None, None, None) == -1
                continue
            res = call(lib, v, n, perm, rank, srt, src_np=src)
            assert set(res) == {"dst"} | ({"perm"} if perm else set()) | ({"rank"} if rank else set()) | ({"sorted"} if srt else set())
            check(res, v, src)


@pytest.mark.parametrize("kind", ["randn", "ties", "equal", "ascending", "zeros"])
@pytest.mark.parametrize("S", [1, 3, 64, 65, 129, 300, 1024])
def test_task_metric_dcg_on_the_reranked_labels(lib, S, kind):
    """rlt_task_metrics' dcg_out against the float64 sum over the kernel's own re-ranked labels.  NaN-free inputs: with NaNs the
    two ranks differ by design.  Both are float64 sums of the same S terms in different orders: bound S * 2^-52 * sum |term|."""
    B = 5
    v = RR.inputs(kind, B, S, seed=2)
    y = np.random.default_rng(S).integers(0, 2, (B, S)).astype(np.float32)
    res = call(lib, v, 1, src_np=[y.view(np.int32)])
    y_rr = res["dst"][0].view(np.float32)
    terms = RR.dcg_terms(y_rr)
    dcg = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    yd, vd = torch.from_numpy(y).cuda(), torch.from_numpy(v).cuda()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    auc = torch.empty_like(dcg)                 # the entry point wants both per-list outputs
    assert lib.load().rlt_task_metrics(P(yd), P(vd), B, S, P(dcg), P(auc), None, None) == 0
    got = dcg.cpu().numpy()
    bound = S * 2.0 ** -52 * np.abs(terms).sum(axis=1)
    err = np.abs(got - terms.sum(axis=1))
    print(f"S={S} {kind}: max err {err.max():.3e}, bound {bound.min():.3e}")
    assert (err <= bound).all(), (err, bound)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_ops_rerank_lists(lib):
    from rlt_hip import ops
    B, S = 6, 70
    v = RR.inputs("specials", B, S, seed=1)
    y = np.random.default_rng(0).integers(0, 2, (B, S)).astype(np.float32)
    vd, yd = torch.from_numpy(v).cuda().reshape(B, S, 1), torch.from_numpy(y).cuda()
    perm, rank, srt, (y_rr, v_rr) = ops.rerank_lists(vd, yd, vd, want_rank=True, want_sorted=True)
    p, r, sv, (yy,) = RR.rerank(v, y)
    assert perm.dtype == torch.int32 and tuple(perm.shape) == (B, S) and np.array_equal(perm.cpu().numpy(), p)
    assert np.array_equal(rank.cpu().numpy(), r)
    assert np.array_equal(srt.cpu().numpy().view(np.uint32), sv.view(np.uint32))
    assert np.array_equal(v_rr.cpu().numpy().view(np.uint32), sv.view(np.uint32)) and np.array_equal(y_rr.cpu().numpy(), yy)
    perm, rank, srt, moved = ops.rerank_lists(vd)
    assert rank is None and srt is None and moved == [] and np.array_equal(perm.cpu().numpy(), p)
    with pytest.raises(ValueError):
        ops.rerank_lists(vd, want_perm=False)
    with pytest.raises(ValueError):
        ops.rerank_lists(vd, yd[:, :-1])
    with pytest.raises(ValueError):
        ops.rerank_lists(vd, yd, yd, yd, yd, yd)
    # not a tape node
    g = vd.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        ops.rerank_lists(g)
    with pytest.raises(RuntimeError, match="not differentiable"):
        ops.rerank_lists(vd, yd.clone().requires_grad_(True))
    with torch.no_grad():
        assert np.array_equal(ops.rerank_lists(g)[0].cpu().numpy(), p)


def _cut_and_labels(B, S, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random((B, S)) < 0.2).astype(np.float32)
    y[0] = 0.0                                  # a list without a relevant document
    cut = torch.softmax(torch.from_numpy(rng.standard_normal((B, S)).astype(np.float32)), dim=1).cuda()
    return cut, torch.from_numpy(y).cuda(), y


def test_reranked_eval_identity_order_changes_nothing(lib):
    from utils.rerank import RerankedEval
    B, S = 37, 50
    ev = RerankedEval(S, by="rerank", metric="f1", reward="fbeta:2", fixed_k=(1, 5, 50, 70), sweep=np.linspace(-40.0, -5.0, 6))
    assert ev.fixed_k == (1, 5, 50)
    head = -torch.arange(S, dtype=torch.float32, device="cuda").repeat(B, 1)          # already descending
    for seed in (1, 2):
        cut, yd, _ = _cut_and_labels(B, S, seed)
        ev.update(head.reshape(B, S, 1), cut, yd)
    s = ev.summary()
    assert s["n"] == 2 * B and s["by"] == "rerank" and set(s["orig"]) == set(s["rr"]) == set(s["diff"])
    assert {"f1", "dcg", "best_cut_f1", "best_cut_dcg", "fixed_k5_f1", "greedy_k_f1", "reward", "best_cut_reward", "sweep_f1"} <= set(s["rr"])
    assert s["rr"] == s["orig"] and all(d == 0 for d in s["diff"].values())
    q = ev.per_query()
    for name in ("f1", "dcg", "best_f1", "best_k", "reward", "best_reward"):
        assert q[name].tobytes() == q[name + "_rr"].tobytes(), name
    assert not any("perm" in name for name in q)


def test_reranked_eval_by_the_labels_is_a_perfect_ranking(lib):
    from utils.rerank import RerankedEval
    B, S = 41, 300
    ev = RerankedEval(S, by="classi", metric="dcg")
    cut, yd, y = _cut_and_labels(B, S, 7)
    ev.update(yd, cut, yd)
    q = ev.per_query()
    n_rel = y.sum(axis=1).astype(np.int64)
    has = n_rel > 0
    assert has.sum() == B - 1
    assert (q["best_f1_rr"][has] == 1.0).all() and np.array_equal(q["best_k_rr"][has], n_rel[has])
    assert (q["best_f1_rr"][~has] == 0.0).all()
    assert (q["best_f1"] <= q["best_f1_rr"]).all() and np.array_equal(q["k"], cut.argmax(dim=1).cpu().numpy() + 1)
    s = ev.summary()
    assert s["rr"]["best_cut_f1"] == pytest.approx((B - 1) / B, abs=1e-12) and s["diff"]["best_cut_f1"] > 0


def test_model_rerank(lib):
    import models
    torch.manual_seed(0)
    B, S = 5, 8
    x = torch.randn(B, S, 3, device="cuda")
    for num_tasks, by in ((3, "rerank"), (3, "classi"), (2.2, "rerank"), (2.1, "classi")):
        m = models.MtAttnCut(num_tasks=num_tasks, dropout=0.3).cuda().train()
        perm, k = m.rerank(x, by=by)
        assert m.training and perm.dtype == torch.int32 and tuple(perm.shape) == (B, S) and tuple(k.shape) == (B,)
        m.eval()
        with torch.no_grad():
            out = m(x)
        head = out[m.head_names().index(by)].reshape(B, S).cpu().numpy()
        assert np.array_equal(perm.cpu().numpy(), RR.perm(head))
        assert np.array_equal(k.cpu().numpy(), m.truncate(x)[0].cpu().numpy())
    with pytest.raises(ValueError, match="no 'rerank' head"):
        models.AttnCut().cuda().rerank(x)
    with pytest.raises(ValueError, match="no 'classi' head"):
        models.MtAttnCut(num_tasks=2.2).cuda().rerank(x, by="classi")


def test_run_with_rerank_eval_end_to_end(lib, tmp_path):
    """One epoch of MtAttnCut on a synthetic set with --rerank-eval rerank: the history carries the `_rr` figures; then the
    checkpoint is reported with and without the flag: the flag adds `*_rr` arrays and `rerank_by`, and every other array of the
    two files has the same bytes."""
    import json
    import run
    from dataloader.synth import write_synthetic_robust04
    base, save = str(tmp_path / "data"), str(tmp_path / "ckpt")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=48, n_test=44, seed=11, seq_len=300)
    common = ["--model-name", "mtattncut", "--dataset-base", base, "--use-conf", "0", "--batch-size", "64", "--seed", "3", "--dropout", "0.1",
              "--save-path", save, "--criterion", "f1", "--tensorboard-dir", ""]
    hist = str(tmp_path / "history.json")
    run.main(common + ["--epochs", "1", "--model-persist", "1", "--rerank-eval", "rerank", "--history-json", hist])
    h = json.load(open(hist))["history"]
    rr = h[0]["test_rr"]
    assert rr["by"] == "rerank" and {"f1", "f1_rr", "dcg", "dcg_rr"} <= set(rr)
    assert rr["f1"] == pytest.approx(h[0]["test"][1], abs=1e-9) and rr["dcg"] == pytest.approx(h[0]["test"][2], abs=1e-9)
    (L, summ), = rr["lengths"].items()
    assert L == "300" and summ["n"] == 44 and summ["rr"]["best_cut_f1"] >= 0.0
    argv = common + ["--epochs", "0", "--ft", "1", "--model-path", os.path.join(save, "mtattncut.pkl")]
    flagged, plain = str(tmp_path / "rr.npz"), str(tmp_path / "plain.npz")
    run.main(argv + ["--rerank-eval", "rerank", "--report-out", flagged])
    run.main(argv + ["--report-out", plain])
    d, p0 = np.load(flagged), np.load(plain)
    new = {"f1_rr", "dcg_rr", "best_f1_rr", "best_k_rr", "rerank_by"}
    assert set(d.files) == set(p0.files) | new and not (set(p0.files) & new)
    for key in p0.files:
        assert d[key].tobytes() == p0[key].tobytes(), key
    assert str(d["rerank_by"]) == "rerank" and d["f1_rr"].shape == d["f1"].shape == (44,)
    with pytest.raises(ValueError, match="no such head"):
        run.Trainer(run.build_parser().parse_args(common + ["--num-tasks", "2.1", "--rerank-eval", "rerank"]))
