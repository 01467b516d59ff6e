"""rlt_probe_heads on the MI355X against the float64 restatement (tests/probe_restate.py), torch autograd in float64, the
reference modules' own results (tests/golden/probe_*.npz, tools/make_probe_golden.py), and the probe models built on it."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_restate as R  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
TOL = 1e-5


def _gold(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def _pm(x):
    """(B,S,E) numpy -> position-major (S*B,E) on the device."""
    B, S, E = x.shape
    return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2).reshape(S * B, E))).cuda()


def _raw(x, y, w, b, kinds, margin=5e-4, grads=True, out=True, shift=False):
    """One rlt_probe_heads call; returns numpy (loss, dw, db, out).  shift: x starts one float past a 16-byte boundary."""
    from rlt_hip import native as N
    B, S, E = x.shape
    n = len(kinds)
    xd, yd = _pm(x), torch.from_numpy(y).cuda()
    if shift:
        buf = torch.empty(xd.numel() + 1, device="cuda")
        buf[1:].copy_(xd.reshape(-1))
        xd = buf[1:].view(S * B, E)
        assert xd.data_ptr() % 16 == 4
    wd, bd = torch.from_numpy(np.ascontiguousarray(w)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    loss = torch.empty(n, device="cuda")
    dw = torch.empty(n, E, device="cuda") if grads else None
    db = torch.empty(n, device="cuda") if grads else None
    o = torch.empty(n, B, S, device="cuda") if out else None
    wsb = N.query("rlt_probe_heads_workspace", n, S, B, E)
    ws = N.workspace(wsb, xd.device)
    N.call("rlt_probe_heads", N.ptr(xd), N.ptr(wd), N.ptr(bd), (N.c_int * n)(*kinds), n, S, B, E, N.ptr(yd), margin,
           N.ptr(loss), N.ptr(dw), N.ptr(db), N.ptr(o), N.ptr(ws), wsb, N.stream())
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    return f(loss), f(dw), f(db), f(o)


def _check(got, ref, what, dscale=None):
    """Relative TOL on every output.  The rerank loss is a difference of two class means of softmax scores, each about 1/S:
    its error is measured against that size (fp32 cancellation, torch's too), not against the small difference."""
    loss, dw, db, out = got
    rl, rdw, rdb, rout = ref
    lscale = max(abs(rl), float(np.abs(rout).mean()) if np.allclose(rout.sum(axis=-1), 1.0) else 0.0, 1e-6)
    assert abs(loss - rl) <= TOL * lscale, (what, loss, rl)
    np.testing.assert_allclose(out, rout, rtol=TOL, atol=TOL * 1e-3 * np.abs(rout).max(), err_msg=what)
    if dw is not None:
        scale = max(np.abs(rdw).max(), dscale or 0.0, 1e-30)
        np.testing.assert_allclose(dw, rdw, rtol=0, atol=TOL * scale, err_msg=what)
        assert abs(db - rdb) <= TOL * max(scale, abs(rdb)), (what, db, rdb)


GRID = [(1, 40, 7, [0, 1]), (3, 300, 63, [1, 0, 0]), (25, 40, 512, [0, 1, 1, 0]), (47, 40, 1, [1]),
        (128, 300, 7, [0, 1, 0, 1, 0, 1]), (256, 300, 63, [0, 1]), (256, 40, 512, [1, 1, 0, 0, 1]),
        (3, 40, 512, [0]), (1, 300, 1, [1, 0]), (128, 40, 63, [1]), (1000, 40, 7, [0, 1, 1]),
        # every dispatch branch: scalar loads with 4 and 16 column chunks, 8 heads (NHM = 8) at each load width
        (129, 40, 7, [0, 1, 1, 0, 1, 0, 0, 1]), (1001, 40, 7, [1, 0, 1, 0, 0, 1, 1, 0]), (256, 300, 7, [0, 1, 0, 1, 1, 0, 1]),
        (1024, 40, 7, [1, 1, 0, 0, 1, 0, 1, 0]), (64, 40, 63, [0, 1, 1, 0, 1, 0, 1, 0])]


@pytest.mark.parametrize("E,S,B,kinds", GRID)
def test_kernel_against_float64_restatement(E, S, B, kinds):
    x, y = R.probe_data(100 + E + S + B, B, S, E)
    w, b = R.head_params(7 * E + len(kinds), len(kinds), E)
    loss, dw, db, out = _raw(x, y, w, b, kinds)
    for h, k in enumerate(kinds):
        ref = R.head(k, x, y, w[h], b[h])
        _check((loss[h], dw[h], db[h], out[h]), ref, f"E{E} S{S} B{B} head {h} kind {k}")


@pytest.mark.parametrize("E,kinds", [(256, [0, 1]), (1000, [1, 0, 1])])
def test_kernel_unaligned_features_take_the_scalar_loads(E, kinds):
    B, S = 7, 40
    x, y = R.probe_data(200 + E, B, S, E)
    w, b = R.head_params(201 + E, len(kinds), E)
    got = _raw(x, y, w, b, kinds, shift=True)
    for h, k in enumerate(kinds):
        _check(tuple(g[h] for g in got), R.head(k, x, y, w[h], b[h]), f"unaligned E{E} head {h}")


def test_kernel_against_torch_autograd_float64():
    B, S, E = 63, 300, 256
    x, y = R.probe_data(3, B, S, E)
    w, b = R.head_params(4, 2, E)
    got = _raw(x, y, w, b, [0, 1])
    xt, yt = torch.from_numpy(x).double(), torch.from_numpy(y).double()
    for h in range(2):
        lin = torch.nn.Linear(E, 1).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w[h:h + 1]))
            lin.bias.copy_(torch.from_numpy(b[h:h + 1]))
        z = lin(xt).squeeze(2)
        if h == 0:
            o = torch.sigmoid(z)
            loss = torch.nn.BCELoss()(o, yt)
        else:
            o = torch.softmax(z, dim=1)
            pos, neg = yt == 1, yt == 0
            loss = torch.clamp(o[neg].sum() / neg.sum() - o[pos].sum() / pos.sum() + 5e-4, min=0.0)
        loss.backward()
        ref = (loss.item(), lin.weight.grad[0].numpy(), lin.bias.grad.item(), o.detach().numpy())
        _check((got[0][h], got[1][h], got[2][h], got[3][h]), ref, f"autograd head {h}")


def test_edges_missing_class_hinge_and_saturation():
    B, S, E = 7, 40, 25
    x, _ = R.probe_data(9, B, S, E)
    w, b = R.head_params(10, 2, E)
    for y in (np.zeros((B, S), np.float32), np.ones((B, S), np.float32)):       # no positives / no negatives
        loss, dw, db, _ = _raw(x, y, w, b, [1, 1])
        assert np.all(loss == 0) and np.all(dw == 0) and np.all(db == 0)
    # hinge at or below 0: identical features along each list make every score exactly 1/32, so both class means are
    # exactly 1/32 and the hinge's argument is exactly the margin
    S2 = 32
    xs = np.repeat(x[:, :1, :], S2, axis=1)
    _, y = R.probe_data(9, B, S2, E)
    for margin in (0.0, -1e-6):
        loss, dw, db, out = _raw(xs, y, w, b, [1], margin=margin)
        assert np.all(out == 1.0 / 32)
        assert loss[0] == 0 and np.all(dw == 0) and db[0] == 0, margin
    loss, _, _, _ = _raw(xs, y, w, b, [1], margin=1e-3)
    assert loss[0] == np.float32(1e-3)                # active just above: the loss is the margin
    # logits of +-40 against torch in fp32.  At +40 the sigmoid is exactly 1: a 0 label costs log(0) clamped at -100 and the
    # gradient is exactly 0 (the 1e-12 clamp, then s(1-s) = 0); at -40 it is 4e-18, not 0, and both sides agree on it.
    xe = np.full((B, S, 1), 40.0, np.float32)
    ye = np.zeros((B, S), np.float32)
    ye[:, ::2] = 1.0
    loss, dw, db, out = _raw(xe, ye, np.ones((1, 1), np.float32), np.zeros(1, np.float32), [0])
    assert np.all(out == 1.0) and loss[0] == 50.0 and dw[0, 0] == 0 and db[0] == 0
    xe[:, 1::4, 0] = -40.0
    loss, dw, db, out = _raw(xe, ye, np.ones((1, 1), np.float32), np.zeros(1, np.float32), [0])
    lin = torch.nn.Linear(1, 1)
    with torch.no_grad():
        lin.weight.fill_(1.0)
        lin.bias.zero_()
    tl = torch.nn.BCELoss()(torch.sigmoid(lin(torch.from_numpy(xe))).squeeze(2), torch.from_numpy(ye))
    tl.backward()
    assert loss[0] == pytest.approx(tl.item(), rel=TOL)
    assert dw[0, 0] == pytest.approx(lin.weight.grad.item(), rel=TOL) and db[0] == pytest.approx(lin.bias.grad.item(), rel=TOL)


def test_bitwise_reproducible_and_eval_call():
    B, S, E = 512, 300, 128
    x, y = R.probe_data(21, B, S, E)
    w, b = R.head_params(22, 3, E)
    a = _raw(x, y, w, b, [0, 1, 0])
    c = _raw(x, y, w, b, [0, 1, 0])
    for u, v in zip(a, c):
        assert np.array_equal(u, v)
    ev = _raw(x, y, w, b, [0, 1, 0], grads=False)
    assert np.array_equal(ev[0], a[0]) and np.array_equal(ev[3], a[3])
    nout = _raw(x, y, w, b, [0, 1, 0], out=False)
    assert np.array_equal(nout[0], a[0]) and np.array_equal(nout[1], a[1])


def test_probe_heads_autograd_binding():
    from rlt_hip import native as N, ops
    B, S, E = 7, 40, 25
    x, y = R.probe_data(31, B, S, E)
    w, b = R.head_params(32, 2, E)
    ws = [torch.nn.Parameter(torch.from_numpy(w[h:h + 1]).cuda()) for h in range(2)]
    bs = [torch.nn.Parameter(torch.from_numpy(b[h:h + 1]).cuda()) for h in range(2)]
    xd, yd = _pm(x), torch.from_numpy(y).cuda()
    loss, outs = ops.probe_heads(xd, ws, bs, [N.PROBE_BCE, N.PROBE_RERANK], yd, S, B)
    assert outs[0].shape == (B, S, 1)
    (2.0 * loss[0] + 3.0 * loss[1]).backward()
    loss2, _ = ops.probe_heads(xd, ws, bs, [N.PROBE_BCE, N.PROBE_RERANK], yd, S, B)
    loss2.sum().backward()                                             # .grad accumulates
    for h, k, c in ((0, 0, 3.0), (1, 1, 4.0)):
        _, rdw, rdb, _ = R.head(k, x, y, w[h], b[h])
        np.testing.assert_allclose(ws[h].grad.cpu().numpy()[0], c * rdw, rtol=0, atol=1e-5 * c * np.abs(rdw).max())
    with pytest.raises(ValueError):
        ops.probe_heads(xd.requires_grad_(), ws, bs, [0, 1], yd, S, B)


@pytest.mark.parametrize("S", [40, 300])
def test_against_reference_fixtures(S):
    import models as hm
    from oracle.weights import fill_state_dict
    g = _gold(f"probe_heads_s{S}")
    for tag in sorted({k.split("/")[0] for k in g if not k.startswith("adam")}):
        B, S_, E = (int(v) for v in g[f"{tag}/shape"])
        seed = int(g[f"{tag}/seed"])
        model = (hm.TaskC if tag[0] == "c" else hm.TaskR)(d_model=E)
        fill_state_dict(model, seed)
        model = model.cuda()
        x, y = R.probe_data(seed + 1, B, S_, E)
        loss, outs = model.loss(_pm(x), torch.from_numpy(y).cuda(), S_, B)
        loss.sum().backward()
        ref = (float(g[f"{tag}/loss"]), g[f"{tag}/dw"], float(g[f"{tag}/db"][0]), g[f"{tag}/out"])
        got = (float(loss[0].detach()), model.linear.weight.grad.cpu().numpy()[0], float(model.linear.bias.grad[0]),
               outs[0].squeeze(2).detach().cpu().numpy())
        _check(got, ref, tag)
        fwd = model(torch.from_numpy(x).cuda()).squeeze(2).cpu().numpy()          # the module's forward
        np.testing.assert_allclose(fwd, g[f"{tag}/out"], rtol=TOL, atol=TOL * 1e-3, err_msg=tag)
        if S == 40:                                   # five Adam steps, FusedAdam over the probe's flat parameters
            from rlt_hip.parallel import FlatModel, FusedAdam
            m2 = (hm.TaskC if tag[0] == "c" else hm.TaskR)(d_model=E)
            fill_state_dict(m2, seed)
            m2 = m2.cuda()
            b0 = float(m2.linear.bias.detach()[0])
            flat = FlatModel(m2)
            opt = FusedAdam(flat, lr=float(g["adam/lr"]))
            for step in range(5):
                opt.zero_grad()
                ls, _ = m2.loss(_pm(x), torch.from_numpy(y).cuda(), S_, B, want_out=False)
                ls.sum().backward()
                opt.step()
                assert abs(float(ls[0]) - g[f"adam_{tag}/loss"][step]) <= TOL * max(abs(g[f"adam_{tag}/loss"][step]), 1.0 / S_)
                np.testing.assert_allclose(m2.linear.weight.detach().cpu().numpy()[0], g[f"adam_{tag}/w"][step], rtol=0,
                                           atol=TOL * np.abs(g[f"adam_{tag}/w"][step]).max(), err_msg=f"adam {tag} {step}")
                gb, hb = float(g[f"adam_{tag}/b"][step]), float(m2.linear.bias.detach()[0])
                if tag[0] == "c":
                    assert abs(hb - gb) <= TOL * max(1.0, abs(gb)), (tag, step)
                else:
                    # a softmax head's bias gradient is exactly 0 (sum_i dz_i = 0): the bias stays put here, while torch's
                    # fp32 rounding noise, normalised by Adam, moves the reference's by a small fraction of lr per step
                    assert hb == b0 and abs(gb - b0) <= (step + 1) * float(g["adam/lr"]), (tag, step, hb, gb, b0)


@pytest.fixture(params=["bf16x6", "fp32", "bf16x3"])
def precision(request):
    from rlt_hip import native
    keep = native.get_precision()
    native.set_precision(request.param)
    yield request.param
    native.set_precision(keep)


def test_probebase_and_probe_against_fixture(precision):
    """ProbeBase in each MFMA precision mode, held to the MMOECut model tolerance (the same in all three modes)."""
    import models as hm
    from oracle.weights import fill_state_dict, synthetic_lists
    g = _gold("probe_models_s40")
    B, S, F = (int(v) for v in g["pb/shape"])
    pb = hm.ProbeBase(seq_len=S, dropout=0.0).eval()
    fill_state_dict(pb, int(g["pb/seed"]))
    pb = pb.cuda()
    x, _ = synthetic_lists(B, S, F, int(g["pb/seed"]) + 1)
    with torch.no_grad():
        experts_in, experts_o, towers = pb(x.cuda())
    got = [("experts_in", experts_in), ("expert0", experts_o[0]), ("expert1", experts_o[1])] + \
        [(f"tower{i}", t) for i, t in enumerate(towers)]
    for name, t in got:
        a = t.contiguous().cpu().numpy().reshape(-1)
        ref_norm = float(g[f"pb/{name}/norm"])
        assert abs(np.linalg.norm(a.astype(np.float64)) - ref_norm) <= 1e-4 * ref_norm, name      # the MMOECut model bound
        np.testing.assert_allclose(a[g[f"pb/{name}/idx"]], g[f"pb/{name}/val"], rtol=0,
                                   atol=1e-4 * np.abs(a).max(), err_msg=name)
    # the Probe's six heads on those features: the fused losses equal the restatement on the same features
    probe = hm.Probe().cuda()
    y = (torch.rand(B, S, device="cuda") < 0.3).float()
    with torch.no_grad():
        h_pm, e_pm, _ = pb.forward_pm(x.cuda())
    res = probe.losses([h_pm, e_pm[0], e_pm[1]], y, S, B)
    assert set(res) == {"c1", "r1", "ce1", "ce2", "re1", "re2"}
    feats = {"c1": experts_in, "r1": experts_in, "ce1": experts_o[0], "re1": experts_o[0], "ce2": experts_o[1], "re2": experts_o[1]}
    for name, (loss, out) in res.items():
        mod = getattr(probe, "probe_" + name)
        kind = R.BCE if name.startswith("c") else R.RERANK
        ref = R.head(kind, feats[name].contiguous().cpu().numpy(), y.cpu().numpy(),
                     mod.linear.weight.detach().cpu().numpy()[0], float(mod.linear.bias[0]))
        assert abs(float(loss) - ref[0]) <= TOL * max(abs(ref[0]), 1.0 / S), name
        np.testing.assert_allclose(out.squeeze(2).cpu().numpy(), ref[3], rtol=TOL, atol=1e-9, err_msg=name)


# ---------------------------------------------------------------------------------------- the scripts, end to end
PKG = os.path.join(REPO, "ranked-list-truncation_amd")


def _script(name, args, timeout=240):
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(PKG, name)] + [str(a) for a in args], capture_output=True, text=True,
                         timeout=timeout, cwd=REPO)
    assert res.returncode == 0, (name, res.stdout[-1500:], res.stderr[-3000:])
    return res


@pytest.fixture(scope="module")
def small_set(tmp_path_factory):
    """A small robust04-shaped synthetic set and 1-epoch AttnCut / Choopy checkpoints of run.py --model-persist 1."""
    from dataloader import write_synthetic_robust04
    base = tmp_path_factory.mktemp("probe_data")
    write_synthetic_robust04(str(base), "robust04", "drmm_tks", n_train=40, n_test=20, seed=5)
    ckpt = base / "ckpt"
    for model in ("attncut", "choopy"):
        _script("run.py", ["--model-name", model, "--dataset-base", base, "--use-conf", "0", "--epochs", 1, "--batch-size", 20,
                           "--model-persist", 1, "--save-path", ckpt, "--tensorboard-dir", "", "--seed", 1])
        assert (ckpt / f"{model}.pkl").exists()
    return base, ckpt


def _finite(v):
    return v is not None and np.isfinite(v)


@pytest.mark.parametrize("model,ft,vt", [("attncut", 0, "c"), ("attncut", 1, "r"), ("choopy", 1, "c")])
def test_verify_bmt_end_to_end(small_set, tmp_path, model, ft, vt):
    base, ckpt = small_set
    hist = tmp_path / "hist.json"
    _script("verify_BMT.py", ["--model-name", model, "--verify-type", vt, "--ft", ft, "--model-path", ckpt / f"{model}.pkl",
                              "--dataset-base", base, "--epochs", 2, "--batch-size", 20, "--lr", 1e-3, "--seed", 3,
                              "--history-json", hist, "--tensorboard-dir", tmp_path / "tb"])
    out = json.loads(hist.read_text())
    assert out["metric_name"] == ("auc" if vt == "c" else "DCG")
    assert len(out["train_metrics"]) == 2 and all(_finite(v) for v in out["train_metrics"])
    for h in out["history"]:
        assert all(_finite(v) for v in h["train"] + h["test"])
    if vt == "c":
        assert all(0.0 <= v <= 1.0 for v in out["train_metrics"])
    tags = {json.loads(line)["tag"] for line in open(tmp_path / "tb" / "scalars.jsonl")}
    assert {"train/loss_epoch", "test/loss_epoch"} <= tags


def test_verify_probe_end_to_end(small_set, tmp_path):
    base, _ = small_set
    hist = tmp_path / "hist.json"
    _script("verify_probe.py", ["--ft", 0, "--dataset-base", base, "--epochs-base", 1, "--epochs-probe", 2, "--batch-size", 20,
                                "--lr", 1e-3, "--seed", 3, "--save-path", tmp_path / "ckpt", "--history-json", hist,
                                "--tensorboard-dir", tmp_path / "tb"])
    out = json.loads(hist.read_text())
    assert len(out["base"]) == 1 and (tmp_path / "ckpt" / "probe_base.pkl").exists()
    assert len(out["probe"]) == 2
    for h in out["probe"]:
        assert all(_finite(h[k]) for k in ("c1", "r1", "ce1", "ce2", "re1", "re2")), h
        assert all(0.0 <= h[k] <= 1.0 for k in ("c1", "ce1", "ce2"))
    recs = [json.loads(line) for line in open(tmp_path / "tb" / "scalars.jsonl")]
    steps = [r["step"] for r in recs if r["tag"] == "probe/expert0_rerank"]
    assert steps == list(range(len(steps))) and len(steps) == 4          # 2 epochs x 2 steps, a counter that counts
    assert set(out["tags"].values()) == {r["tag"] for r in recs}
