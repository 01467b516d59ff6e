"""cut_head='hazard' from the models up to run.py (`pytest -m gpu`): the online property of Choopy with within-list causal attention and
the hazard head, the untouched default path, parameters that do not change, the multi-task heads in their order, gradients
through ops.hazard_head against torch float64 autograd, and one epoch of run.py.  Small shapes: B <= 6, S in {40, 65}."""
import json
import math

import numpy as np
import pytest
import torch

import hazard_restate as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


def online_choopy(S, seed=5, **kw):
    import models as hm
    torch.manual_seed(seed)
    return hm.Choopy(seq_len=S, attention_axis="position", attention_mask="causal", **kw).to(dev()).eval()


@pytest.mark.parametrize("i", [0, 20, 63])
def test_stop_probabilities_and_the_above_rule_are_online(N, i):
    """scores at ranks > i perturbed: the stop probabilities at ranks <= i keep their bits, and every list that had cut at
    k <= i + 1 under the `above` rule cuts there still.  tau is the median over the lists of the largest stop probability among
    ranks <= i of the unperturbed run, so at least half the lists cut there - asserted, it is what makes the test say something."""
    B, S = 6, 65
    m = online_choopy(S, cut_head="hazard")
    torch.manual_seed(100 + i)
    x = torch.randn(B, S, 1, device=dev())
    x2 = x.clone()
    x2[:, i + 1:] += torch.randn(B, S - i - 1, 1, device=dev())
    stop, stop2 = m.stop_probabilities(x), m.stop_probabilities(x2)
    assert tuple(stop.shape) == (B, S)
    assert torch.equal(stop[:, :i + 1], stop2[:, :i + 1])
    if i + 1 < S - 1:
        assert not torch.equal(stop[:, i + 1:S - 1], stop2[:, i + 1:S - 1])            # (the perturbation did reach the model)
    assert bool((stop[:, -1] == 1).all())
    tau = float(stop[:, :i + 1].max(1).values.median())
    k, k2 = m.truncate(x, rule="above", tau=tau), m.truncate(x2, rule="above", tau=tau)
    early = k <= i + 1
    assert float(early.float().mean()) >= 0.5, (k, tau)
    assert torch.equal(k[early], k2[early])
    # the rule reads the stop probabilities: the first rank that reaches tau
    want = (stop.double() >= tau).float().argmax(1) + 1
    assert torch.equal(k.long(), want.long())
    # every other rule, and the argmax, read p
    p = m(x)
    assert tuple(p.shape) == (B, S, 1) and float((p.detach().sum(1) - 1).abs().max()) < 1e-5
    kq = m.truncate(x, rule="quantile", tau=0.5)
    assert torch.equal(kq.long(), ((p[..., 0].double().cumsum(1) >= 0.5).float().argmax(1) + 1).long())
    ka, pk = m.truncate(x)
    assert torch.equal(ka.long(), p[..., 0].argmax(1) + 1) and torch.equal(pk, p[..., 0].max(1).values)
    # without the causal mask the same head is not online: the encoder under it reads the whole list
    import models as hm
    full = hm.Choopy(seq_len=S, attention_axis="position", cut_head="hazard").to(dev()).eval()
    full.load_state_dict(m.state_dict())
    assert not torch.equal(full.stop_probabilities(x)[:, :i + 1], full.stop_probabilities(x2)[:, :i + 1])


@pytest.mark.parametrize("name", ["Choopy", "AttnCut", "MtChoopy", "MtAttnCut"])
def test_default_path_is_untouched_and_parameters_do_not_change(N, name):
    import models as hm
    B, S = 4, 40
    cls = getattr(hm, name)
    kw = {"seq_len": S} if "Choopy" in name else {}
    torch.manual_seed(3)
    plain = cls(**kw).to(dev()).eval()
    torch.manual_seed(3)
    soft = cls(cut_head="softmax", **kw).to(dev()).eval()
    torch.manual_seed(3)
    haz = cls(cut_head="hazard", **kw).to(dev()).eval()
    assert (plain.cut_head, soft.cut_head, haz.cut_head) == ("softmax", "softmax", "hazard") and haz.hazard_prior == "uniform"
    x = torch.randn(B, S, 1 if "Choopy" in name else 3, device=dev())
    as_list = lambda o: list(o) if isinstance(o, (list, tuple)) else [o]
    with torch.no_grad():
        a, b, c = as_list(plain(x)), as_list(soft(x)), as_list(haz(x))
    assert len(a) == len(b) == len(c) and all(torch.equal(u, v) for u, v in zip(a, b))          # bit for bit
    assert all(torch.equal(u, v) for u, v in zip(a[:-1], c[:-1])) and not torch.equal(a[-1], c[-1])
    assert tuple(c[-1].shape) == (B, S, 1) and float((c[-1].sum(1) - 1).abs().max()) < 1e-5
    keys = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert keys(plain) == keys(soft) == keys(haz)
    haz.load_state_dict(plain.state_dict())                                                     # checkpoints load across heads
    plain.load_state_dict(haz.state_dict())
    for bad in ({"cut_head": "geometric"}, {"cut_head": None}, {"cut_head": "hazard", "hazard_prior": "flat"}):
        with pytest.raises(ValueError):
            cls(**bad, **kw)
    with pytest.raises(ValueError):
        plain.stop_probabilities(x)
    assert tuple(haz.stop_probabilities(x).shape) == (B, S) and not haz.training


@pytest.mark.parametrize("name", ["MtChoopy", "MtAttnCut"])
@pytest.mark.parametrize("num_tasks", [3, 2.1, 2.2])
def test_mt_models_return_their_heads_in_the_existing_order(N, name, num_tasks):
    import models as hm
    B, S = 3, 40
    cls = getattr(hm, name)
    kw = {"seq_len": S} if "Choopy" in name else {}
    torch.manual_seed(4)
    soft = cls(num_tasks=num_tasks, **kw).to(dev()).eval()
    haz = cls(num_tasks=num_tasks, cut_head="hazard", **kw).to(dev()).eval()
    haz.load_state_dict(soft.state_dict())
    x = torch.randn(B, S, 1 if "Choopy" in name else 3, device=dev())
    with torch.no_grad():
        a, c = soft(x), haz(x)
    names = {3: ("classi", "rerank", "decison_layer"), 2.1: ("classi", "decison_layer"), 2.2: ("rerank", "decison_layer")}[num_tasks]
    assert haz.head_names() == soft.head_names() == names and len(a) == len(c) == len(names)
    for nm, u, v in zip(names, a, c):
        assert tuple(u.shape) == tuple(v.shape) == (B, S, 1)
        assert torch.equal(u, v) == (nm != "decison_layer"), nm
    stop = haz.stop_probabilities(x)
    # p is the hazard product of the model's own stop probabilities
    s8 = stop.double()
    surv = torch.cat([torch.ones(B, 1, dtype=torch.float64, device=dev()), torch.cumprod(1 - s8[:, :-1], 1)], 1)
    assert float((c[-1][..., 0].double() - s8 * surv).abs().max()) < 1e-6


def test_priors(N):
    """zero weight and bias: the uniform prior gives p = 1/S, no prior the geometric distribution with p_0 = 1/2"""
    import models as hm
    B, S = 2, 40
    x = torch.randn(B, S, 1, device=dev())
    for prior, want in (("uniform", np.full(S, 1.0 / S)), ("none", np.r_[0.5 ** np.arange(1, S), 0.5 ** (S - 1)])):
        m = hm.Choopy(seq_len=S, cut_head="hazard", hazard_prior=prior).to(dev()).eval()
        with torch.no_grad():
            lin = getattr(m.decison_layer, "0")
            lin.weight.zero_()
            lin.bias.zero_()
            p = m(x)[..., 0].double().cpu().numpy()
        # the offsets are fp32: each logit is off by at most u ln S, and d log p_s = (1 - h_s) dz_s - sum_{j<s} h_j dz_j with
        # sum_j h_j = sum_j 1 / (S - j) <= 1 + ln S; one more u for p's own rounding
        rel = U * math.log(S) * (2 + math.log(S)) + U
        assert (np.abs(p - want[None, :]) <= rel * want[None, :]).all(), prior
    assert "hazard_offset" not in " ".join(m.state_dict())


def test_gradients_reach_the_position_encoding_and_match_float64_autograd(N):
    """ChoopyLoss through the hazard head: finite, non-zero gradients at the position encoding; and on the encoder output the
    gradients of ops.hazard_head match torch float64 autograd of the composition at the device's logits and the loss's own dp,
    within the bounds of tests/test_hazard_gpu.py (dx 2 ulp, dw / db the fp32 summation bounds over S B terms)."""
    from models import _common as MC
    from rlt_hip import ops
    from utils import losses as hl
    B, S = 5, 65
    m = online_choopy(S, seed=9, cut_head="hazard")
    m.train()
    m.dropout = 0.0
    x = torch.randn(B, S, 1, device=dev())
    y = (torch.rand(B, S, device=dev()) < 0.3).float()
    loss = hl.ChoopyLoss(metric="f1")(m(x), y)
    loss.backward()
    g = m.position_encoding.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    for prm in m.parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all())

    with torch.no_grad():
        h = MC.encoder(ops.choopy_embed(x, m.position_encoding), m.attention_layer, m.n_head, S, B, 0.0, "position", True)
    E = h.shape[1]
    lin = getattr(m.decison_layer, "0")
    w, b = lin.weight.detach().clone().requires_grad_(True), lin.bias.detach().clone().requires_grad_(True)
    off = m.hazard_offset(S, h.device)
    hl_ = h.clone().requires_grad_(True)
    p, stop = ops.hazard_head(hl_, w, b, S, B, off)
    p.retain_grad()
    stop.retain_grad()
    (hl.ChoopyLoss(metric="f1")(p.unsqueeze(2), y) + 0.25 * (stop * stop).sum()).backward()
    dp, dstop = p.grad.double().cpu(), stop.grad.double().cpu()
    # the device's logits, through the C ABI
    z = torch.empty(B, S, device=dev())
    p2 = torch.empty(B, S, device=dev())
    N.call("rlt_hazard_head_fwd", N.ptr(h), N.ptr(w.detach().reshape(-1).contiguous()), N.ptr(b.detach()), N.ptr(off), S, B, E, N.ptr(p2), None, N.ptr(z), N.stream())
    torch.cuda.synchronize()
    assert torch.equal(p2, p.detach())
    zt = z.double().cpu().requires_grad_(True)
    F = torch.nn.functional
    head = zt[:, :S - 1]
    L = torch.cat([torch.zeros(B, 1, dtype=torch.float64), torch.cumsum(F.logsigmoid(-head), 1)], 1)
    p_t = torch.exp(torch.cat([F.logsigmoid(head), torch.zeros(B, 1, dtype=torch.float64)], 1) + L)
    stop_t = torch.cat([torch.sigmoid(head), torch.ones(B, 1, dtype=torch.float64)], 1)
    ((p_t * dp).sum() + (stop_t * dstop).sum()).backward()
    assert np.abs(zt.grad.numpy() - H.backward(z.double().cpu().numpy(), dp.numpy(), dstop.numpy())).max() <= 1e-12
    dz = zt.grad.float().double().numpy()                                   # fp32(dz), (B,S)
    dz_pm = dz.T.reshape(S * B, 1)
    w8, x8 = w.detach().double().cpu().numpy().reshape(1, E), h.double().cpu().numpy()
    prod = dz_pm * w8
    err = np.abs(hl_.grad.double().cpu().numpy() - prod) / (2 * H.ulp32(prod) + TINY * np.abs(w8))
    err_w = np.abs(w.grad.double().cpu().numpy().reshape(-1) - (dz_pm * x8).sum(0)) / ((S * B + 3) * U * (np.abs(dz_pm) * np.abs(x8)).sum(0))
    err_b = abs(float(b.grad) - dz.sum()) / ((S * B + 2) * U * np.abs(dz).sum())
    print(f"  worst error as a multiple of its bound: dx {err.max():.3f}, dw {err_w.max():.3f}, db {err_b:.3f}")
    assert err.max() <= 1 and err_w.max() <= 1 and err_b <= 1


def test_run_py_trains_sweeps_and_records_the_head(N, tmp_path, caplog):
    import logging
    import run
    from dataloader.synth import write_synthetic_robust04
    base, state = str(tmp_path / "data"), str(tmp_path / "state.pt")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=16, n_test=8, seed=3, seq_len=40)
    common = ["--model-name", "choopy", "--dataset-base", base, "--use-conf", "0", "--batch-size", "8", "--seed", "1", "--epochs", "1",
              "--tensorboard-dir", "", "--cut-head", "hazard"]
    with caplog.at_level(logging.WARNING):
        run.main(common + ["--attention-axis", "position", "--attention-mask", "causal", "--save-state", state, "--model-persist", "1",
                           "--report-out", str(tmp_path / "r.npz"), "--save-path", str(tmp_path / "best"),
                           "--cut-sweep", "above:0.02:0.5:5", "--sweep-out", str(tmp_path / "sweep.json")])
    assert not [r for r in caplog.records if "--cut-head hazard without" in r.getMessage()]
    st = torch.load(state, map_location="cpu")
    assert st["cut_head"] == "hazard" and st["hazard_prior"] == "uniform" and st["attention_mask"] == "causal"
    assert not any("hazard" in k for k in st["model"])
    rep = np.load(str(tmp_path / "r.npz"))
    assert str(rep["cut_head"]) == "hazard" and str(rep["hazard_prior"]) == "uniform"
    meta = json.load(open(str(tmp_path / "best" / "choopy.pkl.meta.json")))
    assert meta == {"attention_axis": "position", "attention_mask": "causal", "cut_head": "hazard", "hazard_prior": "uniform"}
    sweep = json.load(open(str(tmp_path / "sweep.json")))["results"]["40"]
    assert sweep["rule"] == "above" and math.isfinite(sweep["test"]["f1"]) and 1 <= sweep["test"]["k"] <= 40
    # stop probabilities start near 1/(S-s) >= 1/40: thresholds between 0.02 and 0.5 give cuts that move with tau
    curve = json.load(open(str(tmp_path / "sweep.json")))["curves"]["test_k_40"]
    assert curve == sorted(curve) and curve[0] < curve[-1]
    # off the online configuration the run goes through, with a warning
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        run.main(common + ["--save-state", str(tmp_path / "s2.pt")])
    assert [r for r in caplog.records if "--cut-head hazard without" in r.getMessage()]
    st2 = torch.load(str(tmp_path / "s2.pt"), map_location="cpu")
    assert st2["cut_head"] == "hazard" and "attention_mask" not in st2
    args = run.build_parser().parse_args([])
    assert args.cut_head == "softmax" and args.hazard_prior == "uniform"
    with pytest.raises(ValueError):
        run.main(["--model-name", "bicut", "--dataset-base", base, "--use-conf", "0", "--epochs", "0", "--tensorboard-dir", "",
                  "--cut-head", "hazard"])
