"""model.stream / utils.stream.StreamingTruncator end to end (`pytest -m gpu`): a position-axis, causal, hazard-head Choopy
(seq_len 70, d_model 128, 2 layers, random weights, the decision layer scaled so that the stop probabilities spread) fed a page of
ranks at a time, in the three precision modes.

GEMM dispatch may choose another kernel at M = C*B rows than at M = S*B, so the streamed stop probabilities are NOT required
bit-equal to the one-shot model.stop_probabilities(x).  Both are measured against stop64, a float64 torch restatement
(nn.TransformerEncoder in double under the triangular mask + the hazard formula of tests/hazard_restate.py):

    max |stop_stream - stop64|  <=  max(4 * max |stop_oneshot - stop64|, 2^-22)

the margin of 4 covering a different summation order in the five GEMMs of each layer.  Cuts: tau is the midpoint of the widest gap
between neighbouring sorted one-shot stop values inside their 30 % .. 70 % quantile range; that gap must exceed twice the measured
distance (asserted), and then every list's streamed k equals model.truncate(x, rule='above', tau=tau) for pages of 1, 10, 32, 70."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import hazard_restate as H

pytestmark = pytest.mark.gpu
S, B, E, HEADS, LAYERS = 70, 6, 128, 8, 2
PAGES = (1, 10, 32, 70)


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def setup():
    """-> model, x (B,S,1), stop64 (B,S) float64 numpy"""
    import models as hm
    torch.manual_seed(21)
    m = hm.Choopy(seq_len=S, d_model=E, n_head=HEADS, num_layers=LAYERS, dropout=0.0, attention_axis="position",
                  attention_mask="causal", cut_head="hazard").to(dev()).eval()
    lin = getattr(m.decison_layer, "0")
    with torch.no_grad():
        lin.weight.mul_(6.0)
    x = 10.0 * torch.randn(B, S, 1, device=dev())          # one input column of 128: large, so that the lists differ from each other
    # float64 restatement on the host
    enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(d_model=E, nhead=HEADS, dropout=0.0), num_layers=LAYERS,
                                      enable_nested_tensor=False).double().eval()
    enc.load_state_dict({k: v.detach().double().cpu() for k, v in m.attention_layer.state_dict().items()})
    with torch.no_grad():
        pe = m.position_encoding.detach().double().cpu()
        h = torch.cat([x.double().cpu(), pe.unsqueeze(0).expand(B, S, E - 1)], 2).transpose(0, 1)          # (S, B, E)
        mask = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
        h = enc(h, mask=mask)
        z = (h @ lin.weight.detach().double().cpu().reshape(E, 1))[..., 0].transpose(0, 1) + float(lin.bias)   # (B, S)
    z = z.numpy() + H.prior_offset(S)[None, :]
    _, stop64 = H.forward(z)
    return m, x, stop64


def streamed(m, x, tau, page):
    """-> stop (B,S), k, documents_read - one truncator, pages of `page` ranks"""
    st = m.stream(tau, B)
    stops = []
    for t0 in range(0, S, page):
        assert st.position == t0
        res = st.push(x[:, t0:t0 + page])
        stops.append(res["stop"])
    assert st.position == S and not bool(res["active"].any())
    return torch.cat(stops, 1), res["k"], st.documents_read(), st


@pytest.mark.parametrize("mode", ("fp32", "bf16x6", "bf16x3"))
def test_streamed_stops_and_cuts_against_the_one_shot_model_and_float64(N, mode):
    from rlt_hip import ops
    m, x, stop64 = setup()
    with ops.precision(mode):
        one = m.stop_probabilities(x)
        d_one = float(np.abs(one.double().cpu().numpy() - stop64).max())
        # tau = 2: nothing stops before the end, every row of every list is computed
        d_stream, equal = 0.0, True
        for page in PAGES:
            stop, k, _, _ = streamed(m, x, 2.0, page)
            assert bool(torch.isfinite(stop).all()) and bool((k == S).all())
            d = float(np.abs(stop.double().cpu().numpy() - stop64).max())
            print(f"  {mode} page {page}: max|stream - f64| = {d:.3e}, max|one-shot - f64| = {d_one:.3e}, bit-equal to the one-shot: {torch.equal(stop, one)}")
            d_stream, equal = max(d_stream, d), equal and torch.equal(stop, one)
            assert d <= max(4 * d_one, 2.0 ** -22), (mode, page, d, d_one)
        # the cuts
        inner = np.sort(one[:, :-1].double().cpu().numpy().reshape(-1))
        mid = inner[int(0.3 * inner.size):int(0.7 * inner.size) + 1]
        gaps = np.diff(mid)
        g = int(gaps.argmax())
        tau = float((mid[g] + mid[g + 1]) / 2)
        assert gaps[g] > 2 * max(d_stream, d_one), (gaps[g], d_stream, d_one)
        want = m.truncate(x, rule="above", tau=tau)
        assert len(set(want.tolist())) > 1, want                         # the lists do not all cut at one rank
        for page in PAGES:
            stop, k, read, st = streamed(m, x, tau, page)
            assert torch.equal(k, want), (mode, page, k, want)
            # ceil(k / C) * C; the list's last page may be short (70 = 32 + 32 + 6), and ranks that do not exist are not read
            assert torch.equal(read.long(), ((want.long() + page - 1) // page * page).clamp(max=S))
            # the rows of a list behind the page of its stop were not computed
            pages_of = (want.long() + page - 1) // page * page
            cols = torch.arange(S, device=dev())[None, :]
            assert bool(torch.isnan(stop[cols >= pages_of[:, None]]).all()) and bool(torch.isfinite(stop[cols < pages_of[:, None]]).all())
            # reset() reproduces the run bit for bit
            st.reset()
            assert st.position == 0 and bool((st.k == 0).all())
            again = torch.cat([st.push(x[:, t0:t0 + page])["stop"] for t0 in range(0, S, page)], 1)
            assert torch.equal(again.view(torch.int32), stop.view(torch.int32)) and torch.equal(st.k, want)
            assert torch.equal(st.documents_read(), read)


def test_documents_read_counts_whole_pages_of_the_last_short_page(N):
    m, x, _ = setup()
    st = m.stream(2.0, B)
    for t0 in range(0, S, 32):                                            # 32 + 32 + 6
        out = st.push(x[:, t0:t0 + 32, 0])                                # (B, C) is taken too
    assert bool((out["k"] == S).all()) and bool((st.documents_read() == S).all())
    with pytest.raises(ValueError):
        st.push(x[:, :1])                                                 # past seq_len
    with pytest.raises(ValueError):
        m.stream(0.5, B).push(x[:2, :4])                                  # another batch size


def test_stream_raises_on_every_wrong_configuration_and_class(N):
    import models as hm
    for kw, word in (({"attention_axis": "list"}, "attention_axis"), ({"attention_axis": "position"}, "attention_mask"),
                     ({"attention_axis": "position", "attention_mask": "causal"}, "cut_head"),
                     ({"attention_axis": "position", "cut_head": "hazard"}, "attention_mask"), ({"cut_head": "hazard"}, "attention_axis")):
        with pytest.raises(ValueError, match=word):
            hm.Choopy(seq_len=S, **kw).stream(0.5, 2)
    for cls, kw, word in ((hm.AttnCut, {}, "BiLSTM"), (hm.MtChoopy, {}, "normalise"), (hm.MtAttnCut, {}, "BiLSTM"),
                          (hm.BiCut, {"input_size": 3}, "BiLSTM"), (hm.MMOECut, {}, "cannot stream"), (hm.MOECut, {}, "cannot stream"),
                          (hm.PLECut, {}, "cannot stream")):
        with pytest.raises(ValueError, match=word):
            cls(**kw).stream(0.5, 2)


def test_run_py_stream_eval(N, tmp_path):
    import run
    from dataloader.synth import write_synthetic_robust04
    base, hist = str(tmp_path / "data"), str(tmp_path / "h.json")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=16, n_test=8, seed=3, seq_len=40)
    common = ["--model-name", "choopy", "--dataset-base", base, "--use-conf", "0", "--batch-size", "8", "--seed", "1", "--epochs", "1",
              "--tensorboard-dir", ""]
    online = ["--attention-axis", "position", "--attention-mask", "causal", "--cut-head", "hazard"]
    run.main(common + online + ["--stream-eval", "10", "--stream-tau", "0.05", "--history-json", hist])
    h = json.load(open(hist))
    assert h["stream_page"] == 10 and h["stream_tau"] == 0.05 and h["stream_lists"] == 8
    assert 1 <= h["stream_k"] <= 40 and h["stream_k"] <= h["stream_read"] <= 40 and h["stream_read"] % (10 / 8) == 0
    assert math.isfinite(h["stream_f1"]) and math.isfinite(h["stream_dcg"])
    # off by default, and an error off the online configuration
    hist2 = str(tmp_path / "h2.json")
    run.main(common + online + ["--history-json", hist2])
    assert not [k for k in json.load(open(hist2)) if k.startswith("stream_")]
    with pytest.raises(SystemExit):
        run.main(common + ["--stream-eval", "10"])
    with pytest.raises(SystemExit):
        run.main(["--model-name", "attncut"] + common[2:] + ["--stream-eval", "10"])
