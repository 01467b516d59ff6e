"""StreamingTruncator with batch compaction end to end (`pytest -m gpu`): the model, inputs, float64 restatement and tau choice of
tests/test_stream_model_gpu.py (a position-axis, causal, hazard-head Choopy: seq_len 70, 6 lists, d_model 128, 8 heads, 2 layers,
random weights, the decision layer scaled so that the stop probabilities spread), restated here, in the three precision modes.

After a compaction the chunk's GEMMs run at another row count, so the streamed stop probabilities are NOT required bit-equal to the
uncompacted stream (the existing position for the page size); they are held to that file's bound against the float64 restatement,

    max |stop_stream - stop64|  <=  max(4 * max |stop_oneshot - stop64|, 2^-22)

over the entries that were computed, and tau sits in a gap of the one-shot stop values wider than twice the measured distance, so
that every cut equals model.truncate(x, rule='above', tau=tau).  What IS exact: the cuts, documents_read, the NaN pattern of stop,
live_lists() after every push, and rows_computed() - the sum over the pages of C * (lists active on entry to the page), the
timing-free statement that the GEMMs shrank."""
import functools
import json

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
    x = 10.0 * torch.randn(B, S, 1, device=dev())
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


def tau_in_a_gap(one):
    """the midpoint of the widest gap between neighbouring sorted one-shot stop values inside their 30 % .. 70 % quantile range"""
    inner = np.sort(one[:, :-1].double().cpu().numpy().reshape(-1))
    mid = inner[int(0.3 * inner.size):int(0.7 * inner.size) + 1]
    gaps = np.diff(mid)
    g = int(gaps.argmax())
    return float((mid[g] + mid[g + 1]) / 2), float(gaps[g])


def pages_of(page):
    return [(t0, min(page, S - t0)) for t0 in range(0, S, page)]


def streamed(st, x, page, after=None, live_only=False):
    """-> stop (B,S), the last push's result"""
    stops, res = [], None
    for t0, c in pages_of(page):
        assert st.position == t0
        rows = x[:, t0:t0 + c]
        res = st.push(rows[st.live_lists().long()] if live_only else rows, live_only=live_only)
        stops.append(res["stop"])
        if after is not None:
            after(t0 + c, res)
    return torch.cat(stops, 1), res


def rows_restated(want, page, below=1.0):
    """the rows the GEMMs run over when compact() follows every push: slots on entry to each page, times its ranks"""
    want = np.asarray(want)
    slots, rows = B, 0
    for t0, c in pages_of(page):
        rows += c * slots
        live = int((want > t0 + c).sum())                  # a list is undecided after the page iff its cut lies behind it
        if live < slots and live <= below * slots:
            slots = live
    return rows


@pytest.mark.parametrize("mode", ("fp32", "bf16x6", "bf16x3"))
def test_compacted_stream_cuts_stops_rows_and_live_lists(N, mode):
    from rlt_hip import ops
    m, x, stop64 = setup()
    with ops.precision(mode):
        one = m.stop_probabilities(x)
        d_one = float(np.abs(one.double().cpu().numpy() - stop64).max())
        tau, gap = tau_in_a_gap(one)
        want = m.truncate(x, rule="above", tau=tau)
        want_h = want.cpu().numpy()
        assert len(set(want_h.tolist())) > 1, want                      # at least two lists stop on different pages (of 1 rank)
        d_stream = 0.0
        for page in PAGES:
            plain_read = m.stream(tau, B)
            plain_stop, plain = streamed(plain_read, x, page)
            st = m.stream(tau, B, compact_every=1)

            def after(pos, res, st=st):
                undecided = np.flatnonzero(want_h > pos).astype(np.int32)
                assert st.live_lists().cpu().numpy().tolist() == undecided.tolist(), pos
                assert st.compact() == undecided.size and st.slots == undecided.size          # a second compact: nothing left to move
                assert res["active"].cpu().numpy().tolist() == (want_h > pos).tolist()

            stop, res = streamed(st, x, page, after)
            assert st.position == S and not bool(res["active"].any())
            assert torch.equal(res["k"], want) and torch.equal(st.k, want), (mode, page, res["k"], want)
            # the NaN pattern and documents_read are those of the uncompacted stream
            assert torch.equal(torch.isnan(stop), torch.isnan(plain_stop)) and torch.equal(plain["k"], want)
            assert torch.equal(st.documents_read(), plain_read.documents_read())
            assert torch.equal(st.documents_read().long(), ((want.long() + page - 1) // page * page).clamp(max=S))
            done = ~torch.isnan(stop)
            d = float(np.abs(stop.double().cpu().numpy() - stop64)[done.cpu().numpy()].max())
            print(f"  {mode} page {page}: max|compacted stream - f64| = {d:.3e}, max|one-shot - f64| = {d_one:.3e}, "
                  f"bit-equal to the uncompacted stream: {torch.equal(stop[done].view(torch.int32), plain_stop[done].view(torch.int32))}")
            assert d <= max(4 * d_one, 2.0 ** -22), (mode, page, d, d_one)
            d_stream = max(d_stream, d)
            # the rows the GEMMs and LayerNorms ran over
            entry = sum(c * int((want_h > t0).sum()) for t0, c in pages_of(page))
            assert st.rows_computed() == entry == rows_restated(want_h, page), (page, st.rows_computed(), entry)
            assert plain_read.rows_computed() == S * B
            if min((int(k) - 1) // page for k in want_h) < (S - 1) // page:   # a list stops before the last page: its later pages are saved
                assert st.rows_computed() < S * B, page
            else:
                assert page == S and st.rows_computed() == S * B              # one page holds the whole list: nothing to save
            if page == 1:
                assert st.rows_computed() == int(want_h.sum())
            # reset() reproduces the run bit for bit
            st.reset()
            assert st.position == 0 and st.slots == B and bool((st.k == 0).all()) and st.rows_computed() == 0
            assert st.live_lists().tolist() == list(range(B))
            again, res2 = streamed(st, x, page)
            assert torch.equal(again.view(torch.int32), stop.view(torch.int32)) and torch.equal(res2["k"], want)
            assert st.rows_computed() == entry
        assert gap > 2 * max(d_stream, d_one), (gap, d_stream, d_one)


def test_compact_below_waits_until_half_have_retired(N):
    m, x, _ = setup()
    tau, _ = tau_in_a_gap(m.stop_probabilities(x))
    want = m.truncate(x, rule="above", tau=tau)
    want_h = want.cpu().numpy()
    for page in (1, 10):
        st = m.stream(tau, B, compact_every=1, compact_below=0.5)
        seen = []
        _, res = streamed(st, x, page, lambda pos, res: seen.append(st.slots))
        assert torch.equal(res["k"], want)
        assert st.rows_computed() == rows_restated(want_h, page, 0.5), (page, st.rows_computed())
        assert rows_restated(want_h, page) <= st.rows_computed() <= S * B
        assert all(b == a or 2 * b <= a for a, b in zip([B] + seen, seen)), seen       # every move at least halves the slots
        # compact_every = 3: compact() runs after the third, sixth, .. push only
        st3 = m.stream(tau, B, compact_every=3)
        slots3 = []
        _, res3 = streamed(st3, x, page, lambda pos, res: slots3.append(st3.slots))
        assert torch.equal(res3["k"], want)
        assert all(slots3[i] == (slots3[i - 1] if i else B) for i in range(len(slots3)) if (i + 1) % 3)


def test_live_only_pushes_give_the_bits_of_full_batch_pushes(N):
    m, x, _ = setup()
    tau, _ = tau_in_a_gap(m.stop_probabilities(x))
    for page in (1, 10, 32):
        full, res_f = streamed(m.stream(tau, B, compact_every=1), x, page)
        live, res_l = streamed(m.stream(tau, B, compact_every=1), x, page, live_only=True)
        assert torch.equal(full.view(torch.int32), live.view(torch.int32))
        assert torch.equal(res_f["k"], res_l["k"]) and torch.equal(res_f["active"], res_l["active"])
    st = m.stream(tau, B, compact_every=1)
    with pytest.raises(ValueError):
        st.push(x[:2, :4], live_only=True)


def test_a_stream_with_every_list_retired_takes_pushes_and_launches_nothing(N, monkeypatch):
    from rlt_hip import ops
    m, x, _ = setup()
    st = m.stream(0.0, B, compact_every=1)                  # tau = 0: every list stops at its first rank
    res = st.push(x[:, :10])
    assert res["k"].tolist() == [1] * B and not bool(res["active"].any()) and bool(torch.isfinite(res["stop"]).all())
    assert st.slots == 0 and st.live_lists().numel() == 0 and st.compact() == 0

    class Counter:
        launches = []

        def timed(self, name, fn):
            self.launches.append(name)
            fn()

    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(ops.KernelTimer, "active", Counter())
    for t0, c in ((10, 10), (20, 1), (21, 49)):
        assert st.position == t0
        res = st.push(x[:, t0:t0 + c])
        assert res["k"].tolist() == [1] * B and not bool(res["active"].any()) and bool(torch.isnan(res["stop"]).all())
        assert res["stop"].shape == (B, c)
    assert st.position == S and Counter.launches == [] and calls == []
    assert st.rows_computed() == 10 * B and st.documents_read().tolist() == [10] * B and st.k.tolist() == [1] * B
    monkeypatch.undo()
    # the hook does count: an uncompacted push launches
    monkeypatch.setattr(ops.KernelTimer, "active", Counter())
    m.stream(0.0, B).push(x[:, :1])
    assert "seq_attn_append" in Counter.launches and "hazard_append" in Counter.launches


def test_without_compact_every_the_truncator_is_the_old_one(N):
    from utils.stream import StreamingTruncator
    m, x, _ = setup()
    tau, _ = tau_in_a_gap(m.stop_probabilities(x))
    for page in (10, 32):
        old, res_o = streamed(StreamingTruncator(m, tau, B), x, page)
        new, res_n = streamed(m.stream(tau, B, compact_every=None, compact_below=0.25), x, page)
        assert torch.equal(old.view(torch.int32), new.view(torch.int32)) and torch.equal(res_o["k"], res_n["k"])
    st = m.stream(tau, B)
    st.push(x[:, :32])
    assert st.slots == B and st._spare is None and st.k is st._k and st.rows_computed() == 32 * B       # nothing was allocated or moved
    # an explicit compact() on it works: the plan, the read, the move
    n = st.compact()
    assert n == int(st.active.sum()) == st.slots
    for kw in ({"compact_every": 0}, {"compact_every": -1}, {"compact_every": 1, "compact_below": 1.5}):
        with pytest.raises(ValueError):
            m.stream(tau, B, **kw)


def test_run_py_stream_compact(N, tmp_path):
    import run
    from dataloader.synth import write_synthetic_robust04
    base = str(tmp_path / "data")
    write_synthetic_robust04(base, "robust04", "drmm_tks", n_train=16, n_test=8, seed=3, seq_len=40)
    common = ["--model-name", "choopy", "--dataset-base", base, "--use-conf", "0", "--batch-size", "8", "--seed", "1", "--epochs", "1",
              "--tensorboard-dir", ""]
    online = ["--attention-axis", "position", "--attention-mask", "causal", "--cut-head", "hazard"]
    hist, hist_c = str(tmp_path / "h.json"), str(tmp_path / "hc.json")
    run.main(common + online + ["--stream-eval", "10", "--stream-tau", "0.05", "--history-json", hist])
    run.main(common + online + ["--stream-eval", "10", "--stream-tau", "0.05", "--stream-compact", "1", "--history-json", hist_c])
    h, hc = json.load(open(hist)), json.load(open(hist_c))
    assert not [k for k in h if k.startswith(("stream_compact", "stream_rows"))]
    assert hc["stream_compact"] == 1 and hc["stream_compact_below"] == 1.0 and hc["stream_rows_full"] == 40.0
    assert 10.0 <= hc["stream_rows"] <= hc["stream_rows_full"]
    print(f"  stream_k {hc['stream_k']}, stream_read {hc['stream_read']}, stream_rows {hc['stream_rows']} of {hc['stream_rows_full']}")
    for key in ("stream_k", "stream_f1", "stream_dcg", "stream_read", "stream_page", "stream_tau", "stream_lists"):
        assert hc[key] == h[key], (key, hc[key], h[key])
    assert hc["stream_rows"] == hc["stream_read"]            # compacted after every page: a list costs exactly the pages it read
    with pytest.raises(SystemExit):
        run.main(common + online + ["--stream-compact", "1"])
    with pytest.raises(SystemExit):
        run.main(common + online + ["--stream-eval", "10", "--stream-compact", "1", "--stream-compact-below", "2"])
