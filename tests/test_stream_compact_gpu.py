"""rlt_stream_compact_plan and rlt_kv_cache_compact (csrc/stream_compact.hip) through the raw C ABI (`pytest -m gpu`), against the
numpy restatement tests/stream_compact_restate.py.  Zero tolerance everywhere: every comparison is np.array_equal on integer views.

  plan         B at the wavefront and workgroup-chunk edges x eight retirement patterns; active values 2 and -1 count as live; origin a
               permutation into a longer k_full, and NULL; carry with NaN payloads and -0.0; k_full pre-filled with a sentinel; an
               out-of-range origin is skipped; guard words behind every output; two calls give the same bits
  cache gather W x t0 x B_src with B_dst from the patterns; src tags (rank, list, column) in its bits, NaN payloads among them; dst
               pre-filled with a sentinel: rows >= t0*B_dst and the guard rows keep it, src is unchanged, a map entry of -1 leaves its rows
  continuity   lists appended to rank t0, caches and carry compacted with the two calls, further chunks appended at B_dst: out, lse,
               the cache rows, stop, z, p and carry of every surviving list equal the uncompacted stream (same qkv rows, an `active`
               mask instead of the compaction) bit for bit - the append and hazard kernels do not depend on B or on a list's slot"""
import functools

import numpy as np
import pytest
import torch

import stream_compact_restate as R

pytestmark = pytest.mark.gpu
PLAN_B = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
PATTERNS = ("all", "none", "alternating", "first_half_retired", "second_half_retired", "only_last", "only_first", "random_half")
GUARD = 8
SENT = -77


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


def pattern(name, B, seed=5):
    a = np.zeros(B, np.int32)
    if name == "all":
        a[:] = 1
    elif name == "alternating":
        a[1::2] = 1
    elif name == "first_half_retired":
        a[B // 2:] = 1
    elif name == "second_half_retired":
        a[:B // 2] = 1
    elif name == "only_last":
        a[-1] = 1
    elif name == "only_first":
        a[0] = 1
    elif name == "random_half":
        a[np.random.default_rng(seed + B).permutation(B)[:B // 2]] = 1
    return a


def guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device=dev())


def run_plan(N, active, origin, carry, k, k_full0, B_full):
    """-> the outputs as numpy arrays, guard words included"""
    from rlt_hip.native import ptr
    B = active.shape[0]
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    a_d, o_d, c_d, k_d = d(active), d(origin), d(carry), d(k)
    slot_src, origin_out = guarded(B, torch.int32, SENT), guarded(B, torch.int32, SENT)
    carry_out = None if carry is None else guarded(B, torch.float64, float(SENT))
    k_full = None if k is None else torch.cat([d(k_full0), torch.full((GUARD,), SENT, dtype=torch.int32, device=dev())])
    n_live = guarded(1, torch.int32, SENT)
    N.call("rlt_stream_compact_plan", ptr(a_d), ptr(o_d), ptr(c_d), ptr(k_d), B, B_full, ptr(slot_src), ptr(origin_out), ptr(carry_out),
           ptr(k_full), ptr(n_live), N.stream())
    for t, ref in ((a_d, active), (o_d, origin), (c_d, carry), (k_d, k)):                # the inputs are read only
        if t is not None:
            assert np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))
    return {n: None if t is None else t.cpu().numpy() for n, t in
            (("slot_src", slot_src), ("origin", origin_out), ("carry", carry_out), ("k_full", k_full), ("n_live", n_live))}


def check_plan(got, want, B, B_full):
    n = want["n_live"]
    assert got["n_live"][0] == n and (got["n_live"][1:] == SENT).all()
    for name in ("slot_src", "origin"):
        assert np.array_equal(got[name][:B], want[name]), name
        assert (got[name][B:] == SENT).all(), name + " guard"
    if want["carry"] is not None:
        assert np.array_equal(got["carry"][:n].view(np.uint64), want["carry"].view(np.uint64))
        assert (got["carry"][n:] == float(SENT)).all()                                    # behind n_live: untouched, and the guard
    if want["k_full"] is not None:
        assert np.array_equal(got["k_full"][:B_full], want["k_full"]) and (got["k_full"][B_full:] == SENT).all()


def special_carry(B, rng):
    c = -rng.random(B) * 40.0
    bits = c.view(np.uint64)
    bits[::5] = np.uint64(0x7FF8000000000000) | rng.integers(1, 1 << 40, size=bits[::5].shape, dtype=np.uint64)      # quiet NaNs with payloads
    bits[3::11] = np.uint64(0x7FF0000000000000) | rng.integers(1, 1 << 40, size=bits[3::11].shape, dtype=np.uint64)   # signalling ones
    c[1::7] = -0.0
    return c


# ------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("B", PLAN_B)
def test_plan_equals_the_restatement_on_every_pattern(N, B):
    rng = np.random.default_rng(100 + B)
    B_full = B + 5
    perm = rng.permutation(B_full)[:B].astype(np.int32)
    carry = special_carry(B, rng)
    k = rng.integers(1, 300, B).astype(np.int32)
    k_full0 = np.full(B_full, -5, np.int32)
    for name in PATTERNS:
        active = pattern(name, B)
        live = np.flatnonzero(active)
        active[live[::3]] = 2                                                             # any non-zero value is live
        active[live[1::3]] = -1
        for origin, bf, kf0 in ((perm, B_full, k_full0), (None, B, k_full0[:B])):
            want = R.plan(active, origin, carry, k, kf0)
            got = run_plan(N, active, origin, carry, k, kf0, bf)
            check_plan(got, want, B, bf)
            assert want["n_live"] == int((pattern(name, B) != 0).sum())
            # only the retired lists' entries of k_full changed
            org = np.arange(B, dtype=np.int32) if origin is None else origin
            changed = np.flatnonzero(got["k_full"][:bf] != -5)
            assert set(changed.tolist()) == set(org[active == 0].tolist())
            again = run_plan(N, active, origin, carry, k, kf0, bf)
            for key in got:
                assert np.array_equal(got[key].view(np.uint8), again[key].view(np.uint8)), (name, key)
        # the optional pairs left out
        got = run_plan(N, active, None, None, None, None, B)
        check_plan(got, R.plan(active), B, B)


def test_plan_skips_an_origin_out_of_range_and_takes_b_full_from_the_argument(N):
    active = np.array([0, 1, 0, 0, 0, 1, 0], np.int32)
    origin = np.array([3, 2, -1, 9, 8, 100, 0], np.int32)          # B_full = 9: -1 and 9 are outside, 8 is the last inside
    k = np.array([11, 12, 13, 14, 15, 16, 17], np.int32)
    k_full0 = np.full(9, -5, np.int32)
    want = R.plan(active, origin, None, k, k_full0)
    assert want["k_full"].tolist() == [17, -5, -5, 11, -5, -5, -5, -5, 15]
    got = run_plan(N, active, origin, None, k, k_full0, 9)
    check_plan(got, want, 7, 9)
    assert got["origin"][:2].tolist() == [2, 100]                   # a live slot's origin is copied as it is
    # with B_full = 8 the entry 8 is outside too: the ninth word is not written although the buffer has it
    got = run_plan(N, active, origin, None, k, k_full0, 8)
    assert got["k_full"][:9].tolist() == [17, -5, -5, 11, -5, -5, -5, -5, -5]


# ------------------------------------------------------------------------------------------------ 2. the cache gather
@functools.lru_cache(maxsize=None)
def tagged(t0, B_src, W):
    """(t0*B_src, W) float32 whose bits tag (rank, list, column); every seventh column holds the tag as a NaN payload, and the
    first column of odd lists is -0.0 / +0.0 by rank parity"""
    s, b, c = np.meshgrid(np.arange(t0, dtype=np.uint32), np.arange(B_src, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    tag = (s << 19) | (b << 11) | c
    bits = np.where(c % 7 == 3, np.uint32(0x7FC00000) | (tag & np.uint32(0x3FFFFF)), tag)
    bits = np.where((c == 0) & (b % 2 == 1), np.where(s % 2 == 0, np.uint32(0x80000000), np.uint32(0)), bits)
    out = bits.astype(np.uint32).reshape(t0 * B_src, W).view(np.float32)
    out.setflags(write=False)
    return out


def run_gather(N, src_d, slot_src, t0, B_src, B_dst, W, rows_behind=3):
    """dst has rows_behind more ranks' worth of rows and GUARD guard rows, all at the sentinel -> dst as numpy"""
    from rlt_hip.native import ptr
    dst = torch.full(((t0 + rows_behind) * max(B_dst, 1) + GUARD, W), float(SENT), dtype=torch.float32, device=dev())
    m = torch.from_numpy(np.ascontiguousarray(slot_src)).to(dev())
    N.call("rlt_kv_cache_compact", ptr(src_d), ptr(dst), ptr(m), t0, B_src, B_dst, W, N.stream())
    return dst.cpu().numpy()


@pytest.mark.parametrize("B_src", (6, 65, 130))
@pytest.mark.parametrize("t0", (1, 33, 70))
@pytest.mark.parametrize("W", (32, 256, 512, 2048))
def test_cache_gather_equals_the_restatement(N, W, t0, B_src):
    src = tagged(t0, B_src, W)
    src_d = torch.from_numpy(src).to(dev())
    # at the largest shapes three of the eight patterns (the host comparison of 70 MB arrays is what takes the time, not the launch)
    names = PATTERNS if t0 * B_src * W <= 1 << 22 else ("alternating", "all", "only_last")
    for name in names:
        active = pattern(name, B_src)
        p = R.plan(active)
        B_dst = p["n_live"]
        got = run_gather(N, src_d, p["slot_src"], t0, B_src, B_dst, W)
        blank = np.full(got.shape, float(SENT), np.float32)
        want = R.gather_cache(src, p["slot_src"], t0, B_src, B_dst, blank)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, B_dst)
        assert (got[t0 * B_dst:] == float(SENT)).all()                                    # rows >= t0*B_dst and the guard rows
        if B_dst:
            assert np.array_equal(got[:t0 * B_dst].view(np.uint32).reshape(t0, B_dst, W),
                                  src.view(np.uint32).reshape(t0, B_src, W)[:, p["slot_src"][:B_dst]])
    assert np.array_equal(src_d.cpu().numpy().view(np.uint32), src.view(np.uint32))       # src is not written


@pytest.mark.parametrize("W,t0,B_src", [(32, 33, 65), (256, 70, 6), (2048, 3, 130)])
def test_a_map_entry_out_of_range_leaves_its_rows_and_two_calls_agree(N, W, t0, B_src):
    src = tagged(t0, B_src, W)
    src_d = torch.from_numpy(src).to(dev())
    B_dst = B_src - 1
    m = np.random.default_rng(W).permutation(B_src)[:B_dst].astype(np.int32)             # any order, not only an ascending map
    m[0], m[B_dst // 2], m[-1] = -1, B_src, -(2 ** 31)
    got = run_gather(N, src_d, m, t0, B_src, B_dst, W)
    blank = np.full(got.shape, float(SENT), np.float32)
    want = R.gather_cache(src, m, t0, B_src, B_dst, blank)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    rows = got[:t0 * B_dst].reshape(t0, B_dst, W)
    assert (rows[:, [0, B_dst // 2, B_dst - 1]] == float(SENT)).all() and not (rows[:, 1] == float(SENT)).any()
    again = run_gather(N, src_d, m, t0, B_src, B_dst, W)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_the_python_wrappers(N):
    from rlt_hip import ops
    active = torch.tensor([1, 0, 2, 0, 1], dtype=torch.int32, device=dev())
    carry = torch.tensor([-1.0, -2.0, -3.0, -4.0, -5.0], dtype=torch.float64, device=dev())
    k = torch.tensor([0, 4, 0, 9, 0], dtype=torch.int32, device=dev())
    k_full = torch.zeros(5, dtype=torch.int32, device=dev())
    p = ops.stream_compact_plan(active, None, carry, k, k_full)
    assert p["n_live"].tolist() == [3] and p["slot_src"].tolist() == [0, 2, 4, -1, -1] and p["origin"].tolist() == [0, 2, 4, -1, -1]
    assert p["carry"][:3].tolist() == [-1.0, -3.0, -5.0] and k_full.tolist() == [0, 4, 0, 9, 0]
    src = torch.from_numpy(tagged(3, 5, 32).copy()).to(dev())
    dst = torch.full((3 * 3 + 2, 32), float(SENT), device=dev())
    ops.kv_cache_compact(src, dst, p["slot_src"], 3, 5, 3)
    assert torch.equal(dst[:9].view(torch.int32).view(3, 3, 32), src.view(torch.int32).view(3, 5, 32)[:, [0, 2, 4]]) and bool((dst[9:] == SENT).all())
    for bad in (lambda: ops.stream_compact_plan(active.float()), lambda: ops.stream_compact_plan(active, carry=carry.float()),
                lambda: ops.stream_compact_plan(active, k=k), lambda: ops.stream_compact_plan(active, k=k, k_full=k),
                lambda: ops.stream_compact_plan(active, origin=k[:4]), lambda: ops.kv_cache_compact(src, dst, p["slot_src"], 3, 3, 5),
                lambda: ops.kv_cache_compact(src, dst[:5], p["slot_src"], 3, 5, 3), lambda: ops.kv_cache_compact(src, dst, p["slot_src"].long(), 3, 5, 3),
                lambda: ops.kv_cache_compact(src, dst[:, :16].contiguous(), p["slot_src"], 3, 5, 3)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.kv_cache_compact(src, src, p["slot_src"], 3, 5, 3)                            # in place: the library refuses the overlap


# ------------------------------------------------------------------------------------------------ 3. continuity
S, LISTS = 70, 6
RETIRE = (1, 2, 4)
SECOND_AT, SECOND_RETIRE = 66, (3,)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


def chunks_through(events, page):
    """pages of `page` ranks, cut where an event falls"""
    marks = sorted(set(events) | {S})
    out, t = [], 0
    for m in marks:
        while t < m:
            out.append(min(page, m - t))
            t += out[-1]
    return out


def run_stream(N, qkv, w, bias, H, HD, page, events, compact):
    """events {t0: lists to retire on entry to rank t0}.  compact: take them out with the two calls; else clear their `active`.
    -> per-list results in list order (NaN where a list was not computed), the final caches' rows per list, the carry per list"""
    from rlt_hip.native import ptr
    E = H * HD
    B = LISTS
    q3 = qkv.view(S, B, 3 * E)
    slots = list(range(B))
    retired = set()
    cache = nan(S * B, 2 * E)
    carry = torch.zeros(B, dtype=torch.float64, device=dev())
    out, lse = nan(S, B, E), nan(B, H, S)
    stop, z, p = nan(B, S), nan(B, S), nan(B, S)
    k_all = torch.zeros(B, dtype=torch.int32, device=dev())
    t0 = 0
    for c in chunks_through(events, page):
        if t0 in events:
            retired |= set(events[t0])
            if compact:
                Bs = len(slots)
                act = torch.tensor([0 if o in retired else 1 for o in slots], dtype=torch.int32, device=dev())
                org = torch.tensor(slots, dtype=torch.int32, device=dev())
                slot_src, org_out = torch.empty_like(act), torch.empty_like(act)
                carry_out, n_live = torch.empty_like(carry), torch.empty(1, dtype=torch.int32, device=dev())
                N.call("rlt_stream_compact_plan", ptr(act), ptr(org), ptr(carry), None, Bs, B, ptr(slot_src), ptr(org_out), ptr(carry_out),
                       None, ptr(n_live), N.stream())
                n = int(n_live.item())
                new_cache = nan(S * n, 2 * E)
                N.call("rlt_kv_cache_compact", ptr(cache), ptr(new_cache), ptr(slot_src), t0, Bs, n, 2 * E, N.stream())
                slots, cache, carry = org_out[:n].tolist(), new_cache, carry_out[:n].clone()
        Bs = len(slots)
        idx = torch.tensor(slots, device=dev())
        chunk = q3[t0:t0 + c, idx].reshape(c * Bs, 3 * E).contiguous()
        act = torch.tensor([0 if o in retired else 1 for o in slots], dtype=torch.int32, device=dev())
        o, l = nan(c * Bs, E), nan(Bs, H, c)
        N.call("rlt_seq_attention_append", ptr(chunk), ptr(cache), t0, c, S, Bs, H, HD, ptr(act), ptr(o), ptr(l), N.PRECISION_DEFAULT, N.stream())
        hs, hz, hp = nan(Bs, c), nan(Bs, c), nan(Bs, c)
        hact, hk = act.clone(), torch.zeros(Bs, dtype=torch.int32, device=dev())
        N.call("rlt_hazard_head_append", ptr(o), ptr(w), ptr(bias), None, t0, c, Bs, E, int(t0 + c == S), ptr(carry), 2.0, ptr(hact), ptr(hk),
               ptr(hs), ptr(hp), ptr(hz), N.stream())
        out[t0:t0 + c, idx] = o.view(c, Bs, E)
        lse[idx, :, t0:t0 + c] = l
        stop[idx, t0:t0 + c], z[idx, t0:t0 + c], p[idx, t0:t0 + c] = hs, hz, hp
        k_all[idx] = hk
        t0 += c
    rows = nan(S, B, 2 * E)
    rows[:, torch.tensor(slots, device=dev())] = cache.view(S, len(slots), 2 * E)
    car = nan(B, dtype=torch.float64)
    car[torch.tensor(slots, device=dev())] = carry
    res = {"out": out, "lse": lse, "stop": stop, "z": z, "p": p, "cache": rows, "carry": car, "k": k_all}
    return {n: t.cpu().numpy() for n, t in res.items()}


def bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("page", (1, 10, 32))
@pytest.mark.parametrize("t0c", (31, 32, 33, 64))
@pytest.mark.parametrize("HD,H", [(16, 4), (64, 1)])
def test_a_compacted_stream_continues_bit_for_bit(N, HD, H, t0c, page):
    E = H * HD
    g = torch.Generator().manual_seed(1000 * HD + t0c)
    qkv = torch.randn(S * LISTS, 3 * E, generator=g).to(dev())
    w, bias = (0.3 * torch.randn(E, generator=g)).to(dev()), torch.tensor([0.1], device=dev())
    events = {t0c: RETIRE, SECOND_AT: SECOND_RETIRE}                   # the second compaction works on the already compacted stream
    ref = run_stream(N, qkv, w, bias, H, HD, page, events, compact=False)
    got = run_stream(N, qkv, w, bias, H, HD, page, events, compact=True)
    left = {b: S for b in range(LISTS)}
    left.update({b: t0c for b in RETIRE})
    left.update({b: SECOND_AT for b in SECOND_RETIRE})
    for b, t in left.items():                                          # every list, over the ranks it was computed for
        assert np.isfinite(ref["out"][:t, b]).all() and np.isfinite(ref["stop"][b, :t]).all(), b
        assert np.array_equal(bits(got["out"][:t, b]), bits(ref["out"][:t, b])), ("out", b)
        assert np.array_equal(bits(got["lse"][b, :, :t]), bits(ref["lse"][b, :, :t])), ("lse", b)
        for name in ("stop", "z", "p"):
            assert np.array_equal(bits(got[name][b, :t]), bits(ref[name][b, :t])), (name, b)
            assert np.isnan(got[name][b, t:]).all() and np.isnan(ref[name][b, t:]).all(), (name, b)
    survivors = [b for b, t in left.items() if t == S]
    assert survivors == [0, 5]
    assert np.array_equal(bits(got["cache"][:, survivors]), bits(ref["cache"][:, survivors]))          # K | V of all 70 ranks
    assert np.array_equal(bits(got["carry"][survivors]), bits(ref["carry"][survivors])) and np.isfinite(ref["carry"][survivors]).all()
    assert got["k"][survivors].tolist() == [S, S] and ref["k"][survivors].tolist() == [S, S]               # `final` stopped them
    assert float(ref["stop"][survivors, -1].min()) == 1.0
