"""rlt_hazard_head_append (csrc/hazard.hip) through the raw C ABI against rlt_hazard_head_fwd on the same x: the hazard head fed a
chunk of positions at a time, its survival sum carried from chunk to chunk, the stop decision taken on the device.

  stop, z    bit-equal to the one-shot call on every row, whatever the chunking
  p          bit-equal too: the last row is the remainder, so it matches under `final` and is not forced without it
  carry      after the last chunk: - sum_j softplus(z_j) of tests/hazard_restate.py on the device's z, to 1e-12 relative
  decision   k and active agree with ops.cut_sweep(stop, tau, 'above') on the one-shot stop, for a tau below every stop, one above
             every stop (only `final` stops the list) and one exactly equal to a stop value
  retired    a list retired in an earlier chunk keeps its k and carry, and its output rows keep their NaN sentinel"""
import functools

import numpy as np
import pytest
import torch

import hazard_restate as H

pytestmark = pytest.mark.gpu
S_SET = (1, 2, 63, 64, 65, 300)
E_SET = (64, 128, 256)
B_SET = (1, 5)
SHAPES = [(S, B, E) for S in S_SET for B in B_SET for E in E_SET]
ids = lambda s: "S%d-B%d-E%d" % s


def chunkings(S):
    def fixed(c):
        return [min(c, S - t) for t in range(0, S, c)]
    uneven, t = [], 0
    for c in (3, 61, 1, 70, S):
        if t < S:
            uneven.append(min(c, S - t))
            t += uneven[-1]
    return {"ones": fixed(1), "sevens": fixed(7), "64s": fixed(64), "whole": [S], "uneven": uneven}


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def operands(shape):
    """x (S*B, E) with a drift along the list so that the stop probabilities spread, w, b, the prior offset"""
    S, B, E = shape
    rng = np.random.default_rng([11, S, B, E])
    w = (rng.standard_normal(E) / np.sqrt(E)).astype(np.float32)
    x = rng.standard_normal((S, B, E)).astype(np.float32)
    x += (np.linspace(-2.0, 2.0, S)[:, None, None] * w[None, None, :] / float(w @ w)).astype(np.float32)      # z drifts from -2 to 2
    b = np.array([0.25], dtype=np.float32)
    off = H.prior_offset(S).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (x.reshape(S * B, E), w, b, off))


def one_shot(N, shape, with_offset):
    S, B, E = shape
    x, w, b, off = operands(shape)
    p, stop, z = nan(B, S), nan(B, S), nan(B, S)
    N.call("rlt_hazard_head_fwd", N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(off if with_offset else None), S, B, E, N.ptr(p), N.ptr(stop),
           N.ptr(z), N.stream())
    return p, stop, z


def append_all(N, shape, chunks, with_offset, tau=2.0, decide=False, final_at_end=True, trace=None):
    """-> p, stop, z (B,S), carry (B,) float64, active, k (B,) int32 - every output starts as NaN / 0; trace(t0, c, state) behind
    every chunk"""
    S, B, E = shape
    x, w, b, off = operands(shape)
    p, stop, z = nan(B, S), nan(B, S), nan(B, S)
    carry = torch.zeros(B, dtype=torch.float64, device="cuda")
    active = torch.ones(B, dtype=torch.int32, device="cuda") if decide else None
    k = torch.zeros(B, dtype=torch.int32, device="cuda") if decide else None
    t0 = 0
    for c in chunks:
        pc, sc, zc = nan(B, c), nan(B, c), nan(B, c)
        final = int(final_at_end and t0 + c == S)
        N.call("rlt_hazard_head_append", N.ptr(x[t0 * B:(t0 + c) * B]), N.ptr(w), N.ptr(b), N.ptr(off[t0:t0 + c] if with_offset else None),
               t0, c, B, E, final, N.ptr(carry), float(tau), N.ptr(active), N.ptr(k), N.ptr(sc), N.ptr(pc), N.ptr(zc), N.stream())
        p[:, t0:t0 + c], stop[:, t0:t0 + c], z[:, t0:t0 + c] = pc, sc, zc
        if trace is not None:
            trace(t0, c, carry.clone(), active.clone(), k.clone())
        t0 += c
    return p, stop, z, carry, active, k


def bits(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the values
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_every_chunking_gives_the_one_shot_bits(N, shape):
    S, B, E = shape
    with_offset = (S + E // 64) % 2 == 0                    # both forms over the shapes
    p1, s1, z1 = one_shot(N, shape, with_offset)
    assert bool(torch.isfinite(p1).all()) and bool((s1[:, -1] == 1).all())
    sp = H.terms(z1.cpu().numpy())[0]
    for name, chunks in chunkings(S).items():
        p, stop, z, carry, _, _ = append_all(N, shape, chunks, with_offset)
        assert np.array_equal(bits(z), bits(z1)), (name, "z")
        assert np.array_equal(bits(stop), bits(s1)), (name, "stop")
        assert np.array_equal(bits(p), bits(p1)), (name, "p", float((p - p1).abs().max()))
        want = -sp.sum(1)
        assert np.all(np.abs(carry.cpu().numpy() - want) <= 1e-12 * np.abs(want)), (name, "carry")


@pytest.mark.parametrize("shape", [(65, 5, 128), (2, 1, 64)], ids=ids)
def test_the_last_row_is_not_forced_without_final(N, shape):
    S, B, E = shape
    p1, s1, z1 = one_shot(N, shape, True)
    for chunks in (chunkings(S)["whole"], chunkings(S)["ones"]):
        p, stop, z, carry, _, _ = append_all(N, shape, chunks, True, final_at_end=False)
        assert np.array_equal(bits(z), bits(z1))
        assert np.array_equal(bits(stop[:, :-1]), bits(s1[:, :-1])) and np.array_equal(bits(p[:, :-1]), bits(p1[:, :-1]))
        _, logsig, h, _ = H.terms(z1.cpu().numpy()[:, -1])
        assert np.array_equal(stop[:, -1].cpu().numpy(), h.astype(np.float32)) and bool((stop[:, -1] < 1).all())
        L = np.log(p1.cpu().numpy()[:, -1].astype(np.float64))          # the one-shot remainder is exp(L_{S-1})
        inner = np.exp(logsig + L)
        assert np.all(np.abs(p[:, -1].cpu().numpy() - inner) <= 4 * H.ulp32(inner) + 2.0 ** -24 * inner)


# ------------------------------------------------------------------------------------------------ 2. the decision
@pytest.mark.parametrize("shape", [(300, 5, 128), (65, 5, 64), (64, 1, 256), (1, 5, 64)], ids=ids)
def test_the_decision_is_cut_sweeps_above_rule(N, shape):
    from rlt_hip import ops
    S, B, E = shape
    _, s1, _ = one_shot(N, shape, True)
    inner = s1[:, :-1] if S > 1 else s1
    exact = float(s1[B // 2, min(S // 3, S - 1)])                       # one list stops at exactly this value
    taus = {"below": float(inner.min()) / 2, "above": 1.5, "exact": exact}
    for tname, tau in taus.items():
        thr = torch.full((1,), tau, dtype=torch.float64, device="cuda")
        want = ops.cut_sweep(s1, thr, "above")[0].reshape(-1).cpu().numpy()
        if tname == "below":
            assert (want == 1).all()
        if tname == "above":
            assert (want == S).all()
        for name, chunks in chunkings(S).items():
            seen = []
            append_all(N, shape, chunks, True, tau=tau, decide=True, trace=lambda t0, c, carry, active, k: seen.append((t0, c, carry, active, k)))
            t0, c, _, active, k = seen[-1]
            assert np.array_equal(k.cpu().numpy(), want), (tname, name)
            assert not active.any()                                      # `final` stops whatever is left
            for t0, c, _, active, k in seen[:-1]:                        # active exactly while the cut lies behind the chunk
                assert np.array_equal(active.cpu().numpy() != 0, want > t0 + c), (tname, name, t0)
                assert np.array_equal(k.cpu().numpy(), np.where(want <= t0 + c, want, 0)), (tname, name, t0)


def test_a_retired_list_keeps_k_carry_and_its_sentinel_rows(N):
    shape = S, B, E = (300, 5, 128)
    x, w, b, off = operands(shape)
    _, s1, _ = one_shot(N, shape, True)
    tau = float(s1[:, :-1].median())
    carry = torch.zeros(B, dtype=torch.float64, device="cuda")
    active = torch.ones(B, dtype=torch.int32, device="cuda")
    k = torch.zeros(B, dtype=torch.int32, device="cuda")
    retired_seen = 0
    for t0 in range(0, S, 20):
        before = carry.clone(), active.clone(), k.clone()
        pc, sc, zc = nan(B, 20), nan(B, 20), nan(B, 20)
        N.call("rlt_hazard_head_append", N.ptr(x[t0 * B:(t0 + 20) * B]), N.ptr(w), N.ptr(b), N.ptr(off[t0:t0 + 20]), t0, 20, B, E,
               int(t0 + 20 == S), N.ptr(carry), tau, N.ptr(active), N.ptr(k), N.ptr(sc), N.ptr(pc), N.ptr(zc), N.stream())
        gone = (before[1] == 0).cpu().numpy()
        retired_seen += int(gone.sum())
        for out in (pc, sc, zc):
            o = out.cpu().numpy()
            assert np.isnan(o[gone]).all() and np.isfinite(o[~gone]).all()
        assert torch.equal(carry[gone], before[0][gone]) and torch.equal(k[gone], before[2][gone])
        assert bool((carry[~gone] < before[0][~gone]).all())
        assert not active[gone].any()
    assert retired_seen > 0 and not active.any()


def test_the_python_wrapper(N):
    from rlt_hip import ops
    shape = S, B, E = (65, 5, 128)
    x, w, b, off = operands(shape)
    _, s1, z1 = one_shot(N, shape, True)
    carry = torch.zeros(B, dtype=torch.float64, device="cuda")
    a = ops.hazard_head_append(x[:40 * B], w, b, 0, B, carry, offset=off[:40], want_z=True)
    c = ops.hazard_head_append(x[40 * B:], w, b, 40, B, carry, offset=off[40:], final=True, want_z=True, want_p=True)
    assert torch.equal(torch.cat([a["stop"], c["stop"]], 1), s1) and torch.equal(torch.cat([a["z"], c["z"]], 1), z1)
    assert a["p"] is None and c["p"] is not None
    with pytest.raises(ValueError):
        ops.hazard_head_append(x[:40 * B], w, b, 0, B, carry.float())
    with pytest.raises(ValueError):
        ops.hazard_head_append(x[:40 * B], w, b, 0, B, carry, active=torch.ones(B, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.hazard_head_append(x[:40 * B], w, b, 0, B, carry, offset=off)
