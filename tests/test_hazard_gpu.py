"""rlt_hazard_head_fwd / rlt_hazard_head_bwd (csrc/hazard.hip) through the raw C ABI against tests/hazard_restate.py (float64
numpy, pinned to torch float64 autograd by tests/test_hazard_restate.py).  `pytest -m gpu`.

What is held to what (u = 2^-24, the unit roundoff of fp32; ulp(v) = the spacing of fp32 at |v|):

    z          exact operands (small integers x powers of two: every partial sum is exact): equal to the float64 dot.  Random
               operands: |z - z64| <= E u sum_i |x_i w_i| + |b| u (+ |offset_s| u with an offset: one more fp32 add), the fp32
               summation bound, computed from the operands.
    p, stop    against the restatement applied to the DEVICE's z: 1 ulp (the float64 chain's error is S O(2^-53), only the final
               rounding is left); where |p| is below the normal range, 2^-126 absolute (a subnormal may be flushed).
    dx         against fp32(dz) w (+ the prior value under accumulate_dx), dz the restatement's on the device's z: 2 ulp of the
               larger of the product and the result (half an ulp each for the product and the add, one for a dz that rounds the
               other way), plus 2^-126 |w| for a subnormal dz.
    dw, db     sums of S B terms in fp32, in the kernel's order: (S B + 3) u sum |dz x| and (S B + 2) u sum |dz| (any order of n
               additions is within (n-1) u of the sum of magnitudes to first order; one u for each product's rounding, two for
               dz's last bit).

Every output lies between NaN guard rows; a store outside its array shows.  Each test prints its worst error as a multiple of the
bound; over the 108 shapes an MI355X gave z 0.05, p and stop 0.5 (correctly rounded), dx 0.25 (half an ulp), dw 0.21, db 0.05."""
import functools

import numpy as np
import pytest
import torch

import hazard_restate as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
GUARD = 64                                    # floats: 256 bytes, keeps the 16-byte alignment of what follows

S_SET = (1, 2, 63, 64, 65, 128, 129, 300, 1024)
B_SET = (1, 3, 5)
E_SET = (64, 128, 256, 1024)                  # V1-nch1, V2-nch1, V4-nch1, V4-nch4


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rlt_hip import native
    native.load()
    return native


class Guarded:
    """n floats between two rows of NaN"""

    def __init__(self, n, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        if fill is not None:
            self.buf[GUARD:GUARD + n] = dev(fill).reshape(-1)

    def ptr(self, N):
        return N.ptr(self.buf[GUARD:])

    def get(self, what):
        h = self.buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + self.n:]).all(), f"{what}: written outside its {self.n} elements"
        return h[GUARD:GUARD + self.n].copy()


def dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32)).cuda()          # (a copy: the shared operands are read-only)


def fwd(N, x, w, b, off, S, B, E, want_stop=True):
    """x (S*B,E), w (E), b (1), off (S) or None, numpy float32 -> p, stop (or None), z as (B,S) numpy float32"""
    xd, wd, bd = dev(x), dev(w), dev(b)
    od = dev(off) if off is not None else None
    p, z = Guarded(B * S), Guarded(B * S)
    stop = Guarded(B * S) if want_stop else None
    N.call("rlt_hazard_head_fwd", N.ptr(xd), N.ptr(wd), N.ptr(bd), N.ptr(od), S, B, E, p.ptr(N),
           stop.ptr(N) if want_stop else None, z.ptr(N), N.stream())
    torch.cuda.synchronize()
    return (p.get("p").reshape(B, S), stop.get("stop").reshape(B, S) if want_stop else None, z.get("z").reshape(B, S))


def bwd(N, x, w, z, dp, dstop, S, B, E, dx0=None):
    """-> dx (S*B,E), dw (E), db (1); dx0: the prior value, which selects accumulate_dx"""
    xd, wd, zd, dpd = dev(x), dev(w), dev(z), dev(dp)
    dsd = dev(dstop) if dstop is not None else None
    dx, dw, db = Guarded(S * B * E, dx0), Guarded(E), Guarded(1)
    ws_bytes = N.query("rlt_hazard_head_bwd_workspace", S, B, E)
    assert ws_bytes == B * (E + 4) * 4
    ws = Guarded(ws_bytes // 4)
    N.call("rlt_hazard_head_bwd", N.ptr(xd), N.ptr(wd), N.ptr(zd), N.ptr(dpd), N.ptr(dsd), S, B, E, dx.ptr(N),
           int(dx0 is not None), dw.ptr(N), db.ptr(N), ws.ptr(N), ws_bytes, N.stream())
    torch.cuda.synchronize()
    ws.get("workspace")
    return dx.get("dx").reshape(S * B, E), dw.get("dw"), db.get("db")


@functools.lru_cache(maxsize=None)
def operands(S, B, E):
    g = np.random.default_rng(1000003 * S + 1009 * B + E)
    x = g.standard_normal((S * B, E)).astype(np.float32)
    w = (g.standard_normal(E) / np.sqrt(E)).astype(np.float32)
    b = g.standard_normal(1).astype(np.float32)
    dp, dstop = g.standard_normal((B, S)).astype(np.float32), g.standard_normal((B, S)).astype(np.float32)
    dx0 = g.standard_normal((S * B, E)).astype(np.float32)
    for a in (x, w, b, dp, dstop, dx0):
        a.setflags(write=False)
    return x, w, b, dp, dstop, dx0


def z64(x, w, b, off, S, B, E):
    """the float64 logits (B,S) and the magnitude sums sum_i |x_i w_i| (B,S)"""
    x3 = x.astype(np.float64).reshape(S, B, E)
    w8 = w.astype(np.float64)
    z = (x3 @ w8).T + float(b[0])
    if off is not None:
        z = z + off.astype(np.float64)[None, :]
    return z, (np.abs(x3) @ np.abs(w8)).T


class Worst:
    def __init__(self):
        self.w = {}

    def add(self, what, err, bound):
        """err, bound: arrays; keeps the largest err / bound"""
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        self.w[what] = max(self.w.get(what, 0.0), ratio)

    def done(self, case):
        print(f"  {case}: worst error as a multiple of its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in self.w.items()))
        over = {k: v for k, v in self.w.items() if not v <= 1.0}
        assert not over, (case, over)


def check_p_stop(t, p, stop, z):
    p_ref, stop_ref = H.forward(z)
    t.add("p", np.abs(p - p_ref), np.where(p_ref < TINY, TINY, H.ulp32(p_ref)))
    if stop is not None:
        t.add("stop", np.abs(stop - stop_ref), np.where(stop_ref < TINY, TINY, H.ulp32(stop_ref)))
        assert (stop[:, -1] == 1.0).all()


def check_bwd(t, x, w, z, dp, dstop, S, B, E, dx, dw, db, dx0):
    dz = H.backward(z, dp, dstop).astype(np.float32).astype(np.float64)               # fp32(dz), (B,S)
    assert (dz[:, -1] == 0.0).all()
    dz_pm = dz.T.reshape(S * B, 1)                                                     # row s * B + b
    w8, x8 = w.astype(np.float64)[None, :], x.astype(np.float64)
    prod = dz_pm * w8
    ref = prod + (dx0.astype(np.float64) if dx0 is not None else 0.0)
    t.add("dx+=" if dx0 is not None else "dx", np.abs(dx - ref), 2 * H.ulp32(np.maximum(np.abs(prod), np.abs(ref))) + TINY * np.abs(w8))
    t.add("dw", np.abs(dw - (dz_pm * x8).sum(0)), (S * B + 3) * U * (np.abs(dz_pm) * np.abs(x8)).sum(0))
    t.add("db", np.abs(db - dz.sum()), np.array([(S * B + 2) * U * np.abs(dz).sum()]))
    if S == 1:
        assert not dw.any() and not db.any()


@pytest.mark.parametrize("E", E_SET)
@pytest.mark.parametrize("B", B_SET)
@pytest.mark.parametrize("S", S_SET)
def test_forward_and_backward_against_the_restatement(N, S, B, E):
    x, w, b, dp, dstop, dx0 = operands(S, B, E)
    off = H.prior_offset(S).astype(np.float32)
    t = Worst()
    p, stop, z = fwd(N, x, w, b, off, S, B, E)
    zr, mag = z64(x, w, b, off, S, B, E)
    t.add("z", np.abs(z - zr), E * U * mag + abs(float(b[0])) * U + np.abs(off)[None, :] * U)
    check_p_stop(t, p, stop, z)
    assert np.abs(p.astype(np.float64).sum(1) - 1.0).max() <= (S + 1) * U          # S roundings of values that sum to 1
    for prior in (None, dx0):
        dx, dw, db = bwd(N, x, w, z, dp, dstop, S, B, E, prior)
        check_bwd(t, x, w, z, dp, dstop, S, B, E, dx, dw, db, prior)
    t.done(f"S{S} B{B} E{E}")


@pytest.mark.parametrize("E", E_SET)
@pytest.mark.parametrize("S,B", [(1, 1), (65, 3), (300, 5), (1024, 1)])
def test_exact_operands_give_the_float64_dot(N, S, B, E):
    """x small integers, w signed powers of two, b and the offset multiples of 1/8: every product and partial sum is exact in fp32"""
    g = np.random.default_rng(S * 31 + E)
    x = g.integers(-4, 5, size=(S * B, E)).astype(np.float32)
    w = (g.choice([-1.0, 1.0], size=E) * 2.0 ** g.integers(-3, 1, size=E)).astype(np.float32)
    b = np.array([0.625], dtype=np.float32)
    for off in (None, (g.integers(-40, 41, size=S) / 8.0).astype(np.float32)):
        _, _, z = fwd(N, x, w, b, off, S, B, E)
        zr, _ = z64(x, w, b, off, S, B, E)
        assert np.array_equal(z.astype(np.float64), zr), (S, B, E, off is None)


@pytest.mark.parametrize("level", [40.0, 100.0])
def test_saturated_logits(N, level):
    """z = +-40 / +-100 through b and through the offset (w = 0, so z = b + offset exactly): no NaN, p exactly 0 or correctly
    rounded, finite gradients, the last position holds the remainder"""
    S, B, E = 65, 3, 64
    x = operands(S, B, E)[0]
    w = np.zeros(E, dtype=np.float32)
    ones = np.ones((B, S), dtype=np.float32)
    pattern = np.array([-level, level, 0.0, -level, -level, level, 40.0, -40.0], dtype=np.float32)
    cases = [(np.array([v], dtype=np.float32), None) for v in (level, -level)]
    cases += [(np.zeros(1, dtype=np.float32), np.resize(pattern[r:], S).astype(np.float32)) for r in (0, 1, 2)]
    cases += [(np.array([-level], dtype=np.float32), np.where(np.arange(S) == 40, 2 * level, 0.0).astype(np.float32))]
    for b, off in cases:
        p, stop, z = fwd(N, x, w, b, off, S, B, E)
        assert np.array_equal(z, np.broadcast_to(b[0] + (off if off is not None else np.zeros(S, dtype=np.float32)), (B, S)))
        assert np.isfinite(p).all() and np.isfinite(stop).all()
        p_ref, stop_ref = H.forward(z)
        rounded = p_ref.astype(np.float32)
        ok = (p == rounded) | ((p == 0.0) & (p_ref < TINY))
        assert ok.all(), (b, p[~ok], p_ref[~ok])
        assert np.abs(stop - stop_ref).max() <= 2.0 ** -24 and (stop[:, -1] == 1.0).all()
        rest = 1.0 - p_ref[:, :-1].sum(1)
        assert np.abs(p[:, -1] - rest).max() <= (S + 1) * U and abs(p.astype(np.float64).sum(1) - 1.0).max() <= (S + 1) * U
        for ds in (ones, None):
            dx, dw, db = bwd(N, x, w, z, ones, ds, S, B, E)
            assert np.isfinite(dx).all() and np.isfinite(dw).all() and np.isfinite(db).all()
            assert np.abs(db[0] - H.backward(z, ones, ds).sum()) <= (S * B + 2) * U * np.abs(H.backward(z, ones, ds)).sum() + 1e-30


@pytest.mark.parametrize("S", [65, 300])
def test_prefix_property_to_the_bit(N, S):
    """rows > i of one list replaced: z, stop and p at positions <= i, and every other list, keep their bits; with dp and dstop zero
    beyond i, dx at rows > i is exactly 0"""
    B, E = 3, 128
    x, w, b, dp, dstop, _ = operands(S, B, E)
    off = H.prior_offset(S).astype(np.float32)
    base = fwd(N, x, w, b, off, S, B, E)
    other = np.random.default_rng(S).standard_normal((S, E)).astype(np.float32) * 3.0 + 1.0
    for i in (0, 62, 63, 64, S - 2):
        x2 = x.copy().reshape(S, B, E)
        x2[i + 1:, 1, :] = other[i + 1:]
        x2 = x2.reshape(S * B, E)
        got = fwd(N, x2, w, b, off, S, B, E)
        for name, a, c in zip(("p", "stop", "z"), base, got):
            assert np.array_equal(a[1, :i + 1].view(np.uint32), c[1, :i + 1].view(np.uint32)), (name, i)
            assert np.array_equal(a[[0, 2]].view(np.uint32), c[[0, 2]].view(np.uint32)), (name, i)
            if name == "z" and i + 1 < S:
                assert not np.array_equal(a[1, i + 1:], c[1, i + 1:]), i                   # (the replacement did reach the head)
        dp2, ds2 = dp.copy(), dstop.copy()
        dp2[:, i + 1:] = 0.0
        ds2[:, i + 1:] = 0.0
        dx, _, _ = bwd(N, x2, w, got[2], dp2, ds2, S, B, E)
        assert not dx.reshape(S, B, E)[i + 1:].any(), i
        assert dx.reshape(S, B, E)[:i + 1].any()


@pytest.mark.parametrize("S,B,E", [(129, 3, 128), (300, 5, 256)])
def test_null_pointers_and_repeatability(N, S, B, E):
    """every combination of offset, stop and dstop present / NULL against the restatement; a second call gives the same bits"""
    x, w, b, dp, dstop, dx0 = operands(S, B, E)
    t = Worst()
    for off in (None, H.prior_offset(S).astype(np.float32)):
        for want_stop in (False, True):
            p, stop, z = fwd(N, x, w, b, off, S, B, E, want_stop)
            zr, mag = z64(x, w, b, off, S, B, E)
            t.add("z", np.abs(z - zr), E * U * mag + abs(float(b[0])) * U + (np.abs(off)[None, :] * U if off is not None else 0.0))
            check_p_stop(t, p, stop, z)
            again = fwd(N, x, w, b, off, S, B, E, want_stop)
            for a, c in zip((p, stop, z), again):
                assert (a is None and c is None) or np.array_equal(a.view(np.uint32), c.view(np.uint32))
            for ds in (None, dstop):
                out = bwd(N, x, w, z, dp, ds, S, B, E, dx0 if want_stop else None)
                check_bwd(t, x, w, z, dp, ds, S, B, E, *out, dx0 if want_stop else None)
                again = bwd(N, x, w, z, dp, ds, S, B, E, dx0 if want_stop else None)
                for a, c in zip(out, again):
                    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    t.done(f"S{S} B{B} E{E}")
