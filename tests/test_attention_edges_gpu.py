"""Every eval-mode list-attention kernel at its own tile edges, through the raw C ABI, against float64 on the device.

  grid        one id per (precision, head dim, B, S, H), drop_p = 0: the values of B that leave a 64- / 128-row tile or a 256-query
              workgroup filled by 1, 15, 17, 63, 65 ... rows, below and above the 512-list threshold of the pipelined kernels, and
              eight-pair ids for the XCD-swizzled branch of map_block.  The kernel of every part is taken from
              tests/attn_plan_restate.plan and asserted on native.attention_plan before the launch; no environment switch is read
              or set.  test_edges_grid_reaches_every_kernel (host only) pins what the grid reaches.
  inputs      every id runs three inputs (make_inputs): `plain` randn; `last_key`, where key B - 1 carries 0.3 .. 0.9 of most
              queries' softmax weight; `neighbour`, where the first 64 rows of position s + 1 - the rows a ragged last tile of
              position s reads when it fails to mask - are dominant keys for position s's queries.  The host-only test checks in
              float64 that dropping key B - 1, or admitting the neighbour's rows, moves the reference by more than 100 x the
              forward tolerance.  qkv and dout live in NaN-guarded buffers like every output.
  compared    out, dQ, dK, dV: relative max-norm, 1e-5 forward and 3e-5 gradients, 6 x in bf16x3 mode (the tolerances of
              tests/test_attention_dispatch_gpu.py); lse and delta against the two derived bounds at lse_bound / delta_check.
  fix-up      the pipelined forwards' flag words are read back from `images`: all zero for the three inputs above and for a falling
              score ramp, exactly one pair's workgroups for a steeply rising ramp in that pair (test_fixup_*).
  parts       _bwd_prepare -> _bwd_dkv -> _bwd_dq, _bwd_prepare -> _bwd_dq -> _bwd_dkv and rlt_list_attention_bwd are bit-identical;
              each part writes its own columns only (test_backward_parts_in_any_order).

Input constants.  Planted rows scaled by 8 would dominate too, but rounding errors of a score grow with |q| |k| / sqrt(HD) (the
`sharp` case of tools/gpu_probe.py needs 2e-5 at 4 x randn), so the inputs here get their dominance from ALIGNMENT instead: Q
carries a common component along a unit vector w of its pair, and the planted keys lie along w.  |q| |k| / sqrt(HD) stays within 4 x
that of randn, and the sensitivity conditions hold with two orders of magnitude to spare (printed by the host-only test)."""
import functools
import math

import pytest
import torch

import attn_plan_restate as AP
import dropout_restate as D
from test_dropout_gpu import REACHED as TRAIN_REACHED, single_list_floors

GUARD = 256          # sentinel floats behind every buffer
S_ALL = 2
P_DROP = 0.3
SEED = 4321
KINDS = ("plain", "last_key", "neighbour")
NEIGHBOUR_ROWS = 64

# ------------------------------------------------------------------------------------------------ the grid
BELOW_512 = (1, 15, 17, 63, 64, 65, 127, 129, 255, 257, 448)
HEAD_DIMS = {"fp32": (16, 32, 64, 128), "bf16x3": (16, 32, 64), "bf16x6": (16, 32, 64)}
# (precision, HD, B, S, H)
GRID = [(prec, HD, B, S_ALL, 2) for HD in (16, 32, 64, 128) for B in BELOW_512 for prec in HEAD_DIMS if HD in HEAD_DIMS[prec]]
GRID += [("bf16x6", 16, B, S_ALL, 2) for B in (512, 513, 527, 529, 575, 577, 640, 703, 768)]
GRID += [("bf16x6", 64, B, S_ALL, 2) for B in (512, 576, 704, 768, 513, 520, 575, 577)]
EIGHT_PAIRS = [("bf16x6", 16, 512, S_ALL, 4), ("bf16x6", 64, 512, S_ALL, 4), ("bf16x6", 64, 576, S_ALL, 4),
               ("bf16x6", 32, 130, S_ALL, 4), ("fp32", 32, 130, S_ALL, 4)]
GRID += EIGHT_PAIRS
# the pipelined forwards and their fix-up launch: every grid id whose plan names one, and x6h_pipe in train mode
FIXUP = [c + (0.0,) for c in GRID if AP.plan(c[3], c[2], c[4], c[1], 0.0, 1, c[0])["fwd_fixup"] != "none"]
FIXUP += [("bf16x6", 64, B, S_ALL, 2, P_DROP) for B in (512, 576)]
# one id per backward kernel code
ORDER = [("fp32", 16, 65, S_ALL, 2), ("fp32", 32, 129, S_ALL, 2), ("fp32", 128, 65, S_ALL, 2), ("bf16x3", 32, 129, S_ALL, 2),
         ("bf16x6", 32, 129, S_ALL, 2), ("bf16x6", 16, 257, S_ALL, 2), ("bf16x6", 16, 577, S_ALL, 2), ("bf16x6", 16, 512, S_ALL, 4),
         ("bf16x6", 64, 257, S_ALL, 2), ("bf16x6", 64, 577, S_ALL, 2)]
# what eval mode reaches under the default switches: the train-mode sets (tests/test_dropout_gpu.py) with the pipelined head-dim-16
# kernels, which only eval mode has, in place of the seeded two-wavefront backward, which 512 lists and more take in train mode only
EVAL_REACHED = {"fwd": TRAIN_REACHED["fwd"] | {"x6n_pipe"},
                "dkv": (TRAIN_REACHED["dkv"] - {"x6n_2w_seeded"}) | {"x6n_pipe"},
                "dq": (TRAIN_REACHED["dq"] - {"x6n_2w_seeded"}) | {"x6n_pipe"}}


def case_id(c):
    return f"{c[0]}-hd{c[1]}-B{c[2]}" + ("" if c[4] == 2 else f"-H{c[4]}") + (f"-p{c[5]}" if len(c) > 5 and c[5] else "")


def tols(prec):
    scale = 6.0 if prec == "bf16x3" else 1.0
    return {"fwd": 1e-5 * scale, "dq": 3e-5 * scale, "dk": 3e-5 * scale, "dv": 3e-5 * scale}


# the steep pair (tools/gpu_probe.py: attention, "steeply rising"): at a score of 280 one fp32 ulp of the score is 3e-5, and the
# weights of the top keys carry that as a relative error whatever the kernel does.  The probe's forward bound for that input is
# 2e-4, twenty times the project's 1e-5.  dK and dV are linear in those weights, so the same factor of twenty on the project's
# 3e-5 is their bound: 6e-4 (the probe itself allows 1e-3, over dQ | dK | dV together).  Measured in the steep pair: dK 8.3e-6 ..
# 8.4e-5, dV 2.2e-5 .. 4.7e-5 - above 3e-5 under every kernel, x6_dkv1 and x6n_pipe alike.  dQ of the steep pair has no max-norm
# bound: see steep_dq_check.  The steep pair's lse keeps the eps of its mode: lse_bound scales with the score by itself.
STEEP_SPAN = 280.0
STEEP_TOLS = {"fwd": 2e-4, "dq": None, "dk": 6e-4, "dv": 6e-4}
STEEP_SCORE_EPS = 2.0 * 2.0 ** -15          # two fp32 ulps of a score of 280 (steep_dq_check)


def map_block(bid, npair, ntile):
    """csrc/attention_common.h: flat block id -> (pair, row tile)"""
    if npair & 7 == 0:
        xcd, j = bid & 7, bid >> 3
        return (j // ntile) * 8 + xcd, j % ntile
    return bid // ntile, bid % ntile


def steep_pair(npair):
    """Not pair 0.  With eight pairs the swizzled map gives EVERY pair one block among the first eight, so no pair stays out of
    that group; pair 5 is the choice whose blocks under the swizzle (5 and 13 with two row tiles) share nothing with its blocks
    under the plain map (10 and 11): a fix-up launch that mapped its blocks the other way would redo the wrong rows."""
    return 5 if npair == 8 else npair - 2


# ------------------------------------------------------------------------------------------------ inputs
Q_COMMON = {"last_key": 8.0, "neighbour": 2.0}          # length of the common component of a pair's Q rows
NEIGHBOUR_K = 2.0                                       # planted keys: randn + NEIGHBOUR_K * sqrt(HD) * w
NEIGHBOUR_V = 4.0
LAST_KEY_MEDIAN = 0.6                                   # the median softmax weight of key B - 1 over a pair's queries


def pair_view(t, S, B, H, HD):
    """(S * B, n * H * HD) position-major -> (n, S, H, B, HD) view"""
    return t.view(S, B, -1, H, HD).permute(2, 0, 3, 1, 4)


@functools.lru_cache(maxsize=8)
def make_inputs(kind, S, B, H, HD):
    """-> (qkv, dout) float32 on the host; shared between the tests, never modified"""
    g = torch.Generator().manual_seed(B * 131 + HD * 7 + H)
    E = H * HD
    qkv, dout = torch.randn(S * B, 3 * E, generator=g), torch.randn(S * B, E, generator=g)
    if kind == "plain":
        return qkv, dout
    w = torch.nn.functional.normalize(torch.randn(S, H, HD, generator=g), dim=-1)
    q, k, v = pair_view(qkv, S, B, H, HD)
    q += Q_COMMON[kind] * w[:, :, None, :]
    if kind == "last_key":
        # K row B - 1 = c * (the unit mean direction of the pair's Q rows), V row B - 1 = 4.  The key's weight for query i is
        # sigmoid(c a_i - L_i), a_i = q_i . u / sqrt(HD), L_i = the logsumexp of the other keys' scores: c by bisection, per pair.
        qd, kd = q.double(), k.double()
        u = torch.nn.functional.normalize(qd.mean(2), dim=-1)                                   # (S, H, HD)
        a = (qd @ u[..., None])[..., 0] / math.sqrt(HD)                                         # (S, H, B)
        if B > 1:
            L = torch.logsumexp(qd @ kd[:, :, :B - 1].transpose(-1, -2) / math.sqrt(HD), -1)
            lo, hi = torch.zeros(S, H, dtype=torch.float64), torch.full((S, H), 64.0 * math.sqrt(HD), dtype=torch.float64)
            for _ in range(50):
                c = (lo + hi) / 2
                above = torch.sigmoid(c[..., None] * a - L).median(-1).values > LAST_KEY_MEDIAN
                lo, hi = torch.where(above, lo, c), torch.where(above, c, hi)
            c = (lo + hi) / 2
        else:
            c = torch.ones(S, H, dtype=torch.float64)
        k[:, :, B - 1] = (c[..., None] * u).float()
        v[:, :, B - 1] = 4.0
    else:
        n = min(NEIGHBOUR_ROWS, B)
        k[1:, :, :n] += NEIGHBOUR_K * math.sqrt(HD) * w[:-1, :, None, :]
        v[1:, :, :n] *= NEIGHBOUR_V
    return qkv, dout


def ramp_inputs(S, B, H, HD, span, with_ramp=True):
    """randn everywhere; in the steep pair Q = 1 + 0.01 randn and K = the ramp of tools/gpu_probe.py, scores from 0 to `span`"""
    g = torch.Generator().manual_seed(B * 131 + HD * 7 + H + 1)
    E = H * HD
    qkv, dout = torch.randn(S * B, 3 * E, generator=g), torch.randn(S * B, E, generator=g)
    if with_ramp:
        q, k, _ = pair_view(qkv, S, B, H, HD)
        s, h = divmod(steep_pair(S * H), H)
        ramp = torch.linspace(0.0, 1.0, B).view(B, 1)
        q[s, h] = 1.0 + 0.01 * torch.randn(B, HD, generator=g)
        k[s, h] = ramp * (span / math.sqrt(HD)) + 0.01 * torch.randn(B, HD, generator=g)
    return qkv, dout


# ------------------------------------------------------------------------------------------------ reference and bounds
def reference(qkv, dout, S, B, H, HD, mask=None, keys=None):
    """float64 wherever qkv lives -> out (S * B, E), dqkv (S * B, 3E), lse (S, H, B), the rows' largest |scaled score| (S, H, B) and
    softmax-weighted mean over their keys of sum_d |q_d k_d| / sqrt(HD) (S, H, B).
    mask: (S * H, B, B) keep mask of a train-mode call.  keys: (K, V) as (S, H, n, HD) to attend to instead of the call's own
    (the sensitivity conditions; no gradients then)."""
    E = H * HD
    x = pair_view(qkv.double(), S, B, H, HD).detach().clone().requires_grad_(keys is None)
    kk, vv = (x[1], x[2]) if keys is None else keys
    s = x[0] @ kk.transpose(-1, -2) / math.sqrt(HD)
    p = torch.softmax(s, -1)
    if mask is not None:
        p = p * torch.as_tensor(mask, device=qkv.device).double().reshape(S, H, B, B)
    o = (p @ vv).permute(0, 2, 1, 3).reshape(S * B, E)
    grad = None
    if keys is None:
        o.backward(dout.double())
        grad = x.grad.permute(1, 3, 0, 2, 4).reshape(S * B, 3 * E)
    abs_score = (torch.softmax(s.detach(), -1) * (x[0].detach().abs() @ kk.detach().abs().transpose(-1, -2))).sum(-1) / math.sqrt(HD)
    return o.detach(), grad, torch.logsumexp(s, -1).detach(), s.detach().abs().amax(-1), abs_score


def rel(a, b, floor=0.0):
    return float((a.double() - b).abs().max() / (max(float(b.abs().max()), floor) + 1e-30))


def errors(out, dqkv, ref, S, B, H, HD, pairs=None, floors=(0.0, 0.0)):
    """relative max-norm errors of out, dQ, dK, dV; pairs: a bool mask (S * H) restricting both norms to those pairs"""
    E = H * HD
    o_ref, g_ref = ref[0], ref[1]

    def sel(t, n):
        t = pair_view(t, S, B, H, HD)
        t = t if pairs is None else t.reshape(n, S * H, B, HD)[:, pairs]
        return t

    o, o_r = sel(out, 1), sel(o_ref, 1)
    g, g_r = sel(dqkv, 3), sel(g_ref, 3)
    return {"fwd": rel(o, o_r), "dq": rel(g[0], g_r[0], floors[0]), "dk": rel(g[1], g_r[1], floors[1]), "dv": rel(g[2], g_r[2])}


def ulp32(x):
    """the spacing of float32 at |x| (normal range)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


X3_SCORE_EPS = 3.0 * 2.0 ** -18


def lse_bound(lse_ref, score_max, fwd_tol, x3_abs_score=None):
    """lse = m + log l: a relative error eps in the normaliser l is an absolute error eps in lse, and eps is the forward tolerance
    of the mode - for every pair, the steep one included; plus 4 fp32 ulps at the larger of |lse| and the row's largest |scaled
    score| for the rounding of the scores, of m + log l and of the stored value.  Derived, not measured; per row.

    bf16x3 mode (x3_abs_score given: the row's softmax-weighted mean of sum_d |q_d k_jd| / sqrt(HD) over its keys j) - a property of
    the mode, not of a tile edge.  Its scores are not fp32-faithful: every operand is hi + lo of two bf16 (|lo| <= 2^-9 |x|, lo
    itself rounded: 2^-18 |x| lost) and the lo * lo product is dropped (<= 2^-18 |q_d k_d|), so score j is off by up to
    e_j = 3 * 2^-18 * sum_d |q_d k_jd| / sqrt(HD).  To first order lse moves by sum_j P_j (error of score j) <= sum_j P_j e_j: the
    errors of the keys that carry the weight, not of the row's worst key.  With plain randn that is about 3e-5 at head dim 16; where
    one key holds most of a row's weight (`last_key`) lse inherits that key's error undiminished.  Measured with the fp32-ulp term
    alone: 6.56e-5 at hd16 B63 and 7.40e-5 at hd16 B448, `last_key`, against 6.4e-5 (1.03 and 1.16 of the bound); every other id and
    input stayed within it.  The term below replaces nothing: it is added in bf16x3 mode only."""
    bound = fwd_tol + 4.0 * ulp32(torch.maximum(lse_ref.abs(), score_max))
    return bound if x3_abs_score is None else bound + X3_SCORE_EPS * x3_abs_score


def steep_dq_check(c, dqkv, ref, pair, mask):
    """dQ of the steep pair, element by element -> the largest error / bound.

    dQ_i = scale * sum_j dS_ij k_j with dS_ij = P_ij (dP_ij - delta_i) and sum_j dS_ij = 0.  On the ramp all keys that carry weight
    are nearly the same vector (70 per component at head dim 16, 0.14 apart), so the sum cancels to a few thousandths of its terms:
    dQ is ill-conditioned in the weights by design of the input.  sum_j dS_ij = 0 survives rounding only where the backward's
    weights are exactly those behind lse, out and delta.  A weight is exp(score - lse); a score of 280 rounded to fp32 is off by up
    to one ulp, 2^-15, and that is the weight's relative error.  Two roundings are independent of each other here: the score of the
    forward that produced out and so delta, and the score the backward recomputes - eps = STEEP_SCORE_EPS, two ulps.  Weights off
    by eps each, independently, move dQ_id by up to eps * scale * sum_j |dS_ij| |k_jd|.  That - plus the project's gradient
    tolerance of the pair's largest |dQ| for everything else - is the bound.  A kernel that recomputes exactly the forward's weights
    stays far below it (x6_dq1: 7e-5 of the largest |dQ|); x6n_pipe seeds its score accumulators with -lse and rounds the scores
    differently from the forward: 2.8e-3 .. 6.4e-3 of the largest |dQ| measured, about 0.3 of this bound."""
    S, B, H, HD = c.shape
    s, h = divmod(pair, H)
    q, k, v = pair_view(c.qkv.double(), S, B, H, HD)[:, s, h]
    do = pair_view(c.dout.double(), S, B, H, HD)[0, s, h]
    p = torch.softmax(q @ k.t() / math.sqrt(HD), -1)
    dp = do @ v.t()
    if mask is not None:
        dp = dp * torch.as_tensor(mask[pair], device=dp.device).double()
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    got = pair_view(dqkv, S, B, H, HD)[0, s, h].double()
    want = pair_view(ref[1], S, B, H, HD)[0, s, h]
    bound = STEEP_SCORE_EPS * (ds.abs() @ k.abs()) / math.sqrt(HD) + 3e-5 * want.abs().max()
    return float(((got - want).abs() / bound).max()), rel(got, want)


def delta_check(delta, out, dout, S, B, H, HD):
    """delta (S, H, B) against float64 rowsum(dout * out) of the device's own out; bound: a plain fp32 dot product of HD terms,
    HD * 2^-24 * sum |dout * out| per row -> the largest error / bound over the rows"""
    prod = pair_view(dout.double() * out.double(), S, B, H, HD)[0]                      # (S, H, B, HD)
    bound = HD * 2.0 ** -24 * prod.abs().sum(-1)
    err = (delta.double() - prod.sum(-1)).abs()
    return float((err / bound.clamp_min(1e-300)).max()), float(err.max())


# ------------------------------------------------------------------------------------------------ the device side
@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


def guarded(nbytes, guard=GUARD, fill=0.0):
    """float buffer of at least nbytes, NaN behind it -> (buffer, sentinel view)"""
    n = (max(int(nbytes), 16) + 3) // 4
    full = torch.full((n + guard,), float("nan"), device=dev())
    full[:n] = fill
    return full[:n], full[n:]


def intact(*ends):
    return all(bool(torch.isnan(e).all()) for e in ends)


class Call:
    """One (shape, precision, drop_p, input): the plan asserted, every buffer guarded - qkv and dout too, with the 64 rows a ragged
    tile of the last position may reach for behind them."""

    def __init__(self, N, prec, HD, B, S, H, drop_p, qkv, dout):
        self.N, self.shape, self.drop_p, self.code = N, (S, B, H, HD), drop_p, N.precision_code(prec)
        E = H * HD
        want = AP.plan(S, B, H, HD, drop_p, 1, prec)
        self.plan = plan = N.attention_plan(S, B, H, HD, drop_p, 1, self.code)
        for f in ("fwd", "fwd_fixup", "dkv", "dq", "images_bytes", "flags_offset", "images_retained", "ws_bytes"):
            assert plan[f] == want[f], (f, plan[f], want[f])
        self.ib, self.wb = plan["images_bytes"], plan["ws_bytes"]
        assert self.ib == N.query("rlt_list_attention_fwd_workspace", S, B, H, HD, drop_p, self.code)
        assert self.wb == N.query("rlt_list_attention_bwd_workspace", S, B, H, HD, drop_p, self.code)
        self.ends = []
        self.qkv = self.buf(4 * S * B * 3 * E, GUARD + NEIGHBOUR_ROWS * 3 * E).view(S * B, 3 * E)
        self.dout = self.buf(4 * S * B * E, GUARD + NEIGHBOUR_ROWS * E).view(S * B, E)
        self.qkv.copy_(qkv)
        self.dout.copy_(dout)
        self.out = self.buf(4 * S * B * E).view(S * B, E)
        self.lse = self.buf(4 * S * H * B).view(S, H, B)
        self.images = self.buf(self.ib)
        self.ws = self.buf(self.wb)
        self.img = N.ptr(self.images) if self.ib and plan["images_retained"] else None

    def buf(self, nbytes, guard=GUARD, fill=0.0):
        assert nbytes % 4 == 0          # whole floats: the sentinel starts at the buffer's last byte + 1
        b, end = guarded(nbytes, guard, fill)
        self.ends.append(end)
        return b[:int(nbytes) // 4] if nbytes >= 16 else b

    def forward(self, qkv=None, out=None, lse=None):
        N, (S, B, H, HD), ptr = self.N, self.shape, self.N.ptr
        N.call("rlt_list_attention_fwd", ptr(self.qkv if qkv is None else qkv), S, B, H, HD, self.drop_p, SEED,
               ptr(self.out if out is None else out), ptr(self.lse if lse is None else lse), ptr(self.images) if self.ib else None,
               self.ib, self.code, N.stream())

    def flags(self):
        S, B, H, _ = self.shape
        assert self.plan["fwd_fixup"] != "none" and self.plan["flags_offset"] % 4 == 0
        n = S * H * AP.cdiv(B, 256)
        assert self.plan["flags_offset"] + 4 * n <= self.ib
        torch.cuda.synchronize()
        return self.images.view(torch.int32)[self.plan["flags_offset"] // 4:][:n].cpu().tolist()

    def prepare(self, ws=None):
        N, (S, B, H, HD), ptr = self.N, self.shape, self.N.ptr
        N.call("rlt_list_attention_bwd_prepare", ptr(self.out), ptr(self.dout), ptr(self.lse), S, B, H, HD, self.drop_p, self.img,
               ptr(self.ws if ws is None else ws), self.wb, self.code, N.stream())

    def part(self, which, dqkv, ws=None):
        N, (S, B, H, HD), ptr = self.N, self.shape, self.N.ptr
        N.call("rlt_list_attention_bwd_" + which, ptr(self.qkv), ptr(self.dout), ptr(self.lse), self.img,
               ptr(self.ws if ws is None else ws), self.wb, S, B, H, HD, self.drop_p, SEED, ptr(dqkv), self.code, N.stream())

    def whole(self, dqkv, ws):
        N, (S, B, H, HD), ptr = self.N, self.shape, self.N.ptr
        N.call("rlt_list_attention_bwd", ptr(self.qkv), ptr(self.out), ptr(self.dout), ptr(self.lse), S, B, H, HD, self.drop_p, SEED,
               self.img, ptr(dqkv), ptr(ws), self.wb, self.code, N.stream())

    def new_dqkv(self, fill=0.0):
        S, B, H, HD = self.shape
        return self.buf(4 * S * B * 3 * H * HD, fill=fill).view(S * B, 3 * H * HD)

    def delta(self):
        S, B, H, _ = self.shape
        return self.ws[:S * H * B].view(S, H, B)

    def finish(self, *tensors):
        torch.cuda.synchronize()
        assert intact(*self.ends), "sentinel overwritten"
        for t in tensors:
            assert not bool(torch.isnan(t).any()), "NaN inside an output"


def run_all(N, prec, HD, B, S, H, drop_p, qkv, dout):
    """forward, prepare, dK+dV, dQ -> the call and dqkv"""
    c = Call(N, prec, HD, B, S, H, drop_p, qkv, dout)
    c.forward()
    c.prepare()
    dqkv = c.new_dqkv()
    c.part("dkv", dqkv)
    c.part("dq", dqkv)
    c.finish(c.out, c.lse, dqkv, c.delta())
    return c, dqkv


def check_call(name, c, dqkv, ref, prec, groups, mask=None):
    """groups: [(tag, bool mask over the pairs or None, tolerances)] -> asserts out / gradients per group, lse and delta per row"""
    S, B, H, HD = c.shape
    o_ref, _, lse_ref, score_max, abs_score = ref
    floors = single_list_floors(c.qkv, c.dout, H, HD, c.drop_p) if B == 1 else (0.0, 0.0)
    lse_err = (c.lse.double() - lse_ref).abs()
    lse_over = float((lse_err / lse_bound(lse_ref, score_max, tols(prec)["fwd"], abs_score if prec == "bf16x3" else None)).max())
    delta_over, delta_err = delta_check(c.delta(), c.out, c.dout, S, B, H, HD)
    line = f"{name} [{c.plan['fwd']}+{c.plan['fwd_fixup']} {c.plan['dkv']} {c.plan['dq']}]"
    failures = []
    for tag, pairs, t in groups:
        errs = errors(c.out, dqkv, ref, S, B, H, HD, pairs, floors)
        line += f" {tag}" + "".join(f" {k} {v:.2e}" for k, v in errs.items())
        failures += [(tag, k, errs[k], t[k]) for k in errs if t[k] is not None and not errs[k] <= t[k]]
        if t["dq"] is None:
            over, _ = steep_dq_check(c, dqkv, ref, int(pairs.nonzero()[0]), mask)
            line += f" ({over:.2f} of the dq bound)"
            failures += [(tag, "dq", errs["dq"], over)] if not over <= 1.0 else []
    print(line + f" lse {float(lse_err.max()):.2e} ({lse_over:.2f} of its bound) delta {delta_err:.2e} ({delta_over:.2f} of its bound)")
    assert not failures, failures
    assert lse_over <= 1.0, ("lse", float(lse_err.max()), lse_over)
    assert delta_over <= 1.0, ("delta", delta_err, delta_over)


# ------------------------------------------------------------------------------------------------ host only
def test_edges_grid_reaches_every_kernel():
    got, fixups, pipe_bwd_B, eight = {"fwd": set(), "dkv": set(), "dq": set()}, set(), set(), set()
    for prec, HD, B, S, H in GRID:
        p = AP.plan(S, B, H, HD, 0.0, 1, prec)
        for part in got:
            got[part].add(p[part])
        fixups.add((p["fwd"], p["fwd_fixup"]))
        if p["dkv"] == "x6n_pipe" and p["dq"] == "x6n_pipe" and B % 128 not in (0, 64):
            pipe_bwd_B.add(B)
        if S * H == 8:
            eight |= {p["fwd"], p["dkv"], p["dq"]}
    assert got == EVAL_REACHED, got
    assert ("x6h_pipe", "x6_pp") in fixups and ("x6n_pipe", "x6n_2w_seeded") in fixups
    assert len(pipe_bwd_B) >= 5, pipe_bwd_B
    assert {"x6n_pipe", "x6h_pipe"} <= eight and all(c in GRID for c in EIGHT_PAIRS)
    assert len(GRID) == len(set(GRID)) == 11 * 10 + 9 + 8 + 5
    # every kernel the dispatch test names in eval mode is reached in the same part
    from test_attention_dispatch_gpu import CASES, EXPECT
    for name, (part, prec, S, B, H, HD, drop_p) in CASES.items():
        if drop_p == 0:
            assert EXPECT.get(name, name) in got[part], name
    # the fix-up ids: every pipelined forward, eval and train; one order id per backward kernel code
    kinds = {(AP.plan(S, B, H, HD, p, 1, prec)["fwd"], p > 0, S * H) for prec, HD, B, S, H, p in FIXUP}
    assert {("x6n_pipe", False, 4), ("x6n_pipe", False, 8), ("x6h_pipe", False, 4), ("x6h_pipe", False, 8), ("x6h_pipe", True, 4)} == kinds
    order = [AP.plan(S, B, H, HD, 0.0, 1, prec) for prec, HD, B, S, H in ORDER]
    assert {p["dkv"] for p in order} == EVAL_REACHED["dkv"] and {p["dq"] for p in order} == EVAL_REACHED["dq"]
    assert all(c in GRID for c in ORDER)


@pytest.mark.parametrize("npair", (1, 2, 4, 8, 16))
@pytest.mark.parametrize("ntile", (1, 3))
def test_map_block_restatement_is_a_bijection(npair, ntile):
    seen = [map_block(bid, npair, ntile) for bid in range(npair * ntile)]
    assert sorted(seen) == [(p, t) for p in range(npair) for t in range(ntile)]
    if npair % 8 == 0:          # a pair's row tiles share bid & 7: one XCD
        assert all(len({bid & 7 for bid in range(npair * ntile) if map_block(bid, npair, ntile)[0] == p}) == 1 for p in range(npair))
    assert steep_pair(4) == 2 and steep_pair(8) == 5
    assert {b for b in range(16) if map_block(b, 8, 2)[0] == 5} == {5, 13}


@pytest.mark.parametrize("HD", (16, 64))
@pytest.mark.parametrize("B", (65, 513))
def test_inputs_make_the_edges_matter(B, HD):
    """A condition on the inputs, not on the kernels: in the module's own error metric, the float64 reference without key B - 1
    (`last_key`), or with the next position's first rows admitted as keys (`neighbour`: all 64, and the FIRST one alone), lies more
    than 100 x the widest forward tolerance (bf16x3: 6e-5) from the true one."""
    S, H = S_ALL, 2
    tol = max(tols(p)["fwd"] for p in HEAD_DIMS)
    qkv, dout = make_inputs("last_key", S, B, H, HD)
    true = reference(qkv, dout, S, B, H, HD)
    _, k, v = pair_view(qkv.double(), S, B, H, HD)
    moved = rel(reference(qkv, dout, S, B, H, HD, keys=(k[:, :, :B - 1], v[:, :, :B - 1]))[0], true[0])
    weight = torch.exp(pair_view(qkv.double(), S, B, H, HD)[0] @ k[:, :, B - 1:].transpose(-1, -2) / math.sqrt(HD) - true[2][..., None])
    inside = float(((weight > 0.3) & (weight < 0.9)).double().mean())
    print(f"last_key B{B} hd{HD}: without key B-1 {moved:.2e}; weight of key B-1 median {float(weight.median()):.2f}, {inside:.0%} in 0.3 .. 0.9")
    assert moved > 100 * tol and inside > 0.5
    assert float(true[1].abs().amax(0)[:H * HD].min()) > 1e-3          # dQ stays informative: no saturated softmax

    qkv, dout = make_inputs("neighbour", S, B, H, HD)
    true = reference(qkv, dout, S, B, H, HD)
    _, k, v = pair_view(qkv.double(), S, B, H, HD)
    for n in (NEIGHBOUR_ROWS, 1):
        # position s attends to its own keys plus the first n rows of position s + 1; the last position has no neighbour
        kk = torch.cat([k[:-1], k[1:, :, :n]], 2)
        vv = torch.cat([v[:-1], v[1:, :, :n]], 2)
        o = reference(qkv[:(S - 1) * B], dout[:(S - 1) * B], S - 1, B, H, HD, keys=(kk, vv))[0]
        moved = rel(o, true[0][:(S - 1) * B])
        print(f"neighbour B{B} hd{HD}: with {n} of the next position's rows as keys {moved:.2e}")
        assert moved > 100 * tol
    # rounding errors of a score grow with |q| |k| / sqrt(HD): per pair, the largest |q_i| |k_j| of either input within 4 x randn's
    def qk(kind):
        q, k, _ = pair_view(make_inputs(kind, S, B, H, HD)[0].double(), S, B, H, HD)
        return float((q.norm(dim=-1).amax(-1) * k.norm(dim=-1).amax(-1)).max())
    sizes = {kind: qk(kind) / qk("plain") for kind in ("last_key", "neighbour")}
    print(f"|q| |k| against randn B{B} hd{HD}:", {k_: f"{v:.2f}" for k_, v in sizes.items()})
    assert max(sizes.values()) < 4.0, sizes


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID, ids=[case_id(c) for c in GRID])
def test_eval_kernel_at_its_edges(N, case):
    prec, HD, B, S, H = case
    for kind in KINDS:
        qkv, dout = make_inputs(kind, S, B, H, HD)
        c, dqkv = run_all(N, prec, HD, B, S, H, 0.0, qkv, dout)
        ref = reference(c.qkv, c.dout, S, B, H, HD)
        check_call(f"{case_id(case)} {kind}", c, dqkv, ref, prec, [("", None, tols(prec))])
        if c.plan["fwd_fixup"] != "none":
            assert not any(c.flags()), (kind, c.flags())          # the numbers above are the pipelined kernel's own


# ------------------------------------------------------------------------------------------------ the fix-up path
@pytest.mark.gpu
@pytest.mark.parametrize("case", FIXUP, ids=[case_id(c) for c in FIXUP])
def test_fixup_redoes_exactly_the_steep_pair(N, case):
    prec, HD, B, S, H, drop_p = case
    npair, ntile, sp = S * H, AP.cdiv(B, 256), steep_pair(S * H)
    mask = D.attention_mask(SEED, S, B, H, drop_p) if drop_p > 0 else None
    others = torch.ones(npair, dtype=torch.bool, device=dev())
    others[sp] = False
    groups = [("steep pair:", ~others, STEEP_TOLS), ("other pairs:", others, tols(prec))]
    for kind in KINDS if drop_p > 0 else ():          # (the eval-mode ids run the benign inputs in the grid test)
        qkv, dout = make_inputs(kind, S, B, H, HD)
        c, dqkv = run_all(N, prec, HD, B, S, H, drop_p, qkv, dout)
        assert not any(c.flags()), (kind, c.flags())
        check_call(f"{case_id(case)} {kind}", c, dqkv, reference(c.qkv, c.dout, S, B, H, HD, mask), prec, [("", None, tols(prec))])
    for tag, span in (("rising", STEEP_SPAN), ("falling", -STEEP_SPAN)):
        qkv, dout = ramp_inputs(S, B, H, HD, span)
        c = Call(N, prec, HD, B, S, H, drop_p, qkv, dout)
        c.out.fill_(-12345.0)
        c.lse.fill_(-12345.0)
        c.forward()
        flags = c.flags()
        want = [int(span > 0 and map_block(bid, npair, ntile)[0] == sp) for bid in range(npair * ntile)]
        print(f"{case_id(case)} {tag}: flags {flags}")
        assert flags == want, (tag, flags, want)
        assert not bool((c.out == -12345.0).any()) and not bool((c.lse == -12345.0).any())          # every row written
        c.prepare()
        dqkv = c.new_dqkv()
        c.part("dkv", dqkv)
        c.part("dq", dqkv)
        c.finish(c.out, c.lse, dqkv, c.delta())
        check_call(f"{case_id(case)} {tag}", c, dqkv, reference(c.qkv, c.dout, S, B, H, HD, mask), prec, groups, mask)
        if span > 0:
            # the fix-up launch stays within its workgroups, and the pipelined kernel's rows do not depend on other pairs: the
            # unflagged pairs are bit-identical to a forward of the same qkv with randn in the steep pair
            qkv2, _ = ramp_inputs(S, B, H, HD, span, with_ramp=False)
            c2 = Call(N, prec, HD, B, S, H, drop_p, qkv2, dout)
            same = pair_view(c2.qkv, S, B, H, HD).reshape(3, npair, B, HD)[:, others] == pair_view(c.qkv, S, B, H, HD).reshape(3, npair, B, HD)[:, others]
            assert bool(same.all())
            c2.forward()
            assert not any(c2.flags())
            c2.finish(c2.out, c2.lse)
            assert torch.equal(pair_view(c.out, S, B, H, HD).reshape(npair, B, HD)[others], pair_view(c2.out, S, B, H, HD).reshape(npair, B, HD)[others])
            assert torch.equal(c.lse.reshape(npair, B)[others], c2.lse.reshape(npair, B)[others])


# ------------------------------------------------------------------------------------------------ the parts in any order
@pytest.mark.gpu
@pytest.mark.parametrize("case", ORDER, ids=[case_id(c) for c in ORDER])
def test_backward_parts_in_any_order(N, case):
    prec, HD, B, S, H = case
    E = H * HD
    qkv, dout = make_inputs("plain", S, B, H, HD)
    c = Call(N, prec, HD, B, S, H, 0.0, qkv, dout)
    c.forward()
    nan = float("nan")
    got = []
    for order in (("dkv", "dq"), ("dq", "dkv"), None):
        ws, dqkv = c.buf(c.wb), c.new_dqkv(fill=nan)
        if order is None:
            c.whole(dqkv, ws)
        else:
            c.prepare(ws)
            c.part(order[0], dqkv, ws)
            torch.cuda.synchronize()
            mine = slice(0, E) if order[0] == "dq" else slice(E, 3 * E)
            rest = slice(E, 3 * E) if order[0] == "dq" else slice(0, E)
            assert bool(torch.isnan(dqkv[:, rest]).all()) and not bool(torch.isnan(dqkv[:, mine]).any()), order      # its own columns only
            c.part(order[1], dqkv, ws)
        got.append(dqkv)
    c.finish(c.out, c.lse, *got)
    print(f"{case_id(case)} [{c.plan['dkv']} {c.plan['dq']}] three orders")
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
