"""Host restatement of the streaming batch compaction (include/rlt_hip.h, "streaming: compacting the live lists") in numpy:
np.flatnonzero(active), the gathers through it and the k hand-over.  tests/test_stream_compact_restate.py pins it by hand-written
cases; tests/test_stream_compact_gpu.py holds rlt_stream_compact_plan and rlt_kv_cache_compact to it with zero tolerance."""
import numpy as np


def plan(active, origin=None, carry=None, k=None, k_full=None, B_full=None):
    """active (B,) ints, origin (B,) ints or None (identity), carry (B,) float64 or None, k (B,) with k_full (B_full,) or neither ->
    dict: slot_src (B,), origin (B,) - -1 behind the live entries -, carry (n_live,) bit copies or None, k_full (a copy, updated)
    or None, n_live."""
    active = np.asarray(active)
    B = active.shape[0]
    origin = np.arange(B, dtype=np.int32) if origin is None else np.asarray(origin, dtype=np.int32)
    live = np.flatnonzero(active != 0).astype(np.int32)
    n = int(live.size)
    slot_src = np.full(B, -1, np.int32)
    origin_out = np.full(B, -1, np.int32)
    slot_src[:n] = live
    origin_out[:n] = origin[live]
    out = {"slot_src": slot_src, "origin": origin_out, "n_live": n, "carry": None, "k_full": None}
    if carry is not None:
        out["carry"] = np.asarray(carry, dtype=np.float64).view(np.uint64)[live].view(np.float64)       # through the integer view: bitwise
    if k is not None:
        kf = np.array(k_full, dtype=np.int32, copy=True)
        B_full = kf.shape[0] if B_full is None else B_full
        for b in np.flatnonzero(active == 0):
            if 0 <= origin[b] < B_full:
                kf[origin[b]] = k[b]
        out["k_full"] = kf
    return out


def gather_cache(src, slot_src, t0, B_src, B_dst, dst):
    """src (>= t0*B_src, W), dst (>= t0*B_dst, W) float32 -> a copy of dst with row s*B_dst + j = src row s*B_src + slot_src[j]
    for s < t0, j < B_dst, through the uint32 view; a map entry outside [0, B_src) leaves its rows as they are."""
    out = np.array(dst, copy=True)
    s32, o32 = np.asarray(src).view(np.uint32), out.view(np.uint32)
    m = np.asarray(slot_src[:B_dst], dtype=np.int64)
    js = np.flatnonzero((m >= 0) & (m < B_src))
    if t0 and js.size:
        W = s32.shape[1]
        o32[:t0 * B_dst].reshape(t0, B_dst, W)[:, js] = s32[:t0 * B_src].reshape(t0, B_src, W)[:, m[js]]
    return out
