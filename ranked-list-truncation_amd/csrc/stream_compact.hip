// Streaming truncation, batch compaction (include/rlt_hip.h, "streaming: compacting the live lists"): the retired lists of a running
// stream leave the batch, so that the chunk's GEMMs, LayerNorms and cache reads run over the live lists alone.
//   stream_plan_kernel (rlt_stream_compact_plan): ONE workgroup of 1024 threads walks the B slots in chunks of 1024.  A slot's
//     destination is (live slots of the chunks before) + (live slots of the wavefronts before it in the chunk) + (live lanes below it
//     in its wavefront): a carried count, sixteen ballot popcounts through LDS, one masked popcount.  No atomics, one fixed order.
//   kv_gather_kernel (rlt_kv_cache_compact): an HBM-bound row gather.  A row of W floats is W/4 16-byte vectors; a group of G lanes
//     (the power of two >= min(W/4, 64)) owns one row, a wavefront 64/G rows, and every group has KV_ROWS rows in flight: their loads
//     are all issued before the first store.  The map entry of a row is read by the group's first lane and broadcast; it is read once
//     per (workgroup, slot) and kept over the ranks the workgroup walks (grid.y strides over ranks, grid.x over slot tiles), so no
//     index is ever divided.  Runs of neighbouring live slots are contiguous on both sides by construction.
#include "common.h"

namespace {

constexpr int PLAN_THREADS = 1024, PLAN_WAVES = PLAN_THREADS / 64;

__global__ __launch_bounds__(PLAN_THREADS) void stream_plan_kernel(const int32_t* __restrict__ active, const int32_t* __restrict__ origin,
                                                                   const unsigned long long* __restrict__ carry,
                                                                   const int32_t* __restrict__ k, int B, int B_full,
                                                                   int32_t* __restrict__ slot_src, int32_t* __restrict__ origin_out,
                                                                   unsigned long long* __restrict__ carry_out,
                                                                   int32_t* __restrict__ k_full, int32_t* __restrict__ n_live) {
    __shared__ int wcount[2][PLAN_WAVES];                 // two sets: one barrier per chunk
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0, set = 0;                                // live slots of the chunks before: the same in every thread
    for (int c0 = 0; c0 < B; c0 += PLAN_THREADS, set ^= 1) {
        const int b = c0 + tid;                           // c0 <= B - 1 and tid < 1024: no wrap below 2^31 - 1024 (B_full <= 2^30)
        const bool in = b < B;
        const bool live = in && active[b] != 0;
        const unsigned long long bal = __ballot(live);
        if (lane == 0) wcount[set][wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PLAN_WAVES; ++w) {
            const int c = wcount[set][w];
            before += w < wv ? c : 0;
            total += c;
        }
        if (in) {
            const int org = origin ? origin[b] : b;
            if (live) {
                const int j = base + before + __popcll(bal & ((1ull << lane) - 1ull));      // j <= b < B
                slot_src[j] = b;
                origin_out[j] = org;
                if (carry) carry_out[j] = carry[b];       // 8 bytes as an integer: NaN payloads and -0.0 pass
            } else if (k && org >= 0 && org < B_full) {
                k_full[org] = k[b];
            }
        }
        base += total;
    }
    for (int j = base + tid; j < B; j += PLAN_THREADS) {
        slot_src[j] = -1;
        origin_out[j] = -1;
    }
    if (tid == 0) n_live[0] = base;
}

constexpr int KV_ROWS = 4;                                // rows a lane group has in flight: 4 x 16 bytes per lane before the first store
constexpr int KV_WAVES = 4;

struct f4 { float x, y, z, w; } __attribute__((aligned(16)));

// grid.x: tiles of KV_WAVES * (64 / G) * KV_ROWS destination slots; grid.y: ranks.  V4 = W / 4, G = 1 << lg.
__global__ __launch_bounds__(64 * KV_WAVES) void kv_gather_kernel(const f4* __restrict__ src, f4* __restrict__ dst,
                                                                  const int32_t* __restrict__ slot_src, int t0, int B_src, int B_dst,
                                                                  int V4, int lg, int ntiles) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int G = 1 << lg, l = lane & (G - 1), sub = lane >> lg, rpw = 64 >> lg;
    const int tile_slots = KV_WAVES * rpw * KV_ROWS;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int j[KV_ROWS], e[KV_ROWS];
#pragma unroll
        for (int u = 0; u < KV_ROWS; ++u) {
            j[u] = tile * tile_slots + (u * KV_WAVES + wv) * rpw + sub;          // < ntiles * tile_slots <= B_dst + tile_slots
            int m = -1;
            if (l == 0 && j[u] < B_dst) m = slot_src[j[u]];                       // one read per row, by the group's first lane
            m = __shfl(m, lane - l);
            e[u] = (m >= 0 && m < B_src) ? m : -1;                                // -1: no row (behind B_dst, or a map entry out of range)
        }
        bool all_rows = true;
#pragma unroll
        for (int u = 0; u < KV_ROWS; ++u) all_rows = all_rows && e[u] >= 0;
        for (int s = blockIdx.y; s < t0; s += gridDim.y) {
            const f4* sp[KV_ROWS];
            f4* dp[KV_ROWS];
#pragma unroll
            for (int u = 0; u < KV_ROWS; ++u) {
                sp[u] = src + ((size_t)s * B_src + (e[u] < 0 ? 0 : e[u])) * V4;
                dp[u] = dst + ((size_t)s * B_dst + (e[u] < 0 ? 0 : j[u])) * V4;
            }
            if (all_rows) {                                 // the common case, with unconditional stores: hipcc keeps the loads together
                for (int v = l; v < V4; v += G) {
                    f4 x[KV_ROWS];
#pragma unroll
                    for (int u = 0; u < KV_ROWS; ++u) x[u] = sp[u][v];
#pragma unroll
                    for (int u = 0; u < KV_ROWS; ++u) dp[u][v] = x[u];
                }
            } else {                                        // the last tile, or a map entry out of range: row by row
                for (int v = l; v < V4; v += G)
#pragma unroll
                    for (int u = 0; u < KV_ROWS; ++u)
                        if (e[u] >= 0) dp[u][v] = sp[u][v];
            }
        }
    }
}

inline bool aligned_to(const void* p, uintptr_t n) { return p == nullptr || (((uintptr_t)p) & (n - 1)) == 0; }

}  // namespace

extern "C" {

int rlt_stream_compact_plan(const int32_t* active, const int32_t* origin, const double* carry, const int32_t* k, int B, int B_full,
                            int32_t* slot_src, int32_t* origin_out, double* carry_out, int32_t* k_full, int32_t* n_live,
                            void* stream) {
    RLT_CHECK_ARG(active && slot_src && origin_out && n_live);
    RLT_CHECK_ARG((carry != nullptr) == (carry_out != nullptr) && (k != nullptr) == (k_full != nullptr));
    RLT_CHECK_ARG(B > 0 && B_full > 0 && B <= B_full);
    const void* ins[] = {active, origin, carry, k};
    const void* outs[] = {slot_src, origin_out, carry_out, k_full, n_live};
    for (size_t o = 0; o < sizeof(outs) / sizeof(outs[0]); ++o) {
        if (!outs[o]) continue;
        for (const void* in : ins) RLT_CHECK_ARG(outs[o] != in);
        for (size_t p = 0; p < o; ++p) RLT_CHECK_ARG(outs[o] != outs[p]);           // two outputs in one place have no defined result
    }
    RLT_CHECK_SHAPE(B_full <= (1 << 30));
    if (!(aligned_to(carry, 8) && aligned_to(carry_out, 8))) return RLT_E_ALIGN;
    if (!(aligned_to(active, 4) && aligned_to(origin, 4) && aligned_to(k, 4) && aligned_to(slot_src, 4) && aligned_to(origin_out, 4) &&
          aligned_to(k_full, 4) && aligned_to(n_live, 4)))
        return RLT_E_ALIGN;
    hipLaunchKernelGGL(stream_plan_kernel, dim3(1), dim3(PLAN_THREADS), 0, rlt_stream(stream), active, origin,
                       (const unsigned long long*)carry, k, B, B_full, slot_src, origin_out, (unsigned long long*)carry_out, k_full, n_live);
    return RLT_LAUNCH_RESULT();
}

int rlt_kv_cache_compact(const float* src, float* dst, const int32_t* slot_src, int t0, int B_src, int B_dst, int W, void* stream) {
    RLT_CHECK_ARG(src && dst && slot_src);
    RLT_CHECK_ARG(t0 >= 0 && B_src >= 1 && B_dst >= 0 && B_dst <= B_src && W >= 1);
    {   // the two ranges must not overlap: 128-bit byte counts, so that no product of three ints wraps
        const unsigned __int128 sb = (unsigned __int128)t0 * B_src * W * 4u, db = (unsigned __int128)t0 * B_dst * W * 4u;
        const unsigned __int128 s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
        RLT_CHECK_ARG(!(sb != 0 && db != 0 && s0 < d0 + db && d0 < s0 + sb));
    }
    RLT_CHECK_SHAPE(W % 4 == 0 && W <= 2048);
    RLT_CHECK_SHAPE((long long)t0 * B_src < (1LL << 40) / W && B_src <= (1 << 30));   // 64-bit element offsets, 32-bit slot numbers
    if (!rlt_aligned16(src) || !rlt_aligned16(dst)) return RLT_E_ALIGN;
    if (t0 == 0 || B_dst == 0) return 0;
    const int V4 = W / 4;
    int lg = 0;
    while ((1 << lg) < V4 && lg < 6) ++lg;
    const int tile_slots = KV_WAVES * (64 >> lg) * KV_ROWS;
    const int ntiles = rlt_cdiv(B_dst, tile_slots);
    // about eight workgroups of 256 for each of the 256 compute units, the ranks spread over what the slot tiles leave
    const int target = 2048;
    const int gx = ntiles < target ? ntiles : target;
    int gy = rlt_cdiv(target, gx);
    if (gy > t0) gy = t0;
    hipLaunchKernelGGL(kv_gather_kernel, dim3(gx, gy), dim3(64 * KV_WAVES), 0, rlt_stream(stream), (const f4*)src, (f4*)dst, slot_src, t0,
                       B_src, B_dst, V4, lg, ntiles);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
