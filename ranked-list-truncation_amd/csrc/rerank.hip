// Rerank, then truncate: a stable per-list sort by descending head value that carries the labels and the companion arrays
// along, so that every evaluation pass of the library (baselines, cut report, cut sweep, reward evaluation) runs unchanged on
// the re-ranked lists.
//
// The order of list b is that of np.argsort(-pred[b], kind="stable") on float32: values descend, equal values (+0 == -0) keep
// their original order, every NaN comes after every number in original order.  Each element becomes ONE 64-bit key
//     (image of the value << 32) | original index
// where the image is a uint32 that ASCENDS as the value descends (-0 first folded onto +0), 0xfffffffe for every NaN and
// 0xffffffff for the padding up to a power of two.  The keys of a list are distinct, so an ascending sort of them is a total
// order whatever bits pred holds: the result is always a permutation, and stability falls out of the index in the low word.
//
// A group of L lanes (16, 32 or 64: four, two or one list per wavefront) owns a list of up to N = L * R elements, lane hl holding
// the R consecutive elements hl * R .. hl * R + R - 1 in registers.  The sort is a bitonic network on the registers: the stages
// with a distance below R exchange registers of one lane, the others exchange with lane hl ^ (distance / R).  The sorted indices
// go to the wavefront's own LDS (perm); rank is written from the registers, and sorted_pred and the companions are gathered
// through perm with coalesced stores - pred is one more companion, so its bits arrive unchanged.  The grid is sized to the chip
// and strides over the lists.  One launch, no workspace, no atomics, no allocation, no host synchronisation.
//
// Algorithmic bytes per list: read 4 S (1 + n), write up to 4 S (3 + n).
#include "common.h"

namespace {

constexpr int RR_WAVES = 4;                     // wavefronts per workgroup
constexpr int RR_MAX_S = 1024;
constexpr int RR_MAX_N = 4;                     // companion arrays
constexpr int RR_MAX_GRID = 2048;               // workgroups (8 per CU); beyond that they stride over the lists

struct RerankArgs {
    const float* pred;
    const float* src[RR_MAX_N + 1];             // the companions, then pred itself when sorted_pred is asked for
    float* dst[RR_MAX_N + 1];
    int32_t* perm;
    int32_t* rank;
    int B, S, n;                                // n counts the entries of src / dst in use
};

// ascending image of the descending order; NaN behind every number
__device__ __forceinline__ uint32_t rerank_image(float v) {
    uint32_t b = __builtin_bit_cast(uint32_t, v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xfffffffeu;
    if (b == 0x80000000u) b = 0u;               // -0 ties with +0
    const uint32_t up = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ~up;
}

template <int L, int R>
__global__ __launch_bounds__(64 * RR_WAVES) void rerank_kernel(RerankArgs a) {
    constexpr int N = L * R, LPW = 64 / L;
    __shared__ int sperm[RR_WAVES][LPW][N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int hl = lane & (L - 1), grp = lane / L;
    const int S = a.S, B = a.B;
    int* const sp = sperm[wv][grp];
    const long long step = (long long)LPW * gridDim.x * RR_WAVES;
    for (long long pb = (long long)LPW * (blockIdx.x * RR_WAVES + wv); pb < B; pb += step) {      // 64-bit: B up to INT_MAX
        const bool live = pb + grp < B;         // lists beyond B: the idle group shadows the first one, its stores are masked
        const size_t base = (size_t)(live ? pb + grp : pb) * S;
        unsigned long long key[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = hl * R + r;
            const uint32_t im = i < S ? rerank_image(a.pred[base + i]) : 0xffffffffu;
            key[r] = ((unsigned long long)im << 32) | (uint32_t)i;
        }
        // ---- bitonic network, ascending in the key: element i = hl * R + r meets element i ^ j -----------------------------
#pragma unroll
        for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j >= R) {                   // the partner sits in lane hl ^ (j / R), same register
                    const bool keep_min = ((hl * R & k) == 0) == ((hl * R & j) == 0);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const unsigned long long o = __shfl_xor(key[r], j / R);
                        const bool o_less = o < key[r];
                        key[r] = (o_less == keep_min) ? o : key[r];
                    }
                } else {                        // both in this lane
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if ((r & j) == 0) {
                            const bool up = (((hl * R + r) & k) == 0);
                            const unsigned long long x = key[r], y = key[r | j];
                            const bool sw = (y < x) == up;
                            key[r] = sw ? y : x;
                            key[r | j] = sw ? x : y;
                        }
                    }
                }
            }
        }
        // ---- position hl * R + r now holds the element of that rank; the padding sits behind the S real ones ---------------
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int p = hl * R + r;
            const int idx = (int)(uint32_t)key[r];
            sp[p] = idx;
            if (live && p < S) {
                if (a.perm) a.perm[base + p] = idx;
                if (a.rank) a.rank[base + idx] = p;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (live) {
#pragma unroll
            for (int t = 0; t <= RR_MAX_N; ++t) {
                if (t < a.n) {
                    const float* const s = a.src[t] + base;
                    float* const d = a.dst[t] + base;
                    for (int i = hl; i < S; i += L) d[i] = s[sp[i]];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();        // the next list's stores come after these loads
    }
}

}  // namespace

extern "C" {

int rlt_rerank_lists(const float* pred, int B, int S, const float* const* src, float* const* dst, int n,
                     int32_t* perm, int32_t* rank, float* sorted_pred, void* stream) {
    RLT_CHECK_ARG(pred);
    RLT_CHECK_ARG(B > 0 && S > 0);
    RLT_CHECK_ARG(n >= 0 && n <= RR_MAX_N);
    RLT_CHECK_ARG(n == 0 || (src && dst));
    for (int t = 0; t < n; ++t) RLT_CHECK_ARG(src[t] && dst[t]);
    RLT_CHECK_ARG(n > 0 || perm || rank || sorted_pred);
    RLT_CHECK_SHAPE(S <= RR_MAX_S);
    uintptr_t bits = (uintptr_t)pred | (uintptr_t)perm | (uintptr_t)rank | (uintptr_t)sorted_pred;
    for (int t = 0; t < n; ++t) bits |= (uintptr_t)src[t] | (uintptr_t)dst[t];
    if ((bits & 3u) != 0) return RLT_E_ALIGN;
    RerankArgs a{};
    a.pred = pred; a.perm = perm; a.rank = rank;
    a.B = B; a.S = S; a.n = n;
    for (int t = 0; t < n; ++t) { a.src[t] = src[t]; a.dst[t] = dst[t]; }
    if (sorted_pred) { a.src[n] = pred; a.dst[n] = sorted_pred; a.n = n + 1; }
    hipStream_t st = rlt_stream(stream);
    const auto launch = [&](auto kernel, int lanes) {
        const int groups = rlt_cdiv(B, RR_WAVES * (64 / lanes));
        hipLaunchKernelGGL(kernel, dim3(groups < RR_MAX_GRID ? groups : RR_MAX_GRID), dim3(64 * RR_WAVES), 0, st, a);
    };
    if (S <= 64) launch(rerank_kernel<16, 4>, 16);
    else if (S <= 128) launch(rerank_kernel<32, 4>, 32);
    else if (S <= 256) launch(rerank_kernel<64, 4>, 64);
    else if (S <= 512) launch(rerank_kernel<64, 8>, 64);
    else launch(rerank_kernel<64, 16>, 64);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
