// gemm6e: the 256 x 256 six-product tile by ONE wavefront per SIMD (256 threads, 128 x 128 per wavefront: all 256 AGPRs are
// accumulators).  In gemm6c (gemm6c.hip) two wavefronts share a SIMD and the ~250 vector instructions a wavefront spends on the split of the
// next K tile are not absorbed by its partner's MFMAs (slot timeline in profiles/r04_notes.md: 3,800 cycles for a slot that only
// multiplies, 5,200 for one that also splits, 3,072 of MFMAs in both).  A bf16 MFMA hides ~4 plain vector instructions of the
// SAME wavefront when they sit right behind it (tools/micro/mfma_split.hip), so here a slot is one k-step of 16 = 16 groups of
// six MFMAs per wavefront, each MFMA followed by a gap that carries one part of the split of the k-step two slots ahead (its
// eight staged pieces: 4 of A, 4 of B per thread), a store + reload, or fragment reads - placed by tools/gen_gemm6e_slot.py,
// fenced so that hipcc keeps the order.  Three k-step buffers rotate as in gemm6c (same LDS layout, phys6 rows, swizzled
// 16-byte chunks); slot s multiplies buffer s % 3, writes k-step s + 2 into buffer (s + 2) % 3 (free since the barrier that
// opened the slot) and reloads the staging registers of its parity with k-step s + 4.  Loads are per k-step (64 bytes of a
// K-contiguous row per 4 lanes: half lines - the price of a uniform slot).  Its epilogues: write_output_simple (gemm_common.h).
#include "gemm6c.h"

namespace {

template <bool KC>
__device__ __forceinline__ size_t off6e(int tid, int ld) {           // this thread's element offset inside a k-step of an operand
    if (KC) return (size_t)phys6(tid >> 2) * ld + 4 * (tid & 3);     // row phys6(t + 64 i) = phys6(t) + 64 i, float4 kq
    return (size_t)(4 * (tid & 3)) * ld + 4 * (tid >> 2);            // k rows 4 kb + i, columns 4 mb ..
}
template <bool KC>
__device__ __forceinline__ void load6e(const float* __restrict__ P, int ld, int i, float4& v) {   // P: operand + uniform part + off6e
    v = *reinterpret_cast<const float4*>(P + (size_t)(KC ? 64 * i : i) * ld);
}
template <bool KC>
__device__ __forceinline__ int dst6e(int tid, int p) {               // bf16 element offset of piece p inside the operand's h plane
    const int x = tid & 3;
    const int pr = KC ? (tid >> 2) + 64 * p : ((((tid >> 2) * 4) & ~15) | (p << 2) | ((tid >> 2) & 3));
    return pr * 16 + 8 * ((x >> 1) ^ ((pr >> 3) & 1)) + 4 * (x & 1);
}
template <bool KC>
__device__ __forceinline__ void vals6e(const float4 (&v)[4], int p, float& a, float& b, float& c, float& d) {
    if (KC) { a = v[p].x; b = v[p].y; c = v[p].z; d = v[p].w; }
    else {
        const float* f0 = reinterpret_cast<const float*>(&v[0]);
        const float* f1 = reinterpret_cast<const float*>(&v[1]);
        const float* f2 = reinterpret_cast<const float*>(&v[2]);
        const float* f3 = reinterpret_cast<const float*>(&v[3]);
        a = f0[p]; b = f1[p]; c = f2[p]; d = f3[p];
    }
}
template <bool TA, bool TB, bool PERSIST>
__global__ __launch_bounds__(256, 1) void gemm6e_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    uint16_t* lds = reinterpret_cast<uint16_t*>(gsm);          // [3][A_h | A_m | A_l | B_h | B_m | B_l]
    // (tile_frame of gemm_common.h, written out: through the call this kernel compiles to other code)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int wm = wv >> 1, wn = wv & 1;
    int bid, zslab;
    decode_block(g, bid, zslab);
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    int m0 = tm * BM2, n0 = tn * BN2;
    const int kbeg = zslab * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int nks = (kend - kbeg) / 16;              // k-steps per output tile: even, >= 4 (host-checked)

    f32x16 acc[2][2][4];                             // [row half of 64][A block in the half][B block]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i >> 1][i & 1][j][r] = 0.f;

    constexpr bool AKC = !TA, BKC = TB;
    const bool want_cs = TA && g.colsum != nullptr && tn == 0;
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    const int pl = phys6(l31);
    const int csw = 8 * (hh ^ ((pl >> 3) & 1));
    const int arow = (wm * 128 + pl) * 16 + csw, brow = 3 * HB6 + (wn * 128 + pl) * 16 + csw;
    const size_t offA = off6e<AKC>(tid, g.lda), offB = off6e<BKC>(tid, g.ldb);
    int dA[4], dB[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) { dA[p] = dst6e<AKC>(tid, p); dB[p] = 3 * HB6 + dst6e<BKC>(tid, p); }

    // tile of the stream after the current one (PERSIST)
    int vid = blockIdx.x, nm0 = m0, nn0 = n0;
    bool has_next = false;
    // operand pointers of k-step `ks` of the stream: ks < nks -> this output tile; nks.. -> the next one's (or, at the end of the
    // stream, a harmless re-read of the last k-step: loads and stores of the slot body are unconditional)
    auto srcA = [&](int ks) {
        const bool wrap = PERSIST && has_next && ks >= nks;
        const int k0 = kbeg + 16 * (wrap ? ks - nks : min(ks, nks - 1)), mm = wrap ? nm0 : m0;
        return g.A + (AKC ? (size_t)mm * g.lda + k0 : (size_t)k0 * g.lda + mm) + offA;
    };
    auto srcB = [&](int ks) {
        const bool wrap = PERSIST && has_next && ks >= nks;
        const int k0 = kbeg + 16 * (wrap ? ks - nks : min(ks, nks - 1)), nn = wrap ? nn0 : n0;
        return g.B + (BKC ? (size_t)nn * g.ldb + k0 : (size_t)k0 * g.ldb + nn) + offB;
    };
    float4 ra[2][4], rb[2][4];                       // staged k-steps, by parity
    auto stash_all = [&](uint16_t* wb, const float4 (&va)[4], const float4 (&vb)[4]) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float a, b, c, d;
            uint2 hi, mid, lo;
            vals6e<AKC>(va, p, a, b, c, d);
            split4x3<true>(a, b, c, d, hi, mid, lo);
            *reinterpret_cast<uint2*>(wb + dA[p]) = hi;
            *reinterpret_cast<uint2*>(wb + dA[p] + HB6) = mid;
            *reinterpret_cast<uint2*>(wb + dA[p] + 2 * HB6) = lo;
            vals6e<BKC>(vb, p, a, b, c, d);
            split4x3<true>(a, b, c, d, hi, mid, lo);
            *reinterpret_cast<uint2*>(wb + dB[p]) = hi;
            *reinterpret_cast<uint2*>(wb + dB[p] + HB6) = mid;
            *reinterpret_cast<uint2*>(wb + dB[p] + 2 * HB6) = lo;
        }
    };
    bf16x8 a[4][3], b[2][3];
    auto frag_a = [&](const uint16_t* base, int i, int q) { a[i][q] = *reinterpret_cast<const bf16x8*>(base + arow + q * HB6 + i * 32 * 16); };
    auto frag_b = [&](const uint16_t* base, int j, int q) { b[j & 1][q] = *reinterpret_cast<const bf16x8*>(base + brow + q * HB6 + j * 32 * 16); };

    // prologue: k-steps 0, 1 -> buffers 0, 1; k-steps 2, 3 in flight; fragments of A blocks 0, 1 and B block 0 of buffer 0
    {
        const float* pa = srcA(0); const float* pb = srcB(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) { load6e<AKC>(pa, g.lda, i, ra[0][i]); load6e<BKC>(pb, g.ldb, i, rb[0][i]); }
        pa = srcA(1); pb = srcB(1);
#pragma unroll
        for (int i = 0; i < 4; ++i) { load6e<AKC>(pa, g.lda, i, ra[1][i]); load6e<BKC>(pb, g.ldb, i, rb[1][i]); }
        if (want_cs) { csum_add(csum, ra[0]); csum_add(csum, ra[1]); }
        stash_all(lds, ra[0], rb[0]);
        stash_all(lds + KB6, ra[1], rb[1]);
        if (PERSIST) next_tile<PERSIST>(g, BM2, BN2, vid, has_next, nm0, nn0);
        pa = srcA(2); pb = srcB(2);
#pragma unroll
        for (int i = 0; i < 4; ++i) { load6e<AKC>(pa, g.lda, i, ra[0][i]); load6e<BKC>(pb, g.ldb, i, rb[0][i]); }
        pa = srcA(3); pb = srcB(3);
#pragma unroll
        for (int i = 0; i < 4; ++i) { load6e<AKC>(pa, g.lda, i, ra[1][i]); load6e<BKC>(pb, g.ldb, i, rb[1][i]); }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) { frag_a(lds, 0, q); frag_a(lds, 1, q); frag_b(lds, 0, q); }

    // one slot (parity PAR of its k-step index s): multiplies buffer `buf`, writes k-step s + 2 (staged set PAR) into `wbuf`,
    // reloads the set from (pa, pb) = k-step s + 4, reads the first fragments of the next slot out of `nbuf`
    auto slot = [&](auto par_tag, int buf, int wbuf, int nbuf, const float* pa, const float* pb) {
        constexpr int PAR = decltype(par_tag)::value;
        const uint16_t* base = lds + buf * KB6;
        const uint16_t* nbase = lds + nbuf * KB6;
        uint16_t* wb = lds + wbuf * KB6;
        Split6 su;
#define GAP_END __builtin_amdgcn_sched_barrier(0)
#define MM(i_, j_, k_) acc[(i_) >> 1][(i_) & 1][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16( \
            a[i_][(k_) == 0 || (k_) == 3 ? 1 : (k_) == 1 ? 2 : 0], b[(j_) & 1][(k_) == 0 || (k_) == 4 ? 1 : (k_) == 2 ? 2 : 0], acc[(i_) >> 1][(i_) & 1][j_], 0, 0, 0)
#define SP(p_, k_) do { float x0_, x1_, x2_, x3_; \
            if ((p_) < 4) vals6e<AKC>(ra[PAR], (p_) & 3, x0_, x1_, x2_, x3_); else vals6e<BKC>(rb[PAR], (p_) & 3, x0_, x1_, x2_, x3_); \
            split6_part(su, x0_, x1_, x2_, x3_, k_); } while (0)
#define ST(p_) do { const int d_ = (p_) < 4 ? dA[(p_) & 3] : dB[(p_) & 3]; \
            *reinterpret_cast<uint2*>(wb + d_) = su.hi; *reinterpret_cast<uint2*>(wb + d_ + HB6) = su.mid; \
            *reinterpret_cast<uint2*>(wb + d_ + 2 * HB6) = su.lo; \
            if ((p_) < 4) { if (AKC) load6e<AKC>(pa, g.lda, (p_) & 3, ra[PAR][(p_) & 3]); \
                            else if ((p_) == 3) { for (int i_ = 0; i_ < 4; ++i_) load6e<AKC>(pa, g.lda, i_, ra[PAR][i_]); } } \
            else { if (BKC) load6e<BKC>(pb, g.ldb, (p_) & 3, rb[PAR][(p_) & 3]); \
                   else if ((p_) == 7) { for (int i_ = 0; i_ < 4; ++i_) load6e<BKC>(pb, g.ldb, i_, rb[PAR][i_]); } } } while (0)
#define RA(i_, q_, n_) frag_a((n_) ? nbase : base, i_, q_)
#define RB(j_, q_, n_) frag_b((n_) ? nbase : base, j_, q_)
#include "gemm6e_slot.inc"
#undef GAP_END
#undef MM
#undef SP
#undef ST
#undef RA
#undef RB
    };

    int u = 0;                                       // buffer of the slot's k-step
    while (true) {
        for (int s = 0; s < nks; s += 2) {
            const int u1 = u == 2 ? 0 : u + 1, u2 = u1 == 2 ? 0 : u1 + 1;
            if (want_cs && s + 2 < nks) csum_add(csum, ra[0]);
            slot(std::integral_constant<int, 0>{}, u, u2, u1, srcA(s + 4), srcB(s + 4));
            __syncthreads();
            if (want_cs && s + 3 < nks) csum_add(csum, ra[1]);
            slot(std::integral_constant<int, 1>{}, u1, u, u2, srcA(s + 5), srcB(s + 5));
            __syncthreads();
            u = u2;
        }
        write_output_simple<4>(g, acc[0], m0 + wm * 128, n0 + wn * 128, l31, hh, zslab);
        write_output_simple<4>(g, acc[1], m0 + wm * 128 + 64, n0 + wn * 128, l31, hh, zslab);
        if (!PERSIST || !has_next) break;
        m0 = nm0; n0 = nn0;
        next_tile<PERSIST>(g, BM2, BN2, vid, has_next, nm0, nn0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i >> 1][i & 1][j][r] = 0.f;
    }
    if (want_cs) finish_colsum<CsLow4, BM2, false>(g, csum, gsm, tid, m0, zslab);
}

static_assert(family_is(RLT_GEMM_6E, BM2, BN2, (size_t)3 * KB6 * sizeof(uint16_t)), "gemm_plan.h: GEMM_FAMILY");

}  // namespace

extern "C" int rlt_gemm6e_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st) {
    return with_layout(p.d.ta, p.d.tb, [&](auto TA, auto TB) {
        constexpr bool A_ = decltype(TA)::value, B_ = decltype(TB)::value;
        if constexpr (!A_) if (p.d.persistent) return launch(gemm6e_kernel<A_, B_, true>, p, g, rec, st);      // (A stored [M][K] only)
        return launch(gemm6e_kernel<A_, B_, false>, p, g, rec, st);
    });
}
