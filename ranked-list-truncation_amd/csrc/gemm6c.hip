// gemm6c: the 256 x 256 six-product tile with the split of the next K tile BEHIND the MFMAs.
// gemm6b (gemm6.hip) holds one K tile of 32 as six 16 KB planes (96 KB: no room for a second copy) and alternates a multiply
// phase with a split phase in which both wavefronts of every SIMD do vector work only (~15-20 % of its K loop).  Here the
// unit is the MFMA k-step: a k-step buffer is [A_h | A_m | A_l | B_h | B_m | B_l] x 256 rows x 16 k = 48 KB, THREE of them
// rotate (144 KB), and the loop runs in slots of one k-step (48 MFMAs per wavefront, one barrier):
//   slot u multiplies k-step u out of buffer u % 3;
//   an ODD slot also splits the staged register tile (a K tile of 32 = the next two k-steps) into buffers (u+1) % 3 and
//   (u+2) % 3 - both free: their last readers ran before the barrier that opened this slot - piece by piece behind its MFMA
//   groups, then issues the global loads of the register tile after that one (consumed two slots later: one whole slot plus
//   of latency cover from a single staging set);
//   an EVEN slot only multiplies.
// Rows are 32 bytes (16 bf16): logical row r sits at physical row phys6(r) (the two low 2-bit fields swapped) and its two
// 16-byte chunks are XOR-swizzled with bit 3 of the physical row, which makes the ds_read_b128 fragment reads and the
// ds_write_b64 stores of BOTH staging maps conflict-free (derivation: DESIGN.md 4.2).
// Staging maps (every wave-level load covers whole 128-byte lines):
//   K-contiguous operand: the 8 lanes tid & 7 read the 8 float4 of one row's K tile; lanes 0-3 of a row group hold k-step 0
//   of the tile in their loads 0 / 2 and k-step 1 in their loads 1 / 3, lanes 4-7 the other way round (kq = (tid & 7) ^ 4 i):
//   one select per register pair at stash time puts k-step 0 in registers 0 / 2 for every lane (8 v_cndmask per float4 pair -
//   against half-line loads, which double the L2 requests the 256-wide tiles were built to save);
//   MN-contiguous operand: wavefronts 0-3 hold the 16 k rows of k-step 0 (a 4 x 4 block per thread), wavefronts 4-7 those of
//   k-step 1 (wavefronts w and w + 4 share a SIMD, so every SIMD splits the same amount).
// PERSIST (no split-K, A stored [M][K], more tiles than workgroups): the workgroups walk the output tiles as ONE stream of
// k-steps, the first K tile of the next output tile is staged in the last odd slot of the current one and its second K tile
// is in flight during the epilogue - at K = 256 (8 K tiles: five of the eight big products of the encoder layer) the
// prologue and the 256 KB epilogue of a tile were uncovered time.
#include "gemm6c.h"

namespace {

struct Stage6c { float4 v[4]; };
template <bool KC>
__device__ __forceinline__ void load6c(const float* __restrict__ P, int ld, int mn0, int k0, int tid, Stage6c& st) {
    if (KC) {
        const int t = tid >> 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pr = (t & 1) | ((i & 1) << 1) | ((t >> 1) << 2) | ((i >> 1) << 7);       // physical LDS row
            const int kq = (tid & 7) ^ ((i & 1) << 2);
            st.v[i] = *reinterpret_cast<const float4*>(P + (size_t)(mn0 + phys6(pr)) * ld + k0 + 4 * kq);
        }
    } else {
        const int half = tid >> 8, t2 = tid & 255, kb = t2 & 3, mb = t2 >> 2;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            st.v[i] = *reinterpret_cast<const float4*>(P + (size_t)(k0 + 16 * half + 4 * kb + i) * ld + mn0 + 4 * mb);
    }
}
// piece `part` (0..3) of the split + LDS store of a staged operand tile.  T0 / T1: the h plane of this operand in the
// buffers of the tile's k-step 0 / k-step 1 (the m and l planes follow at + HB6, + 2 HB6).
template <bool KC>
__device__ __forceinline__ void stash6c_part(uint16_t* __restrict__ T0, uint16_t* __restrict__ T1, int tid, const Stage6c& st, int part) {
    uint2 hi, mid, lo;
    uint16_t* dst;
    if (KC) {
        // part -> register pair (part >> 1), k-step (part & 1) of the tile
        const int hb = (tid >> 2) & 1, t = tid >> 3, j = 2 * (part >> 1) + (part & 1);       // register index after the swap
        const float4 a = st.v[2 * (part >> 1)], b = st.v[2 * (part >> 1) + 1];
        const bool second = ((part & 1) ^ hb) != 0;                                          // this lane's k-step `part & 1` sits in load j ^ hb
        const float4 x = make_float4(second ? b.x : a.x, second ? b.y : a.y, second ? b.z : a.z, second ? b.w : a.w);
        const int pr = (t & 1) | (((j ^ hb) & 1) << 1) | ((t >> 1) << 2) | ((j >> 1) << 7);
        const int kq4 = tid & 3;
        dst = ((part & 1) ? T1 : T0) + pr * 16 + 8 * ((kq4 >> 1) ^ ((pr >> 3) & 1)) + 4 * (kq4 & 1);
        split4x3<true>(x.x, x.y, x.z, x.w, hi, mid, lo);
    } else {
        const int half = tid >> 8, t2 = tid & 255, kb = t2 & 3, mb = t2 >> 2;
        const float* f0 = reinterpret_cast<const float*>(&st.v[0]);
        const float* f1 = reinterpret_cast<const float*>(&st.v[1]);
        const float* f2 = reinterpret_cast<const float*>(&st.v[2]);
        const float* f3 = reinterpret_cast<const float*>(&st.v[3]);
        const int pr = ((4 * mb) & ~15) | (part << 2) | (mb & 3);                             // phys6(4 mb + part)
        dst = (half ? T1 : T0) + pr * 16 + 8 * ((kb >> 1) ^ ((pr >> 3) & 1)) + 4 * (kb & 1);
        split4x3<true>(f0[part], f1[part], f2[part], f3[part], hi, mid, lo);
    }
    *reinterpret_cast<uint2*>(dst) = hi;
    *reinterpret_cast<uint2*>(dst + HB6) = mid;
    *reinterpret_cast<uint2*>(dst + 2 * HB6) = lo;
}

#if defined(RLT_STAMPS)
// timeline instrumentation (variant builds only, tools/bench_kernels.py g6c_stamps): s_memtime per wavefront at [slot start |
// last MFMA issued | barrier passed] of the first 40 slots of one workgroup
__device__ unsigned long long rlt_g6c_stamp_buf[8 * 40 * 3];
#define RLT_G6C_STAMP(slot_, k_) do { if (blockIdx.x == (gridDim.x / 2 | 1) && (threadIdx.x & 63) == 0 && (slot_) < 40) \
    rlt_g6c_stamp_buf[((threadIdx.x >> 6) * 40 + (slot_)) * 3 + (k_)] = __builtin_readcyclecounter(); } while (0)
#else
#define RLT_G6C_STAMP(slot_, k_) do {} while (0)
#endif
template <bool TA, bool TB, bool PERSIST>
__global__ __launch_bounds__(512) void gemm6c_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    uint16_t* lds = reinterpret_cast<uint16_t*>(gsm);          // [3][A_h | A_m | A_l | B_h | B_m | B_l]
    // (tile_frame of gemm_common.h, written out: through the call this kernel compiles to other code)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int wm = wv >> 1, wn = wv & 1;
    int bid, zslab;
    decode_block(g, bid, zslab);                     // g.tiles_* count 256 x 256 tiles here
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    int m0 = tm * BM2, n0 = tn * BN2;
    const int kbeg = zslab * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int nt = (kend - kbeg) / BK3;              // register tiles (K tiles of 32) per output tile; >= 2 (host-checked)

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    Stage6c sa, sb;
    constexpr bool AKC = !TA, BKC = TB;
    const bool want_cs = TA && g.colsum != nullptr && tn == 0;
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    const int pl = phys6(l31);
    const int csw = 8 * (hh ^ ((pl >> 3) & 1));      // element offset of this lane's 16-byte chunk inside its row
    const int arow = (wm * 64 + pl) * 16 + csw, brow = 3 * HB6 + (wn * 128 + pl) * 16 + csw;

    // tile of the stream after the current one (PERSIST)
    int vid = blockIdx.x, nm0 = m0, nn0 = n0;
    bool has_next = false;
    // register tile `ti` of the stream position: ti < nt -> this output tile; nt, nt + 1 -> the next one's tiles 0, 1 (or, at the
    // end of the stream, a harmless re-read of the last tile: the fetch is unconditional so that hipcc's vmcnt counts stay exact)
    auto fetch = [&](int ti) {
        const bool wrap = PERSIST && has_next && ti >= nt;
        const int k0 = kbeg + (wrap ? ti - nt : min(ti, nt - 1)) * BK3;
        load6c<AKC>(g.A, g.lda, wrap ? nm0 : m0, k0, tid, sa);
        load6c<BKC>(g.B, g.ldb, wrap ? nn0 : n0, k0, tid, sb);
    };
    auto add_cs = [&]() {          // (csum_add, as a closure: slot() below captures it, and hipcc's output follows the capture order)
#pragma unroll
        for (int i = 0; i < 4; ++i) { csum.x += sa.v[i].x; csum.y += sa.v[i].y; csum.z += sa.v[i].z; csum.w += sa.v[i].w; }
    };

    // one slot: the 48 MFMAs of k-step buffer `buf`; STASH: pieces of the staged register tile go behind the MFMA groups into
    // buffers b1 (its k-step 0) and b2 (its k-step 1), then the loads of register tile `fetch_ti` are issued
    auto slot = [&](auto stash_tag, int buf, int b1, int b2, bool do_stash, int fetch_ti) {
        constexpr bool STASH = decltype(stash_tag)::value;
        const uint16_t* base = lds + buf * KB6;
        uint16_t* t1 = lds + b1 * KB6;
        uint16_t* t2 = lds + b2 * KB6;
        bf16x8 a[2][3], b[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 3; ++q) a[i][q] = *reinterpret_cast<const bf16x8*>(base + arow + q * HB6 + i * 32 * 16);
        auto load_b = [&](int j, int s_) {
#pragma unroll
            for (int q = 0; q < 3; ++q) b[s_][q] = *reinterpret_cast<const bf16x8*>(base + brow + q * HB6 + j * 32 * 16);
        };
        load_b(0, 0);
        if (STASH && do_stash && want_cs) add_cs();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j + 1 < 4) load_b(j + 1, (j + 1) & 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x16 c = acc[i][j];
                // smallest terms first
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j & 1][1], c, 0, 0, 0);   // m m'
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][2], b[j & 1][0], c, 0, 0, 0);   // l h'
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j & 1][2], c, 0, 0, 0);   // h l'
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j & 1][0], c, 0, 0, 0);   // m h'
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j & 1][1], c, 0, 0, 0);   // h m'
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j & 1][0], c, 0, 0, 0);   // h h'
                acc[i][j] = c;
                if (STASH && do_stash) {               // piece 2 j + i of eight: A pieces 0..3, then B pieces 0..3
                    const int piece = 2 * j + i;
                    if (piece < 4) stash6c_part<AKC>(t1, t2, tid, sa, piece);
                    else stash6c_part<BKC>(t1 + 3 * HB6, t2 + 3 * HB6, tid, sb, piece - 4);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (STASH) fetch(fetch_ti);
    };

    // prologue: register tile 0 into buffers 0 and 1, register tile 1 in flight
    fetch(0);
    if (want_cs) add_cs();
#pragma unroll
    for (int part = 0; part < 4; ++part) {
        stash6c_part<AKC>(lds, lds + KB6, tid, sa, part);
        stash6c_part<BKC>(lds + 3 * HB6, lds + KB6 + 3 * HB6, tid, sb, part);
    }
    if (PERSIST) next_tile<PERSIST>(g, BM2, BN2, vid, has_next, nm0, nn0);
    fetch(1);
    __syncthreads();

    int u = 0;                                         // k-steps of the stream so far, modulo 3: the buffer of this slot
    int nslot = 0; (void)nslot;
    while (true) {
        for (int ti = 0; ti < nt; ++ti) {
            const int b0 = u, b1 = u == 2 ? 0 : u + 1, b2 = b1 == 2 ? 0 : b1 + 1;
            RLT_G6C_STAMP(nslot, 0);
            slot(BoolTag<false>{}, b0, 0, 0, false, 0);                                   // even slot: k-step 2 ti
            RLT_G6C_STAMP(nslot, 1);
            __syncthreads();
            RLT_G6C_STAMP(nslot, 2);
            ++nslot;
            // odd slot: k-step 2 ti + 1 out of b1; stages register tile ti + 1 into b2 and b0, fetches tile ti + 2
            RLT_G6C_STAMP(nslot, 0);
            slot(BoolTag<true>{}, b1, b2, b0, ti + 1 < nt || has_next, ti + 2);
            RLT_G6C_STAMP(nslot, 1);
            __syncthreads();
            RLT_G6C_STAMP(nslot, 2);
            ++nslot;
            u = b2;
        }
        write_output_t<4>(g, acc, m0 + wm * 64, n0 + wn * 128, true, l31, hh, zslab);
        if (!PERSIST || !has_next) break;
        m0 = nm0; n0 = nn0;
        next_tile<PERSIST>(g, BM2, BN2, vid, has_next, nm0, nn0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }
    if (want_cs) finish_colsum<CsLow4Halves, BM2, false>(g, csum, gsm, tid, m0, zslab);
}

#if defined(RLT_STAMPS)
extern "C" int rlt_debug_g6c_stamps(unsigned long long* host, size_t n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(rlt_g6c_stamp_buf), n * sizeof(unsigned long long));
}
#endif

static_assert(family_is(RLT_GEMM_6C, BM2, BN2, (size_t)3 * KB6 * sizeof(uint16_t)), "gemm_plan.h: GEMM_FAMILY");

}  // namespace

extern "C" int rlt_gemm6c_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st) {
    return with_layout(p.d.ta, p.d.tb, [&](auto TA, auto TB) {
        constexpr bool A_ = decltype(TA)::value, B_ = decltype(TB)::value;
        if constexpr (!A_) if (p.d.persistent) return launch(gemm6c_kernel<A_, B_, true>, p, g, rec, st);      // (A stored [M][K] only)
        return launch(gemm6c_kernel<A_, B_, false>, p, g, rec, st);
    });
}
