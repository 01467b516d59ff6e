// fp32 dense contraction on the f32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products and
// accumulation, 64 FLOP/clk/SIMD = the chip's 157 TFLOP/s fp32 peak).  Serves every nn.Linear-shaped
// product of the hot path and its backward: in_proj / out_proj / FFN of the encoder layer
// (models/AttnCut.py:9), the LSTM input projections (models/AttnCut.py:8) and the weight gradients
// dW = dY^T X (split-K, deterministic slab reduction - no float atomics).
//
// Tiling: 128x128 output tile per 256-thread workgroup (4 wavefronts as 2x2, each 64x64 = 2x2 MFMA
// tiles, 64 accumulator VGPRs), K step 16, operands staged in LDS k-major ([k][m], row 132 floats)
// so that the MFMA operand of lane l (row l&31, k = l>>5) is one conflict-free ds_read_b32; register
// prefetch of the next K tile overlaps the MFMAs of the current one.  blockIdx is remapped so that
// the tiles an XCD runs are contiguous (they share the A panel in that XCD's L2).
// (The frame, the epilogue and the launch: gemm_common.h; the host entry points, split-K reduce included: gemm.hip.)
#include "gemm_common.h"

namespace {

constexpr int LDT = 132;

// KC = true: operand stored [MN][K] (K contiguous)   -> transposing LDS store
// KC = false: operand stored [K][MN] (MN contiguous)  -> direct LDS store
// FAST (host-checked: 16-byte aligned operand, K % 4 == 0, and MN % 4 == 0 for an MN-contiguous operand):
// branch-free - the address is clamped into the matrix, the load is unconditional and out-of-range
// lanes are zeroed with a select.  Guarded loads make hipcc branch around every load and drain vmcnt
// per element, which serialises the whole staging burst.
template <bool KC, int BK, bool FAST>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int ld, int mn0, int k0, int MN, int Kend,
                                          bool vec, int tid, float4 (&reg)[BK / 8]) {
#pragma unroll
    for (int i = 0; i < BK / 8; ++i) {
        const int idx = tid + 256 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (FAST) {
            int r, c;          // r: row of the stored matrix, c: first of 4 contiguous columns
            bool ok;
            if (KC) { r = mn0 + idx / (BK / 4); c = k0 + 4 * (idx % (BK / 4)); ok = r < MN && c < Kend; r = min(r, MN - 1); c = min(c, Kend - 4); }
            else { r = k0 + (idx >> 5); c = mn0 + 4 * (idx & 31); ok = r < Kend && c < MN; r = min(r, Kend - 1); c = min(c, MN - 4); }
            // NOTE: the zero-select for out-of-range lanes is applied in store_tile, NOT here: consuming the
            // loaded value right away would put an s_waitcnt directly behind the load and expose its latency
            (void)ok;
            v = *reinterpret_cast<const float4*>(P + (size_t)r * ld + c);
        } else if (KC) {
            const int row = mn0 + idx / (BK / 4), kk = k0 + 4 * (idx % (BK / 4));
            if (row < MN) {
                const float* src = P + (size_t)row * ld + kk;
                if (vec && kk + 3 < Kend) {
                    v = *reinterpret_cast<const float4*>(src);
                } else {
                    if (kk + 0 < Kend) v.x = src[0];
                    if (kk + 1 < Kend) v.y = src[1];
                    if (kk + 2 < Kend) v.z = src[2];
                    if (kk + 3 < Kend) v.w = src[3];
                }
            }
        } else {
            const int kk = k0 + (idx >> 5), col = mn0 + 4 * (idx & 31);
            if (kk < Kend) {
                const float* src = P + (size_t)kk * ld + col;
                if (vec && col + 3 < MN) {
                    v = *reinterpret_cast<const float4*>(src);
                } else {
                    if (col + 0 < MN) v.x = src[0];
                    if (col + 1 < MN) v.y = src[1];
                    if (col + 2 < MN) v.z = src[2];
                    if (col + 3 < MN) v.w = src[3];
                }
            }
        }
        reg[i] = v;
    }
}

// FAST path: zero, in place, the lanes whose (clamped) load was out of range - called just before the registers
// are consumed (LDS store / bias-gradient side sum), i.e. as late as possible
template <bool KC, int BK>
__device__ __forceinline__ void mask_tile(float4 (&reg)[BK / 8], int tid, int mn0, int k0, int MN, int Kend) {
#pragma unroll
    for (int i = 0; i < BK / 8; ++i) {
        const int idx = tid + 256 * i;
        const bool ok = KC ? (mn0 + idx / (BK / 4) < MN && k0 + 4 * (idx % (BK / 4)) < Kend)
                           : (k0 + (idx >> 5) < Kend && mn0 + 4 * (idx & 31) < MN);
        reg[i] = make_float4(ok ? reg[i].x : 0.f, ok ? reg[i].y : 0.f, ok ? reg[i].z : 0.f, ok ? reg[i].w : 0.f);
    }
}

template <bool KC, int BK>
__device__ __forceinline__ void store_tile(float* __restrict__ T, int tid, const float4 (&reg)[BK / 8]) {
#pragma unroll
    for (int i = 0; i < BK / 8; ++i) {
        const int idx = tid + 256 * i;
        if (KC) {
            const int mn = idx / (BK / 4), k = 4 * (idx % (BK / 4));
            T[(k + 0) * LDT + mn] = reg[i].x;
            T[(k + 1) * LDT + mn] = reg[i].y;
            T[(k + 2) * LDT + mn] = reg[i].z;
            T[(k + 3) * LDT + mn] = reg[i].w;
        } else {
            const int k = idx >> 5, mn = 4 * (idx & 31);
            *reinterpret_cast<float4*>(&T[k * LDT + mn]) = reg[i];
        }
    }
}
template <bool TA, bool TB, int BK, int OCC, bool FAST>
__global__ __launch_bounds__(256, OCC) void gemm_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    float (*As)[BK * LDT] = reinterpret_cast<float (*)[BK * LDT]>(gsm);                    // [2][BK*LDT]
    float (*Bs)[BK * LDT] = reinterpret_cast<float (*)[BK * LDT]>(gsm + 2 * BK * LDT);     // [2][BK*LDT]
    int tid, l31, hh, wm, wn, zslab, tn, m0, n0, kbeg, kend;
    tile_frame<BM, BN>(g, tid, l31, hh, wm, wn, zslab, tn, m0, n0, kbeg, kend);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[BK / 8], rb[BK / 8];
    // A operand: TA=0 -> stored [M][K] (K contiguous); B operand: TB=1 -> stored [N][K] (K contiguous)
    load_tile<!TA, BK, FAST>(g.A, g.lda, m0, kbeg, g.M, kend, g.vecA, tid, ra);
    load_tile<TB, BK, FAST>(g.B, g.ldb, n0, kbeg, g.N, kend, g.vecB, tid, rb);

    // bias gradient on the side: this thread's A elements are 4 consecutive m at fixed k rows
    const bool want_cs = TA && g.colsum != nullptr && tn == 0;
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto add_cs = [&]() {          // (csum_add of gemm_common.h, kept as this kernel's own closure: see decode_block)
#pragma unroll
        for (int i = 0; i < BK / 8; ++i) { csum.x += ra[i].x; csum.y += ra[i].y; csum.z += ra[i].z; csum.w += ra[i].w; }
    };
    const bool whole_mn = m0 + BM <= g.M && n0 + BN <= g.N;
    auto consume = [&](int k0, int buf) {        // mask (fast path), bias-gradient side sum, LDS store
        __builtin_amdgcn_sched_barrier(0);       // do not hoist the first use of the loaded registers above the MFMAs
        if (FAST && !(whole_mn && k0 + BK <= kend)) {       // (scalar test) a whole tile needs no zero-select
            mask_tile<!TA, BK>(ra, tid, m0, k0, g.M, kend);
            mask_tile<TB, BK>(rb, tid, n0, k0, g.N, kend);
        }
        if (want_cs) add_cs();
        store_tile<!TA, BK>(As[buf], tid, ra);
        store_tile<TB, BK>(Bs[buf], tid, rb);
    };
    consume(kbeg, 0);
    __syncthreads();

    int buf = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        const bool more = k0 + BK < kend;
        if (more) {
            load_tile<!TA, BK, FAST>(g.A, g.lda, m0, k0 + BK, g.M, kend, g.vecA, tid, ra);
            load_tile<TB, BK, FAST>(g.B, g.ldb, n0, k0 + BK, g.N, kend, g.vecB, tid, rb);
        }
        const float* a_ = As[buf] + wm * 64 + l31;
        const float* b_ = Bs[buf] + wn * 64 + l31;
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            const int kk = (2 * ks + hh) * LDT;
            const float a0 = a_[kk], a1 = a_[kk + 32];
            const float b0 = b_[kk], b1 = b_[kk + 32];
            acc[0][0] = mfma32(a0, b0, acc[0][0]);
            acc[0][1] = mfma32(a0, b1, acc[0][1]);
            acc[1][0] = mfma32(a1, b0, acc[1][0]);
            acc[1][1] = mfma32(a1, b1, acc[1][1]);
        }
        if (more) consume(k0 + BK, buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    write_output(g, acc, m0, n0, wm, wn, l31, hh, zslab);
    if (want_cs) finish_colsum<CsStride32, BM, true>(g, csum, gsm, tid, m0, zslab);
}

static_assert(family_is(RLT_GEMM_F32, BM, BN, (size_t)4 * 16 * LDT * sizeof(float)), "gemm_plan.h: GEMM_FAMILY");

}  // namespace

extern "C" int rlt_gemm_f32_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st) {
    return with_layout(p.d.ta, p.d.tb, [&](auto TA, auto TB) {
        constexpr bool A_ = decltype(TA)::value, B_ = decltype(TB)::value;
        return p.d.fast ? launch(gemm_kernel<A_, B_, 16, 4, true>, p, g, rec, st) : launch(gemm_kernel<A_, B_, 16, 4, false>, p, g, rec, st);
    });
}
