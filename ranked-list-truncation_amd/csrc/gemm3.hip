// Split-bf16 variant ("bf16x3"): every fp32 operand x is split on the fly into hi = bf16(x) and
// lo = bf16(x - hi); a product a*b is evaluated as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16 MFMA
// (v_mfma_f32_32x32x16_bf16, 16x the rate of the f32 MFMA) with fp32 accumulation.  16 mantissa bits
// per operand: relative error ~2^-16 per product (the dropped lo*lo term and the split residual),
// about 5x the throughput of the exact-fp32 kernel (gemm_f32.hip) at the same interface.
//
// gemm3_kernel, 128 x 128 tile: both operands sit in LDS k-contiguous ([mn][k], rows of 32 bf16 + 8 pad = 80 B) so that a lane's
// MFMA fragment (8 consecutive k of one row) is ONE ds_read_b128; K-contiguous global operands are split and
// stored with ds_write_b64, MN-contiguous ones through a 4x4 register transpose.
#include "gemm3.h"

namespace {

constexpr int LDK3 = 40;                                 // bf16 elements per LDS row
constexpr int TILE3 = 128 * LDK3;                        // one hi or lo tile (elements)

// split4 of split6.h with the four unpacks in front of the subtractions.  The same arithmetic; hipcc schedules the bf16x3 kernels of
// this file differently from the two orders, so the copy stays until a measurement picks one (profiles/bf16_header_isa_identity.md)
__device__ __forceinline__ void split4_unpack_first(float a, float b, float c, float d, uint2& hi, uint2& lo) {
    hi.x = pk2(a, b);
    hi.y = pk2(c, d);
    keep_packed<true>(hi);
    const float ah = lo16(hi.x), bh = hi16(hi.x), ch = lo16(hi.y), dh = hi16(hi.y);
    lo.x = pk2(a - ah, b - bh);
    lo.y = pk2(c - ch, d - dh);
}

// K-contiguous operand ([MN][K]): element idx of the 1024 float4 of a 128 x 32 tile -> (row, 16-byte k chunk).
// Bits: idx = [row>>3][kq>>1 (2 bits)][row&7 (3 bits)][kq&1]: a wavefront still covers 8 rows x 128 contiguous bytes
// of global memory, but the 16 lanes of a ds_write_b64 group hold 8 rows x 2 chunks, whose 4-dword windows at
// 20-dword row stride tile the 32 banks exactly (rows-major lanes, 2 rows x 8 chunks, overlap on 4 banks: a third of
// the LDS cycles of the NT kernel were bank conflicts)
__device__ __forceinline__ int kc_row(int idx) { return ((idx >> 1) & 7) | ((idx >> 6) << 3); }
__device__ __forceinline__ int kc_kq(int idx) { return (idx & 1) | (((idx >> 4) & 3) << 1); }

template <bool KC, bool FAST>
__device__ __forceinline__ void load3(const float* __restrict__ P, int ld, int mn0, int k0, int MN, int Kend, bool vec,
                                      int tid, Stage3& st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (FAST) {     // branch-free: clamp, load, select (see load_tile)
            int r, c;
            bool ok;
            if (KC) { const int idx = tid + 256 * i; r = mn0 + kc_row(idx); c = k0 + 4 * kc_kq(idx); ok = r < MN && c < Kend; r = min(r, MN - 1); c = min(c, Kend - 4); }
            else { r = k0 + 4 * (tid & 7) + i; c = mn0 + 4 * (tid >> 3); ok = r < Kend && c < MN; r = min(r, Kend - 1); c = min(c, MN - 4); }
            (void)ok;          // the zero-select is applied by mask3 just before the registers are consumed
            v = *reinterpret_cast<const float4*>(P + (size_t)r * ld + c);
        } else if (KC) {       // [MN][K]: idx -> (row, 4 consecutive k)
            const int idx = tid + 256 * i;
            const int row = mn0 + kc_row(idx), kk = k0 + 4 * kc_kq(idx);
            if (row < MN) {
                const float* src = P + (size_t)row * ld + kk;
                if (vec && kk + 3 < Kend) v = *reinterpret_cast<const float4*>(src);
                else {
                    if (kk + 0 < Kend) v.x = src[0];
                    if (kk + 1 < Kend) v.y = src[1];
                    if (kk + 2 < Kend) v.z = src[2];
                    if (kk + 3 < Kend) v.w = src[3];
                }
            }
        } else {        // [K][MN]: thread owns a 4(k) x 4(mn) block, i = k row within the block; the k block is the LOW part
                        // of tid so that the 16 lanes of a ds_write_b64 group cover 8 k blocks x 2 rows = 32 distinct
                        // banks (with mn in the low bits the 16 rows are 80 dwords apart: an 8-way bank conflict)
            const int kk = k0 + 4 * (tid & 7) + i, col = mn0 + 4 * (tid >> 3);
            if (kk < Kend) {
                const float* src = P + (size_t)kk * ld + col;
                if (vec && col + 3 < MN) v = *reinterpret_cast<const float4*>(src);
                else {
                    if (col + 0 < MN) v.x = src[0];
                    if (col + 1 < MN) v.y = src[1];
                    if (col + 2 < MN) v.z = src[2];
                    if (col + 3 < MN) v.w = src[3];
                }
            }
        }
        st.v[i] = v;
    }
}

template <bool KC>
__device__ __forceinline__ void mask3(Stage3& st, int tid, int mn0, int k0, int MN, int Kend) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bool ok;
        if (KC) { const int idx = tid + 256 * i; ok = mn0 + kc_row(idx) < MN && k0 + 4 * kc_kq(idx) < Kend; }
        else ok = k0 + 4 * (tid & 7) + i < Kend && mn0 + 4 * (tid >> 3) < MN;
        st.v[i] = make_float4(ok ? st.v[i].x : 0.f, ok ? st.v[i].y : 0.f, ok ? st.v[i].z : 0.f, ok ? st.v[i].w : 0.f);
    }
}

template <bool KC>
__device__ __forceinline__ void store3(uint16_t* __restrict__ Thi, uint16_t* __restrict__ Tlo, int tid, const Stage3& st) {
    if (KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            const int mn = kc_row(idx), k = 4 * kc_kq(idx);
            uint2 hi, lo;
            split4_unpack_first(st.v[i].x, st.v[i].y, st.v[i].z, st.v[i].w, hi, lo);
            *reinterpret_cast<uint2*>(Thi + mn * LDK3 + k) = hi;
            *reinterpret_cast<uint2*>(Tlo + mn * LDK3 + k) = lo;
        }
    } else {
        const int k = 4 * (tid & 7), mn = 4 * (tid >> 3);
        const float* f0 = reinterpret_cast<const float*>(&st.v[0]);
        const float* f1 = reinterpret_cast<const float*>(&st.v[1]);
        const float* f2 = reinterpret_cast<const float*>(&st.v[2]);
        const float* f3 = reinterpret_cast<const float*>(&st.v[3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint2 hi, lo;
            split4_unpack_first(f0[c], f1[c], f2[c], f3[c], hi, lo);
            *reinterpret_cast<uint2*>(Thi + (mn + c) * LDK3 + k) = hi;
            *reinterpret_cast<uint2*>(Tlo + (mn + c) * LDK3 + k) = lo;
        }
    }
}

template <bool TA, bool TB, bool FAST>
__global__ __launch_bounds__(256, 2) void gemm3_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    uint16_t* lds = reinterpret_cast<uint16_t*>(gsm);        // [buf][A_hi | A_lo | B_hi | B_lo][TILE3]
    int tid, l31, hh, wm, wn, zslab, tn, m0, n0, kbeg, kend;
    tile_frame<BM, BN>(g, tid, l31, hh, wm, wn, zslab, tn, m0, n0, kbeg, kend);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // two register stages: while tile t is multiplied out of LDS, tile t+1 sits in registers and tile t+2 is
    // in flight, i.e. two K tiles of global loads are outstanding per thread (the kernel is bound by
    // bytes-in-flight x latency, not by the MFMA pipe)
    Stage3 a0, b0, a1, b1;
    const bool edge = m0 + BM > g.M || n0 + BN > g.N || ((kend - kbeg) & (BK3 - 1)) != 0;      // workgroup-uniform
    const bool want_cs = TA && g.colsum != nullptr && tn == 0;
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int t, Stage3& sa, Stage3& sb) {
        const int k0 = kbeg + t * BK3;
        load3<!TA, FAST>(g.A, g.lda, m0, k0, g.M, kend, g.vecA, tid, sa);
        load3<TB, FAST>(g.B, g.ldb, n0, k0, g.N, kend, g.vecB, tid, sb);
    };
    // consume tile t's registers: mask (fast path), bias-gradient side sum, split + LDS store.  Nothing touches
    // the loaded values before this point, so the loads stay in flight across the MFMA block.
    auto stash = [&](int t, int buf, Stage3& sa, Stage3& sb) {
        // keep the compiler from hoisting the first use of the loaded registers (and with it their s_waitcnt)
        // above the MFMA block that is meant to hide the load latency
        __builtin_amdgcn_sched_barrier(0);
        const int k0 = kbeg + t * BK3;
        if (FAST && edge) {            // interior workgroups with whole K tiles load nothing out of range
            mask3<!TA>(sa, tid, m0, k0, g.M, kend);
            mask3<TB>(sb, tid, n0, k0, g.N, kend);
        }
        if (want_cs) csum_add(csum, sa.v);
        uint16_t* nb = lds + buf * 4 * TILE3;
        store3<!TA>(nb + 0 * TILE3, nb + 1 * TILE3, tid, sa);
        store3<TB>(nb + 2 * TILE3, nb + 3 * TILE3, tid, sb);
    };
    auto multiply = [&](int buf) {
        const uint16_t* base = lds + buf * 4 * TILE3;
        const uint16_t* pa = base + (wm * 64 + l31) * LDK3 + 8 * hh;
        const uint16_t* pb = base + 2 * TILE3 + (wn * 64 + l31) * LDK3 + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * LDK3 + ks * 16);
                al[i] = *reinterpret_cast<const bf16x8*>(pa + TILE3 + i * 32 * LDK3 + ks * 16);
                bh[i] = *reinterpret_cast<const bf16x8*>(pb + i * 32 * LDK3 + ks * 16);
                bl[i] = *reinterpret_cast<const bf16x8*>(pb + TILE3 + i * 32 * LDK3 + ks * 16);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
    };
    const int nt = (kend - kbeg + BK3 - 1) / BK3;
    fetch(0, a0, b0);
    stash(0, 0, a0, b0);
    if (nt > 1) fetch(1, a0, b0);
    if (nt > 2) fetch(2, a1, b1);
    __syncthreads();
    for (int t = 0; t < nt; t += 2) {
        multiply(0);                                   // tile t;   regs0 = tile t+1, regs1 = tile t+2 (in flight)
        if (t + 1 < nt) stash(t + 1, 1, a0, b0);
        if (t + 3 < nt) fetch(t + 3, a0, b0);
        __syncthreads();
        if (t + 1 >= nt) break;
        multiply(1);                                   // tile t+1; regs1 = tile t+2, regs0 = tile t+3 (in flight)
        if (t + 2 < nt) stash(t + 2, 0, a1, b1);
        if (t + 4 < nt) fetch(t + 4, a1, b1);
        __syncthreads();
    }
    write_output(g, acc, m0, n0, wm, wn, l31, hh, zslab);
    if (want_cs) finish_colsum<CsLow8, BM, true>(g, csum, gsm, tid, m0, zslab);
}

// ======================================================================================================
// 256 x 256 tile, 8 wavefronts (4 x 2, each 64 x 128: 128 accumulator VGPRs), one workgroup per CU.
// The 128 x 128 kernel above moves (128 + 128) * K * 4 bytes from L2 per 128 * 128 * K MACs; measured, every large
// product here drives the L2 at 9-10.7 TB/s of request bandwidth (TCC_REQ, profiles/r01_h_ablation_notes.md) - that,
// not the matrix pipe or HBM, is what the 128-wide tiles saturate.  A 256 x 256 tile halves the L2 bytes per MAC
// and cuts the LDS fragment reads per MFMA from 0.67 to 0.5.  Interior tiles and whole K tiles only (the host falls
// back to gemm3_kernel otherwise).  LDS: [buf][A_hi | A_lo | B_hi | B_lo], planes of 256 rows x 64 bytes (32 bf16),
// no padding: the four 16-byte chunks of a row are XOR-swizzled with (row >> 2) & 3, which makes the ds_read_b128
// fragment reads conflict-free for the instruction's lane groups; 2 x 64 KB.  (Row permutation, swizzle and loader: gemm3.h.)

// one quarter (`part` = 0..3) of the split + LDS store of a staged operand tile
template <bool KC>
__device__ __forceinline__ void store3b_part(uint16_t* __restrict__ Thi, uint16_t* __restrict__ Tlo, int tid, const Stage3& st, int part) {
    if (KC) {
        const int idx = tid + 512 * part;
        const int row = prow2(kcb_row(idx)), kq = idx & 7;
        const int off = row * 32 + 8 * swz2(row, kq >> 1) + 4 * (kq & 1);
        uint2 hi, lo;
        split4_unpack_first(st.v[part].x, st.v[part].y, st.v[part].z, st.v[part].w, hi, lo);
        *reinterpret_cast<uint2*>(Thi + off) = hi;
        *reinterpret_cast<uint2*>(Tlo + off) = lo;
    } else {
        const int kb = tid & 7, mb = tid >> 3;
        const float* f0 = reinterpret_cast<const float*>(&st.v[0]);
        const float* f1 = reinterpret_cast<const float*>(&st.v[1]);
        const float* f2 = reinterpret_cast<const float*>(&st.v[2]);
        const float* f3 = reinterpret_cast<const float*>(&st.v[3]);
        // offset of part 0; the other three follow from it by one xor-add (prow2 puts bit 0 of the part into row bit 2, which
        // is also the low bit of the row's swizzle key).  Kept opaque so that ONE offset register lives across the K loop:
        // hoisted as four, the fourth was spilled in the persistent NN kernel and its reload (a scratch load, in order
        // behind the tile prefetch) made every K tile wait for all loads in flight.
        int base = ((mb >> 1) * 8 + (mb & 1)) * 32 + 4 * (kb & 1) + 8 * ((kb >> 1) ^ (((mb >> 1) & 1) * 2));
        asm volatile("" : "+v"(base));
        const int off = (base ^ (8 * (part & 1))) + 128 * (part & 1) + 64 * (part >> 1);
        uint2 hi, lo;
        split4_unpack_first(f0[part], f1[part], f2[part], f3[part], hi, lo);
        *reinterpret_cast<uint2*>(Thi + off) = hi;
        *reinterpret_cast<uint2*>(Tlo + off) = lo;
    }
}
template <bool KC>
__device__ __forceinline__ void store3b(uint16_t* __restrict__ Thi, uint16_t* __restrict__ Tlo, int tid, const Stage3& st) {
#pragma unroll
    for (int part = 0; part < 4; ++part) store3b_part<KC>(Thi, Tlo, tid, st, part);
}

#if defined(RLT_STAMPS)
// timeline instrumentation (variant builds only): s_memtime at four points of one workgroup of gemm3b_kernel, per wavefront
__device__ unsigned long long rlt_gemm_stamp_buf[8 * 4];
#define RLT_GSTAMP(slot) do { if (blockIdx.x == gridDim.x / 2 && (threadIdx.x & 63) == 0) \
    rlt_gemm_stamp_buf[(threadIdx.x >> 6) * 4 + (slot)] = __builtin_readcyclecounter(); } while (0)
#else
#define RLT_GSTAMP(slot) do {} while (0)
#endif

// PERSIST (no split-K, A stored [M][K], at least two K tiles, more tiles than workgroups): gridDim.x workgroups walk the
// tiles id, id + gridDim.x, ... as ONE stream of K tiles - the operand tiles of the next output tile are fetched and
// stashed during the last K tiles of the current one, and its epilogue stores go out while those loads are in flight.
// One workgroup per output tile paid the pipeline start-up (two exposed HBM latencies, ~6,000 cycles) and ran its first
// K tiles against cold loads for every tile: at K = 256 (8 K tiles) that was 57,000 cycles per tile for 24,600 of
// MFMA work (timeline stamps, profiles/r02_notes.md).
template <bool TA, bool TB, bool PERSIST = false>
__global__ __launch_bounds__(512) void gemm3b_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    uint16_t* lds = reinterpret_cast<uint16_t*>(gsm);
    int tid, l31, hh, wm, wn, zslab, tn, m0, n0, kbeg, kend;
    tile_frame<BM2, BN2>(g, tid, l31, hh, wm, wn, zslab, tn, m0, n0, kbeg, kend);      // g.tiles_* count 256-wide tiles here

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    Stage3 sa, sb;
    const bool want_cs = TA && g.colsum != nullptr && tn == 0;
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int t) {
        const int k0 = kbeg + t * BK3;
        load3b<!TA>(g.A, g.lda, m0, k0, tid, sa);
        load3b<TB>(g.B, g.ldb, n0, k0, tid, sb);
    };
    auto stash = [&](int buf) {
        if (want_cs) csum_add(csum, sa.v);
        uint16_t* nb = lds + buf * 4 * PL2;
        store3b<!TA>(nb, nb + PL2, tid, sa);
        store3b<TB>(nb + 2 * PL2, nb + 3 * PL2, tid, sb);
    };
    // fragment rows: row bases are multiples of 32, so the physical row is base + prow2(l31) and its swizzle key is fixed
    const int pl = prow2(l31);
    const int sw = (pl >> 2) & 3;
    // 8 steps (k-step ks, 32-column block j) of 6 MFMAs; the B fragments of the next step (and the A fragments of the
    // next k-step) are read while the current step multiplies.  The scheduling fences keep the compiler from hoisting
    // all 24 fragment reads to the top (96 more live VGPRs than the 256 available).
    // The split + LDS store of the NEXT tile (registers sa, sb) is spread over steps 4..7, two quarters per step, right
    // behind that step's MFMAs: the wavefront issues the VALU work while its MFMAs execute.  With the stash after the
    // whole multiply, the two wavefronts of a SIMD (same workgroup, in lock-step between the barriers) both sit in their
    // MFMA phase, then both in their VALU phase, and the two pipes take turns.  The global loads of tile t+2 follow the
    // last use of each staging register (A after step 5, B after step 7): a full iteration of latency cover.
    // tile of the stream after the current one (PERSIST)
    int vid = blockIdx.x, nm0 = m0, nn0 = n0;
    bool has_next = false;
    auto multiply = [&](int buf, int t, int nt_) {
        const uint16_t* pa = lds + buf * 4 * PL2 + (wm * 64 + pl) * 32;
        const uint16_t* pb = lds + buf * 4 * PL2 + 2 * PL2 + (wn * 128 + pl) * 32;
        uint16_t* nb = lds + (buf ^ 1) * 4 * PL2;
        // the fetch of tile t+2 is unconditional (the last two iterations re-read the last tile into registers nobody
        // consumes): with the loads behind a branch hipcc merges the outstanding-load counts of both paths and waits
        // for the loads it has just issued (vmcnt(3..0) at every staging step instead of vmcnt(7..4)), which exposed
        // one full memory latency per 32-wide K step
        const bool do_stash = t + 1 < nt_ || has_next;
        // K tile t+2 of the stream: of this output tile, or K tile t+2-nt of the next one
        const bool wrap = PERSIST && has_next && t + 2 >= nt_;
        const int kf = kbeg + (wrap ? t + 2 - nt_ : min(t + 2, nt_ - 1)) * BK3;
        const int fm0 = wrap ? nm0 : m0, fn0 = wrap ? nn0 : n0;
        bf16x8 ah[2][2], al[2][2], bh[2], bl[2];
        auto load_a = [&](int ks, int slot) {
            const int co = 8 * ((2 * ks + hh) ^ sw);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[slot][i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * 32 + co);
                al[slot][i] = *reinterpret_cast<const bf16x8*>(pa + PL2 + i * 32 * 32 + co);
            }
        };
        auto load_b = [&](int ks, int j, int slot) {
            const int co = 8 * ((2 * ks + hh) ^ sw);
            bh[slot] = *reinterpret_cast<const bf16x8*>(pb + j * 32 * 32 + co);
            bl[slot] = *reinterpret_cast<const bf16x8*>(pb + PL2 + j * 32 * 32 + co);
        };
        load_a(0, 0);
        load_b(0, 0, 0);
#pragma unroll
        for (int step = 0; step < 8; ++step) {
            const int ks = step >> 2, j = step & 3;
            if (step + 1 < 8) load_b((step + 1) >> 2, (step + 1) & 3, (step + 1) & 1);
            if (step == 2) load_a(1, 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ks][i], bh[step & 1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks][i], bl[step & 1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks][i], bh[step & 1], acc[i][j], 0, 0, 0);
            }
            (void)sa, (void)sb;       // named here first: a closure captures in the order of first use, and hipcc's output follows that order
            if (step >= 4 && do_stash) {
                if (step == 4 && want_cs) csum_add(csum, sa.v);
                if (step < 6) {
                    store3b_part<!TA>(nb, nb + PL2, tid, sa, 2 * (step - 4));
                    store3b_part<!TA>(nb, nb + PL2, tid, sa, 2 * (step - 4) + 1);
                } else {
                    store3b_part<TB>(nb + 2 * PL2, nb + 3 * PL2, tid, sb, 2 * (step - 6));
                    store3b_part<TB>(nb + 2 * PL2, nb + 3 * PL2, tid, sb, 2 * (step - 6) + 1);
                }
            }
            if (step == 5) load3b<!TA>(g.A, g.lda, fm0, kf, tid, sa);
            if (step == 7) load3b<TB>(g.B, g.ldb, fn0, kf, tid, sb);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    const int nt = (kend - kbeg) / BK3;
    RLT_GSTAMP(0);
    fetch(0);
    stash(0);
    fetch(min(1, nt - 1));                             // unconditional, like the fetches in multiply()
    __syncthreads();
    RLT_GSTAMP(1);
    if (PERSIST) next_tile<PERSIST>(g, BM2, BN2, vid, has_next, nm0, nn0);
    int u = 0;                                       // K tiles of the stream so far (LDS buffer parity)
    while (true) {
        for (int t = 0; t < nt; ++t, ++u) {
            multiply(u & 1, t, nt);                    // K tile t; stashes the next K tile of the stream (in registers), fetches the one after
            __syncthreads();
        }
        RLT_GSTAMP(2);
        write_output_t<4>(g, acc, m0 + wm * 64, n0 + wn * 128, true, l31, hh, zslab);
        RLT_GSTAMP(3);
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
    // (no barrier before the LDS write: the K loop ended on one and the epilogue reads no LDS)
    if (want_cs) finish_colsum<CsLow8, BM2, false, false>(g, csum, gsm, tid, m0, zslab);
}

#if defined(RLT_STAMPS)
extern "C" int rlt_debug_gemm_stamps(unsigned long long* host, size_t n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(rlt_gemm_stamp_buf), n * sizeof(unsigned long long));
}
#endif

static_assert(family_is(RLT_GEMM_3, BM, BN, (size_t)2 * 4 * TILE3 * sizeof(uint16_t)) &&
              family_is(RLT_GEMM_3B, BM2, BN2, (size_t)2 * 4 * PL2 * sizeof(uint16_t)), "gemm_plan.h: GEMM_FAMILY");

}  // namespace

extern "C" int rlt_gemm3_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st) {
    return with_layout(p.d.ta, p.d.tb, [&](auto TA, auto TB) {
        constexpr bool A_ = decltype(TA)::value, B_ = decltype(TB)::value;
        auto go = [&](auto kern) { return launch(kern, p, g, rec, st); };
        if (p.d.family == RLT_GEMM_3) return p.d.fast ? go(gemm3_kernel<A_, B_, true>) : go(gemm3_kernel<A_, B_, false>);
        if constexpr (!A_) if (p.d.persistent) return go(gemm3b_kernel<A_, B_, true>);      // (the persistent form exists for A stored [M][K] only)
        return go(gemm3b_kernel<A_, B_>);
    });
}
