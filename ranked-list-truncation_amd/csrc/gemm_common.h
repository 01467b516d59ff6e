// The frame every tiled product kernel of the GEMM family is built on (gemm_f32.hip, gemm3.hip, gemm6.hip, gemm6c.hip, gemm6e.hip;
// the host side is gemm.hip, the plan gemm_plan.hip): the kernel argument block, the workgroup's place in the tile walk, the
// output epilogues, the side column sum of A, and the launch.
//
// Everything here sits in the unnamed namespace, GemmArgs included: the kernels are local to their file and their symbols carry
// GemmArgs under that namespace.  A C++ function that takes a GemmArgs can therefore not be called across files; the family
// launchers at the end have C linkage, which leaves the parameter types out of their names.
#pragma once
#include "common.h"
#include "gemm_plan.h"
#include "split6.h"
#include <type_traits>

namespace {

constexpr int BM = 128, BN = 128;        // output tile of gemm_kernel and gemm3_kernel (the larger tiles: gemm3.h, gemm6.hip)

struct GemmArgs {
    const float* A; const float* B; float* C;
    const float* bias; const float* bias2;
    int M, N, K, lda, ldb, ldc;
    int vecA, vecB;      // 16-byte vector loads allowed
    int flags;
    int kchunk;          // K range per z-slice (multiple of BK); gridDim.z slices
    float* slab;         // split-K partials [z][M*N] or null
    int tiles_m, tiles_n;
    const float* mask; int ldmask;   // epilogue: C = mask > 0 ? C : 0   (ReLU backward fused in dX)
    float* colsum;       // [M]: sum_k op(A)[m][k] (bias gradient from the dW product), TA only; or null
    float* cs_slab;      // split-K partials of colsum [z][M] or null
    float drop_p; uint32_t drop_thr, seed;   // epilogue dropout on the output (after ReLU), keep -> /(1-p)
    float mask_scale;    // with `mask`: kept elements are multiplied by this (1/(1-p) of the forward dropout)
    int slab_xcd;        // split-K launched as a 1-D grid with K slabs pinned to XCDs (see decode_block)
    // 1-bit masks, packed along ROWS: bit (row & 31) of word [(row >> 5) * ldbits + col], ldbits = N.  In the MFMA
    // accumulator layout a lane owns one column and 16 of the 32 rows of a block (the other 16 sit in lane ^ 32), so a
    // 32-row x 32-column block is ONE coalesced 128-byte word store / load per wavefront (packed along columns it took a
    // ballot and a one-lane store per accumulator register: 128 of each per wavefront and 256 x 256 tile)
    uint32_t* bits_out;  // with RLT_GEMM_RELU: bit = (C > 0)
    const uint32_t* bits_in;   // epilogue mask from such bits: C = bit ? C * mask_scale : 0
    int ldbits;
};
// what the C-linkage launchers below rely on: every file's GemmArgs is this one plain block of bytes
static_assert(std::is_standard_layout<GemmArgs>::value && std::is_trivially_copyable<GemmArgs>::value && sizeof(GemmArgs) == 176,
              "GemmArgs crosses translation units by reference");

// (tile, K slab) of this workgroup.
//  * no split-K, or a split count that is not a multiple of 8: XCD-aware bijective remap of the flat tile id (the
//    tiles an XCD runs are contiguous and share operand panels in that XCD's L2); slab = blockIdx.z.
//  * split-K with nsplit % 8 == 0, launched as a 1-D grid of tiles x nsplit: under round-robin dispatch XCD c gets the
//    ids = c (mod 8); it is given the K slabs z = c (mod 8) and runs ALL tiles of a slab together, so every slab of A
//    and B is fetched from HBM by exactly one XCD and shared by that slab's tiles through its L2.  (With tiles spread
//    over XCDs instead, each XCD streams the whole small operand: 8x its bytes - measured 20 GB instead of 11 GB on
//    the FFN weight gradients.)
__device__ __forceinline__ int xcd_remap(int id, int n_tiles) {
    const int q = n_tiles >> 3, r = n_tiles & 7, xcd = id & 7, j = id >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
__device__ __forceinline__ void decode_block(const GemmArgs& g, int& bid, int& z) {
    const int nwg = g.tiles_m * g.tiles_n;
    const int id = blockIdx.x;
    if (g.slab_xcd) {
        const int xcd = id & 7, j = id >> 3, grp = j / nwg;
        z = grp * 8 + xcd;
        bid = j - grp * nwg;
    } else {
        const int q = nwg >> 3, r = nwg & 7, xcd = id & 7, j = id >> 3;         // xcd_remap(id, nwg), written out: with the call
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;      // here and csum_add in gemm_kernel, its code changed
        z = blockIdx.z;
    }
}

// What a kernel computes first: the lane's place in an MFMA block (l31, hh), the wavefront's in the workgroup (wm x wn: 2 x 2 in
// the 256-thread kernels, 4 x 2 in the 512-thread ones, by the same two expressions), the TBM x TBN output tile and the K range.
// A plain function that fills the kernel's own variables - returned as a struct, the values landed in other registers.  Used by
// gemm_kernel, gemm3_kernel, gemm3b_kernel and gemm6_kernel; gemm6b, gemm6c and gemm6e compile to other code through it and keep
// these statements written out (profiles/gemm_split_equivalence.md).
template <int TBM, int TBN>
__device__ __forceinline__ void tile_frame(const GemmArgs& g, int& tid, int& l31, int& hh, int& wm, int& wn, int& zslab, int& tn,
                                           int& m0, int& n0, int& kbeg, int& kend) {
    tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    l31 = lane & 31; hh = lane >> 5;
    wm = wv >> 1; wn = wv & 1;
    int bid;
    decode_block(g, bid, zslab);
    const int tm = bid / g.tiles_n;
    tn = bid - tm * g.tiles_n;
    m0 = tm * TBM; n0 = tn * TBN;
    kbeg = zslab * g.kchunk;
    kend = min(g.K, kbeg + g.kchunk);
}

// The persistent kernels walk the tiles id, id + gridDim.x, ... as one stream: the step to the tile after the current one, under
// decode_block's remap.  (vid, has_next, nm0, nn0) are the kernel's own variables.
template <bool PERSIST>
__device__ __forceinline__ void next_tile(const GemmArgs& g, int bm, int bn, int& vid, bool& has_next, int& nm0, int& nn0) {
    const int nwg = g.tiles_m * g.tiles_n;
    vid += gridDim.x;
    has_next = PERSIST && vid < nwg;
    if (has_next) {
        const int nb = xcd_remap(vid, nwg);
        const int ntm = nb / g.tiles_n;
        nm0 = ntm * bm; nn0 = (nb - ntm * g.tiles_n) * bn;
    }
}

__device__ __forceinline__ float gemm_epilogue(const GemmArgs& g, float v, float bv, int row, int col, const float* dst) {
    v += bv;
    if (g.flags & RLT_GEMM_ACCUMULATE) v += *dst;
    if (g.flags & RLT_GEMM_RELU) v = fmaxf(v, 0.f);
    if (g.mask) v = (g.mask[(size_t)row * g.ldmask + col] > 0.f) ? v * g.mask_scale : 0.f;
    if (g.drop_p > 0.f) v = rlt_keep(g.seed, (uint32_t)row, (uint32_t)col, g.drop_thr) ? v * (1.f / (1.f - g.drop_p)) : 0.f;
    return v;
}
// ---- shared epilogue: accumulator tiles -> C (or split-K slab), fused bias/ReLU/mask/dropout -------
// wavefront tile = 64 rows (2 MFMA blocks) x 32*NJ columns at (rbase, cbase); `interior`: the whole workgroup tile is
// inside C
template <bool V> struct BoolTag { static constexpr bool value = V; };
template <int NJ>
__device__ __forceinline__ void write_output_t(const GemmArgs& g, const f32x16 (&acc)[2][NJ], int rbase, int cbase,
                                               bool interior, int l31, int hh, int z) {
    const bool to_slab = g.slab != nullptr;
    float* out = to_slab ? g.slab + (size_t)z * g.M * g.N : g.C;
    const int ldo = to_slab ? g.N : g.ldc;
    // interior tiles with one of the common epilogues: the bounds and mode tests are hoisted out of the per-element
    // loop (tested per element they cost >1 ms of a K = 256 product that writes 10 GB)
    // Addressing of the interior paths: the row base out + (rb + 32 i + dr) * ldo + cb + 32 j is WAVE-UNIFORM (rb, cb are
    // made scalar with readfirstlane) and every lane adds the same 32-bit element offset 4 hh ldo + l31 to all of them, so
    // a store is `global_store_dword v_off, v_data, s[base]` with the bases stepped on the scalar unit.  With the
    // per-lane 64-bit address arithmetic the compiler generated before (rbase derived from threadIdx in VGPRs), the 128
    // stores of a wavefront cost ~5 VALU instructions and two address registers each and the epilogue spilled.
    const int rb = __builtin_amdgcn_readfirstlane(rbase), cb = __builtin_amdgcn_readfirstlane(cbase);
    const int loff = 4 * hh * ldo + l31;
    if (interior && g.drop_p <= 0.f) {
        auto tile = [&](auto f) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = cb + j * 32 + l31;
                float bv = 0.f;
                if (!to_slab) {
                    if (g.bias) bv += g.bias[col];
                    if (g.bias2) bv += g.bias2[col];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dr = (r & 3) + 8 * (r >> 2);
                        float* base = out + (size_t)(rb + i * 32 + dr) * ldo + (cb + j * 32);       // scalar
                        base[loff] = f(acc[i][j][r] + bv, rb + i * 32 + dr + 4 * hh, col, base + loff);
                    }
                }
            }
        };
        const bool relu = g.flags & RLT_GEMM_RELU, accum = g.flags & RLT_GEMM_ACCUMULATE;
        if (to_slab || (!relu && !accum && !g.mask && !g.bits_in)) { tile([](float v, int, int, const float*) { return v; }); return; }
        if (relu && !accum && !g.mask && !g.bits_out && !g.bits_in) { tile([](float v, int, int, const float*) { return fmaxf(v, 0.f); }); return; }
        if (accum && !relu && !g.mask && !g.bits_in) { tile([](float v, int, int, const float* d) { return v + *d; }); return; }
        if (((g.bits_out && relu) || (g.bits_in && !relu)) && !accum && !g.mask && !to_slab) {
            // 1-bit masks (packed along rows): one word per lane and 32 x 32 block, written / read once
            const float sc = g.mask_scale;
            auto body = [&](auto wr_tag) {
            constexpr bool wr = decltype(wr_tag)::value;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = cb + j * 32 + l31;
                float bv = 0.f;
                if (g.bias) bv += g.bias[col];
                if (g.bias2) bv += g.bias2[col];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const size_t widx = (size_t)((rb + i * 32) >> 5) * g.ldbits + (cb + j * 32);      // scalar
                    uint32_t w = wr ? 0u : (g.bits_in + widx)[l31];
                    if (!wr) w >>= 4 * hh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dr = (r & 3) + 8 * (r >> 2);
                        float v = acc[i][j][r] + bv;
                        if (wr) {
                            v = fmaxf(v, 0.f);
                            w |= (v > 0.f ? 1u : 0u) << dr;
                        } else {
                            v = ((w >> dr) & 1u) ? v * sc : 0.f;
                        }
                        (out + (size_t)(rb + i * 32 + dr) * ldo + (cb + j * 32))[loff] = v;
                    }
                    if (wr) {
                        w <<= 4 * hh;
                        const uint32_t full = w | (uint32_t)__shfl_xor((int)w, 32, 64);
                        if (hh == 0) (g.bits_out + widx)[l31] = full;
                    }
                }
            }
            };
            if (g.bits_out) body(BoolTag<true>{}); else body(BoolTag<false>{});
            return;
        }
        if (g.mask && !relu && !accum && !g.bits_in && !g.bits_out) {
            const float* mk = g.mask; const int ldm = g.ldmask; const float sc = g.mask_scale;
            tile([=](float v, int row, int col, const float*) { return mk[(size_t)row * ldm + col] > 0.f ? v * sc : 0.f; });
            return;
        }
    }
    // interior tiles of the FFN hidden product in train mode: bias + ReLU + dropout (+ the 1-bit mask of what
    // survived both).  Row hashes of the two half-wave rows are wave-uniform (scalar unit); one column hash per lane
    if (interior && g.drop_p > 0.f && (g.flags & RLT_GEMM_RELU) && !(g.flags & RLT_GEMM_ACCUMULATE) && !g.mask && !g.bits_in &&
        !to_slab) {
        const float inv_keep = 1.f / (1.f - g.drop_p);
        const uint32_t thr = g.drop_thr, seed = g.seed;
        auto tile = [&](auto with_bits) {
            uint32_t hc[NJ];
            float bv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = cb + j * 32 + l31;
                hc[j] = rlt_col_hash(seed, (uint32_t)col);
                bv[j] = 0.f;
                if (g.bias) bv[j] += g.bias[col];
                if (g.bias2) bv[j] += g.bias2[col];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                uint32_t w[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) w[j] = 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row_lo = rb + i * 32 + (r & 3) + 8 * (r >> 2);
                    // readfirstlane keeps both hashes on the scalar unit (without it hipcc folds the select below into
                    // one per-lane hash of row_lo + 4*hh on the VALU: 64 hashes and as many live registers per lane)
                    const uint32_t h0 = __builtin_amdgcn_readfirstlane(rlt_row_hash(seed, (uint32_t)row_lo));
                    const uint32_t h1 = __builtin_amdgcn_readfirstlane(rlt_row_hash(seed, (uint32_t)(row_lo + 4)));
                    const uint32_t hr = hh ? h1 : h0;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        float v = fmaxf(acc[i][j][r] + bv[j], 0.f);
                        v = rlt_keep_rc(hr, hc[j], thr) ? v * inv_keep : 0.f;
                        if (decltype(with_bits)::value) w[j] |= (v > 0.f ? 1u : 0u) << acc_row(r, hh);
                        (out + (size_t)row_lo * ldo + (cb + j * 32))[loff] = v;
                    }
                }
                if (decltype(with_bits)::value) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const uint32_t full = w[j] | (uint32_t)__shfl_xor((int)w[j], 32, 64);
                        if (hh == 0) (g.bits_out + (size_t)((rb + i * 32) >> 5) * g.ldbits + (cb + j * 32))[l31] = full;
                    }
                }
            }
        };
        if (g.bits_out) tile(BoolTag<true>{}); else tile(BoolTag<false>{});
        return;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = cbase + j * 32 + l31;
        const bool col_ok = col < g.N;
        float bv = 0.f;
        if (!to_slab && col_ok) {
            if (g.bias) bv += g.bias[col];
            if (g.bias2) bv += g.bias2[col];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const size_t widx = (size_t)((rbase + i * 32) >> 5) * g.ldbits + col;
            const bool blk_ok = col_ok && rbase + i * 32 < g.M;
            const uint32_t win = (!to_slab && g.bits_in && blk_ok) ? g.bits_in[widx] : 0u;
            uint32_t wout = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + i * 32 + acc_row(r, hh);
                if (row >= g.M || !col_ok) continue;
                float v = acc[i][j][r];
                float* dst = out + (size_t)row * ldo + col;
                if (!to_slab) v = gemm_epilogue(g, v, bv, row, col, dst);
                if (!to_slab && g.bits_in) v = ((win >> acc_row(r, hh)) & 1u) ? v * g.mask_scale : 0.f;
                wout |= (v > 0.f ? 1u : 0u) << acc_row(r, hh);
                *dst = v;
            }
            if (!to_slab && g.bits_out) {          // rows beyond M keep a zero bit
                const uint32_t full = wout | (uint32_t)__shfl_xor((int)wout, 32, 64);
                if (hh == 0 && blk_ok) g.bits_out[widx] = full;
            }
        }
    }
}

__device__ __forceinline__ void write_output(const GemmArgs& g, const f32x16 (&acc)[2][2], int m0, int n0,
                                             int wm, int wn, int l31, int hh, int z) {
    write_output_t<2>(g, acc, m0 + wm * 64, n0 + wn * 64, m0 + BM <= g.M && n0 + BN <= g.N, l31, hh, z);
}

// ---- side column sum of A (the bias gradient out of a dW product) -----------------------------------
// Every thread adds the A elements it stages: four consecutive columns m at its own k rows.
template <int N>
__device__ __forceinline__ void csum_add(float4& csum, const float4 (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) { csum.x += v[i].x; csum.y += v[i].y; csum.z += v[i].z; csum.w += v[i].w; }
}
// PARTS threads hold partial sums of the same column group (columns 4 c .. 4 c + 3 of the tile), by the kernel's staging map:
// slot(c, j) is the thread that holds part j of group c.
struct CsStride32 {          // gemm_kernel: threads c, c + 32, ...
    static constexpr int PARTS = 8;
    static __device__ __forceinline__ int slot(int c, int j) { return c + 32 * j; }
};
struct CsLow8 {              // gemm3, gemm3b, gemm6, gemm6b: tid = 8 mb + kb, the k index in the low lane bits
    static constexpr int PARTS = 8;
    static __device__ __forceinline__ int slot(int c, int j) { return 8 * c + j; }
};
struct CsLow4Halves {        // gemm6c: threads 4 mb + kb and 256 + 4 mb + kb (kb < 4), one per k-step of the register tile
    static constexpr int PARTS = 8;
    static __device__ __forceinline__ int slot(int c, int j) { return (j >> 2) * 256 + 4 * c + (j & 3); }
};
struct CsLow4 {              // gemm6e: threads 4 mb + kb (kb < 4)
    static constexpr int PARTS = 4;
    static __device__ __forceinline__ int slot(int c, int j) { return 4 * c + j; }
};
// Reduce them through LDS and write the ROWS sums of this tile.  EDGE: the tile may reach past M (the 128-row kernels; the
// 256-row ones run whole tiles only).  PRE_SYNC: a barrier before the LDS is overwritten - every kernel needs it but gemm3b,
// whose K loop ends on a barrier with nothing read from LDS after it.
template <class MAP, int ROWS, bool EDGE, bool PRE_SYNC = true>
__device__ __forceinline__ void finish_colsum(const GemmArgs& g, float4 csum, float* lds, int tid, int m0, int z) {
    float4* red = reinterpret_cast<float4*>(lds);
    if (PRE_SYNC) __syncthreads();
    red[tid] = csum;
    __syncthreads();
    if (tid < ROWS / 4) {
        float4 t = red[MAP::slot(tid, 0)];
#pragma unroll
        for (int j = 1; j < MAP::PARTS; ++j) { const float4 o = red[MAP::slot(tid, j)]; t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w; }
        float* dst = (g.cs_slab ? g.cs_slab + (size_t)z * g.M : g.colsum) + m0 + 4 * tid;
        const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!EDGE || m0 + 4 * tid + j < g.M) dst[j] = tv[j];
    }
}

// RLT_GEMM_ACCUMULATE in gemm6e: C = relu?(fl(fl(acc + bias) + C)), the value the element-wise loop of write_output_simple gives.
// Written as `v += base[loff]; base[loff] = v;` per element, the read of element r + 1 cannot be moved above the store of element r
// (C may be any pointer and ldo is a run-time value), so the wavefront paid one full memory latency per accumulator register: 256
// dependent load - wait - add - store round trips per tile, with no partner wavefront on the SIMD to run meanwhile.  Here the reads
// are ordered by hand: the 16 C values of a 32 x 32 block are loaded together, and the next block's 16 are issued BEFORE this
// block's stores, so one latency is exposed per call and the rest overlap the stores.  Every element is still read exactly once,
// before its own store and by the lane that stores it, so C may be the buffer an earlier GEMM wrote (in place) - no aliasing promise
// is made to the compiler.  (gemm6c keeps the element-wise form of write_output_t: its persistent form has no free registers -
// batched there, the reads spilled - and its second wavefront per SIMD covers the round trips; profiles/accum_epilogue_notes.md)
template <int NJ>
__device__ __forceinline__ void accumulate_blocks(const GemmArgs& g, const f32x16 (&acc)[2][NJ], float* out, int ldo, int rb, int cb,
                                                  int loff, int l31, bool relu) {
    float bv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        bv[j] = 0.f;
        if (g.bias) bv[j] += g.bias[cb + j * 32 + l31];
        if (g.bias2) bv[j] += g.bias2[cb + j * 32 + l31];
    }
    auto row = [&](int b, int r) {          // scalar base of accumulator register r of block b = 2 j + i
        return out + (size_t)(rb + (b & 1) * 32 + (r & 3) + 8 * (r >> 2)) * ldo + (cb + (b >> 1) * 32);
    };
    float c[2][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) c[0][r] = row(0, r)[loff];
#pragma unroll
    for (int b = 0; b < 2 * NJ; ++b) {
        if (b + 1 < 2 * NJ) {
#pragma unroll
            for (int r = 0; r < 16; ++r) c[(b + 1) & 1][r] = row(b + 1, r)[loff];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[b & 1][b >> 1][r] + bv[b >> 1];
            v += c[b & 1][r];
            if (relu) v = fmaxf(v, 0.f);
            row(b, r)[loff] = v;
        }
    }
}

// epilogue of gemm6e for the plain / bias / bias + ReLU / accumulate / split-K-slab outputs (the host sends every other epilogue
// - 1-bit masks, float masks, dropout - to gemm6c): one loop nest, the accumulator registers read where they are stored
template <int NJ>
__device__ __forceinline__ void write_output_simple(const GemmArgs& g, const f32x16 (&acc)[2][NJ], int rbase, int cbase, int l31, int hh, int z) {
    const bool to_slab = g.slab != nullptr;
    float* out = to_slab ? g.slab + (size_t)z * g.M * g.N : g.C;
    const int ldo = to_slab ? g.N : g.ldc;
    const int rb = __builtin_amdgcn_readfirstlane(rbase), cb = __builtin_amdgcn_readfirstlane(cbase);
    const int loff = 4 * hh * ldo + l31;
    const bool relu = !to_slab && (g.flags & RLT_GEMM_RELU), accum = !to_slab && (g.flags & RLT_GEMM_ACCUMULATE);
    if (accum) { accumulate_blocks<NJ>(g, acc, out, ldo, rb, cb, loff, l31, relu); return; }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = cb + j * 32 + l31;
        float bv = 0.f;
        if (!to_slab) {
            if (g.bias) bv += g.bias[col];
            if (g.bias2) bv += g.bias2[col];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                float* base = out + (size_t)(rb + i * 32 + dr) * ldo + (cb + j * 32);       // scalar
                float v = acc[i][j][r] + bv;
                if (relu) v = fmaxf(v, 0.f);
                base[loff] = v;
            }
        }
    }
}
// (ta, tb) as compile-time tags
template <typename F>
int with_layout(bool ta, bool tb, F f) {
    if (ta) return tb ? f(BoolTag<true>{}, BoolTag<true>{}) : f(BoolTag<true>{}, BoolTag<false>{});
    return tb ? f(BoolTag<false>{}, BoolTag<true>{}) : f(BoolTag<false>{}, BoolTag<false>{});
}

// every tiled product kernel: grid, workgroup size and LDS bytes are the plan's; p.d goes to *rec right before the launch
template <typename Kern>
int launch(Kern kern, const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st) {
    const int rc = rlt_allow_lds(kern, p.lds_bytes);
    if (rc) return rc;
    *rec = p.d;
    hipLaunchKernelGGL(kern, dim3(p.grid_x, 1, p.grid_z), dim3(p.wg), p.lds_bytes, st, g);
    return RLT_LAUNCH_RESULT();
}

// gemm_plan.h's row of a family against the kernel's own constants (asserted in the file that owns them)
constexpr bool family_is(int family, int bm, int bn, size_t lds) {
    return GEMM_FAMILY[family].bm == bm && GEMM_FAMILY[family].bn == bn && GEMM_FAMILY[family].lds == lds;
}

}  // namespace

// One launcher per family file, called by gemm_run (gemm.hip) with the plan: picks the instantiation p.d names (layout, fast
// loaders, persistent form) and launches it through launch().  0 or a hip error code.
extern "C" {
int rlt_gemm_f32_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st);    // gemm_kernel
int rlt_gemm3_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st);       // gemm3_kernel, gemm3b_kernel
int rlt_gemm6_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st);       // gemm6_kernel, gemm6b_kernel
int rlt_gemm6c_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st);
int rlt_gemm6e_launch(const GemmPlan& p, const GemmArgs& g, rlt_gemm_dispatch* rec, hipStream_t st);
}
