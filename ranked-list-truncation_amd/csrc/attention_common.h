// Shared by the six kernel families of the list-axis attention (attention.hip, attention16.hip, attention3.hip, attention6.hip,
// attention6n.hip, attention6h.hip) and their dispatch (attention_dispatch.hip): the kernels' argument block, the device helpers
// they have in common, and the family launchers' declarations.
#pragma once
#include "common.h"

struct AttnArgs {
    const float* qkv; const float* out; const float* dout; const float* lse; const float* delta;
    const void* img; const void* dimg;        // bf16x6 mode: pre-split tile images the kernel stages from (which ones: the launchers below)
    float* o; float* lse_o; float* dqkv;
    int S, B, H;
    float scale;
    float drop_p; uint32_t drop_thr, seed;    // dropout on the attention probabilities (train mode)
    uint32_t* redo;                           // pipelined forward kernels and their fix-up launch: one flag word per workgroup, else null
};

// One LDS-DMA piece as inline assembly: M0 carries the LDS destination.  hipcc treats M0 as a reserved register (a
// clobber on it is rejected with a warning and ignored), so the statement saves and restores it: whatever the compiler
// keeps in M0 around the asm (its own global_load_lds builtins in a mixed instantiation, movrel / readlane lowerings)
// survives.  Two scalar moves per piece, ~5 pieces per wavefront and tile.
#define RLT_DMA_ASM(dst, src)                                                                                         \
    do {                                                                                                              \
        uint32_t m0_keep_;                                                                                            \
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0" \
                     : "=&s"(m0_keep_) : "s"(dst), "v"(src) : "memory");                                              \
    } while (0)

namespace {

constexpr int KT = 64;      // rows per LDS tile
constexpr int QT = 128;     // rows owned by a workgroup (4 wavefronts x 32)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;


// per-(position, head) stream of the dropout RNG; keep(pair_seed, query, key)
__device__ __forceinline__ uint32_t pair_seed(uint32_t seed, int pair) { return rlt_mix32(seed ^ ((uint32_t)pair * 0x9E3779B9U)); }

// flat block id -> (position*head pair, row tile); all row tiles of a pair go to one XCD (they
// share that pair's K/V in the XCD's L2) when the pair count allows.
__device__ __forceinline__ void map_block(int bid, int npair, int ntile, int& pair, int& tile) {
    if ((npair & 7) == 0) {
        const int xcd = bid & 7, j = bid >> 3;
        pair = (j / ntile) * 8 + xcd;
        tile = j % ntile;
    } else {
        pair = bid / ntile;
        tile = bid % ntile;
    }
}

// store D^T accumulators (row = d, col = lane's row index) to global rows: dst + row*ld + d
template <int HD>
__device__ __forceinline__ void store_acc_T(float* __restrict__ dst_row, int hh, const f32x16 (&acc)[(HD + 31) / 32],
                                            float mul) {
    constexpr int DT = (HD + 31) / 32;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = dt * 32 + 8 * g + 4 * hh;
            if (d0 < HD) {
                float4 v;
                v.x = acc[dt][4 * g + 0] * mul; v.y = acc[dt][4 * g + 1] * mul;
                v.z = acc[dt][4 * g + 2] * mul; v.w = acc[dt][4 * g + 3] * mul;
                *reinterpret_cast<float4*>(dst_row + d0) = v;
            }
        }
}


}  // namespace

// ---- family launchers.  Each is HANDED its kernel (an RLT_ATTN_* code of the call's plan, attention_plan.h) and the part it runs
// (which = 0 forward, 1 dK+dV, 2 dQ); it owns the LDS bytes, the grid, rlt_allow_lds and the DROP template switch (a.drop_p > 0),
// nothing else.  A kernel whose preconditions do not hold (no images, a list count off the tile, a family's other code ...) is
// RLT_E_ARG: no launcher launches something else instead.  The prepare passes write the tile images the plan names.
// exact fp32 on the 32x32x2 MFMA (attention.hip): RLT_ATTN_F32 / _F32_SB / _F32_OCC1; delta = rowsum(dout * out) for every family
int rlt_attn_f32_run(int kernel, int which, const AttnArgs& a, int HD, hipStream_t st);
int rlt_attn_delta_run(const float* out, const float* dout, int S, int B, int H, int HD, float* delta, hipStream_t st);
// exact fp32 at head dim 16 on the 16x16x4 MFMA (attention16.hip): RLT_ATTN_F32_HD16
int rlt_attn16_run(int which, const AttnArgs& a, hipStream_t st);
// bf16x3 (attention3.hip): RLT_ATTN_X3.  which = 0 writes the Q / K / V records into `images` first; which = 3 is the backward
// prepare (the dO records into `dimages`, delta into a.delta from a.o)
size_t rlt_attn3_images_bytes(int S, int B, int H, int HD, int nmat);
int rlt_attn3_run(int which, const AttnArgs& a, int HD, void* images, void* dimages, hipStream_t st);
// bf16x6 on the 32x32x16 MFMA, head dims 16 / 32 / 64 (attention6.hip): RLT_ATTN_X6, _X6_PP, _X6_DKV1, _X6_DQ1 and the _IMG forms,
// which stage pre-split tile images - Q | K | V in a.img (prepare: dO = false, from a.qkv), dO in a.dimg (dO = true, from a.dout);
// nmat matrices of S*H pairs x ceil(B / 64) tiles.  With a.redo set the ping-pong forward is the fix-up launch behind attention6h.hip
size_t rlt_attn6_images_bytes(int S, int B, int H, int HD, int nmat);
int rlt_attn6_prepare(bool dO, const AttnArgs& a, int HD, hipStream_t st);
int rlt_attn6_run(int kernel, int which, const AttnArgs& a, int HD, hipStream_t st);
// bf16x6 at head dim 16 on the 16x16x32 MFMA (attention6n.hip): RLT_ATTN_X6N_2W, _X6N_2W_SEEDED (with a.redo set: the fix-up launch
// behind the pipelined forward) and _X6N_PIPE.  The pipelined forward stages K / V images from a two-block buffer (prepare_at:
// matrix `what` into block `slot` of a.img) and leaves a flag word per workgroup in a.redo; the pipelined backward kernels stage
// Q / K / V / dO images + row seeds from a.img: rlt_attn6n_images_bytes bytes, written by rlt_attn6n_prepare (what = 0 Q, 1 K,
// 2 V, 3 dO, 4 seeds)
size_t rlt_attn6n_fwd_images_bytes(int S, int B, int H);
size_t rlt_attn6n_images_bytes(int S, int B, int H);
int rlt_attn6n_prepare_at(int what, int slot, const AttnArgs& a, hipStream_t st);
int rlt_attn6n_prepare(int what, const AttnArgs& a, hipStream_t st);
int rlt_attn6n_run(int kernel, int which, const AttnArgs& a, hipStream_t st);
// bf16x6 at head dim 64, pipelined forward (attention6h.hip): RLT_ATTN_X6H_PIPE.  K / V images in blocks 0 / 1 of a.img (written by
// rlt_attn6h_prepare2), a flag word per workgroup in a.redo for the fix-up launch
size_t rlt_attn6h_fwd_images_bytes(int S, int B, int H);
int rlt_attn6h_prepare2(int what0, int slot0, int what1, int slot1, const AttnArgs& a, hipStream_t st);
int rlt_attn6h_run(int which, const AttnArgs& a, hipStream_t st);
