// What gemm3.hip introduced and the six-product kernels reuse (gemm6.hip: all of it; gemm6c.hip, gemm6e.hip: BK3, BM2 / BN2): the
// K tile of 32, the staging registers of an operand tile, and gemm3b's 256-row LDS plane - row permutation, chunk swizzle and
// the loader that goes with them.  The layout is described at gemm3b_kernel.
#pragma once
#include "gemm_common.h"

namespace {

constexpr int BK3 = 32;                                  // K tile of the split-bf16 kernels
struct Stage3 { float4 v[4]; };                          // registers of one staged operand tile: 4 float4 per thread

constexpr int BM2 = 256, BN2 = 256;
constexpr int PL2 = 256 * 32;
// physical LDS row of a logical tile row: bits 0 and 2 swapped, so that logical rows 4 apart (the two rows a 16-lane
// ds_write_b64 group covers, in both staging maps below) land in different 16-dword halves of the 32 store banks
__device__ __forceinline__ int prow2(int row) { return (row & ~5) | ((row & 1) << 2) | ((row >> 2) & 1); }
// byte-16 chunk swizzle on the PHYSICAL row: makes the ds_read_b128 fragment reads conflict-free
__device__ __forceinline__ int swz2(int prow, int chunk) { return chunk ^ ((prow >> 2) & 3); }
// K-contiguous staging map: element idx -> (row, 16-byte k group); 16 consecutive lanes = 8 k groups x rows {r, r+4}
__device__ __forceinline__ int kcb_row(int idx) { return (((idx >> 3) & 1) << 2) | ((idx >> 4) & 3) | ((idx >> 6) << 3); }

template <bool KC>
__device__ __forceinline__ void load3b(const float* __restrict__ P, int ld, int mn0, int k0, int tid, Stage3& st) {
    if (KC) {           // [MN][K]: element idx of the 2048 float4 of a 256 x 32 tile -> (row, 16-byte k group)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 512 * i;
            st.v[i] = *reinterpret_cast<const float4*>(P + (size_t)(mn0 + kcb_row(idx)) * ld + k0 + 4 * (idx & 7));
        }
    } else {            // [K][MN]: thread owns a 4(k) x 4(mn) block, k block in the low lane bits
        const int kb = tid & 7, mb = tid >> 3;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            st.v[i] = *reinterpret_cast<const float4*>(P + (size_t)(k0 + 4 * kb + i) * ld + mn0 + 4 * mb);
    }
}

}  // namespace
