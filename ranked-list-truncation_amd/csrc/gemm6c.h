// The k-step buffer of gemm6c.hip, which gemm6e.hip rotates in the same way: six planes [A_h | A_m | A_l | B_h | B_m | B_l] of
// 256 rows x 16 k.  The layout is described at gemm6c_kernel.
#pragma once
#include "gemm3.h"

namespace {

constexpr int HB6 = 256 * 16;                  // bf16 elements of one plane of a k-step buffer
constexpr int KB6 = 6 * HB6;                   // one k-step buffer (48 KB)
__device__ __forceinline__ int phys6(int r) { return (r & ~15) | ((r & 3) << 2) | ((r >> 2) & 3); }

}  // namespace
