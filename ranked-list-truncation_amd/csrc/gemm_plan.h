// csrc/gemm_plan.hip: the one dispatch decision of the GEMM family, read by gemm_run (gemm.hip), the family launchers (gemm_common.h,
// gemm6s.h), rlt_gemm_workspace and rlt_gemm_plan.  Host only.
#pragma once
#include <stddef.h>
#include "../../include/rlt_hip.h"

// what the decision may depend on - no pointers (the fields: include/rlt_hip.h)
typedef rlt_gemm_call GemmCall;

struct GemmPlan {
    int rc;                      // 0, RLT_E_WORKSPACE, or -1 (gemm6s: mask bits out without ReLU); non-zero: nothing is launched, d stays NONE
    rlt_gemm_dispatch d;         // the record of rlt_gemm_last_dispatch: family, layout, loader form, persistent form, final split
    int tiles_m, tiles_n;        // output tiles of the family's tile size (gemm6s: row streams, column panels)
    unsigned grid_x, grid_z, wg; // the launch of the product kernel
    size_t lds_bytes;            // its dynamic LDS
    bool reduce;                 // splitk_reduce_kernel follows (d.ns > 1)
    size_t ws_bytes;             // what the split the shape WANTS needs of `ws` (rlt_gemm_workspace), given or not
};
GemmPlan gemm_plan(const GemmCall& c);

// per kernel family (RLT_GEMM_*): output tile, workgroup size, dynamic LDS bytes.  Each family's file asserts its row against the
// kernels' own constants.
struct GemmFamily { int bm, bn, wg; size_t lds; };
constexpr GemmFamily GEMM_FAMILY[] = {
    {0, 0, 0, 0},
    {128, 128, 256, 4 * 16 * 132 * 4},          // gemm_kernel: A and B, two buffers of 16 k-rows of 132 floats
    {128, 128, 256, 2 * 4 * 128 * 40 * 2},      // gemm3_kernel: two buffers of hi / lo tiles of A and B
    {256, 256, 512, 2 * 4 * 256 * 32 * 2},      // gemm3b_kernel
    {256, 128, 512, 2 * 3 * (256 + 128) * 32 * 2},   // gemm6_kernel: two buffers of three planes of A and B
    {256, 256, 512, 6 * 256 * 32 * 2},          // gemm6b_kernel: one K tile as six planes
    {256, 256, 512, 3 * 6 * 256 * 16 * 2},      // gemm6c_kernel: three k-step buffers
    {256, 256, 256, 3 * 6 * 256 * 16 * 2},      // gemm6e_kernel: the same buffers, one wavefront per SIMD
    {32, 256, 256, 0},                          // gemm6s_kernel: LDS by K, below
};
constexpr size_t GEMM6S_LDS_K256 = 160 * 1024, GEMM6S_LDS_K128 = 48 * 1024;
