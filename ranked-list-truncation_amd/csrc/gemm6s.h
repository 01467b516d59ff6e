// csrc/gemm6s.hip: the weights-stationary K = 256 products of the bf16x6 mode, called from gemm_run (gemm.hip) like the launchers of gemm_common.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "gemm_plan.h"

struct Gemm6sArgs {
    const float* A; const float* B; float* C;      // C[M x N] = A[M x 256] op(B) (+ bias + bias2)
    const float* bias; const float* bias2;         // (N) or null
    int M, N, K, lda, ldb, ldc;
    // the FFN mask pair of rlt_gemm_bits (include/rlt_hip.h): bit (row & 31) of word [(row >> 5) * N + col]
    uint32_t* bits_out;                            // with relu: bit = (C > 0)
    const uint32_t* bits_in;                       // C = bit ? C * mask_scale : 0
    float mask_scale;
};
// Shape / alignment conditions: the gemm6s row of gemm_plan() (csrc/gemm_plan.hip).
// Mask epilogue (bits_out): the rows past M of the last 32-row block are evaluated as relu(bias) > 0 and their bits land in the final
// mask word - no consumer reads them (rlt_gemm_bits indexes rows < M), but the word differs from the tiled kernels' (which write 0 there).
// Launches the instantiation the plan names with the plan's grid and LDS bytes and writes p.d to *rec right before the launch.  0 or a
// hip error code.
int rlt_gemm6s_launch(const Gemm6sArgs& g, const GemmPlan& p, rlt_gemm_dispatch* rec, hipStream_t st);
