// Element and batch terms of the multi-task losses, shared by rlt_mt_terms (loss.hip) and rlt_probe_heads (probe.hip) so
// both paths compute nn.BCELoss and RerankLoss with the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

// torch binary_cross_entropy of one element (class probability c, label t): logs clamped at -100
__device__ __forceinline__ float rlt_bce_term(float c, float t) {
    const float l1 = fmaxf(logf(c), -100.f);
    const float l0 = fmaxf(log1pf(-c), -100.f);
    return (t - 1.f) * l0 - t * l1;
}

// torch binary_cross_entropy_backward of one element before the reduction's scale: (c - t) / max((1-c)c, 1e-12)
__device__ __forceinline__ float rlt_bce_dgrad(float c, float t) {
    return (c - t) / fmaxf((1.f - c) * c, 1e-12f);
}

// utils/losses.py:136-141 (RerankLoss) from the batch sums: the sum of the scores and the count of the y == 1 entries
// (s_pos, n_pos) and of the y == 0 entries (s_neg, n_neg).  hinge = max(0, mean_neg - mean_pos + margin), 0 when a class
// is empty or the argument is <= 0 (Python's max(0, x) returns the 0); gpos / gneg = d hinge / d s of a y == 1 / y == 0
// entry (-1/n_pos, +1/n_neg while the hinge is active, else 0).
__device__ __forceinline__ void rlt_rerank_hinge(double s_pos, double n_pos, double s_neg, double n_neg, float margin,
                                                 float& hinge, float& gpos, float& gneg) {
    hinge = 0.f; gpos = 0.f; gneg = 0.f;
    if (n_pos > 0 && n_neg > 0) {
        const float gap = (float)(s_neg / n_neg) - (float)(s_pos / n_pos) + margin;
        if (gap > 0.f) { hinge = gap; gpos = (float)(-1.0 / n_pos); gneg = (float)(1.0 / n_neg); }
    }
}
