// The segment table of a flat bucket (include/rlt_hip.h, rlt_grad_norm): n_seg + 1 ascending int64 offsets, multiples of 4, from
// 0 to n.  Shared by the gradient-norm pass (optim.hip) and the recipe step (recipe.hip).
#pragma once
#include "common.h"

// largest s in [0, n_seg) with off[s] <= pos (0 when there is none): the segment that holds element pos of an ascending table
__device__ __forceinline__ int seg_of(const long long* __restrict__ off, int n_seg, long long pos) {
    int lo = 0, hi = n_seg;                       // invariant: the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

// A segment table the HOST can read (pinned or managed memory, or a process without a device) is checked before the launch; one
// in device memory cannot be read without a synchronising copy and is the caller's duty (the kernels stay in bounds with any
// table).  1: host-readable.
static inline bool host_readable(const void* ptr) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();                  // not known to the runtime, or no device: plain host memory
        return true;
    }
    return a.type != hipMemoryTypeDevice;
}

static inline bool seg_table_ok(const int64_t* off, int n_seg, size_t n) {
    if (off[0] != 0 || off[n_seg] != (int64_t)n) return false;
    for (int s = 0; s < n_seg; ++s)
        if (off[s + 1] < off[s] || off[s] % 4 != 0) return false;
    return true;
}
