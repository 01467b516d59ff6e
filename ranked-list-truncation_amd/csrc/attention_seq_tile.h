// The per-tile device functions and the limits of the within-list attention kernels: attention_seq.hip (the one-shot forward and
// backward) and attention_seq_append.hip (the K/V-cached append forward) are written from these, so that a query row of the
// append kernel goes through the same instructions in the same order as the row of the one-shot causal forward - the bit-for-bit
// contract between the two (tests/test_seq_append_gpu.py) rests on this one definition.
#pragma once
#include "attention_common.h"

namespace {

constexpr int SQ_TR = 64;            // rows per LDS tile
constexpr int SQ_LD = 68;            // floats per LDS tile row (64 columns + 4: 16-byte rows, row reads spread over the banks)
constexpr int SQ_MAX_S = 1024;

// rows row0 .. row0+63 of list b, columns c0 .. c0+cw-1 (cw a multiple of 16) of a position-major matrix with `ld` floats per
// row -> tile[64][SQ_LD]; rows >= S and columns >= cw are written as zeros.  256 threads, 16 lanes per 256-byte row.
__device__ __forceinline__ void sq_stage(float* __restrict__ tile, const float* __restrict__ src, size_t ld, int B, int b,
                                         int row0, int S, int c0, int cw, int tid) {
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, c4 = (idx & 15) * 4, row = row0 + r;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < S && c4 < cw) v[i] = *reinterpret_cast<const float4*>(src + ((size_t)row * B + b) * ld + c0 + c4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, c4 = (idx & 15) * 4;
        *reinterpret_cast<float4*>(tile + r * SQ_LD + c4) = v[i];
    }
}

// N floats of a global row (16-byte aligned) into registers
template <int N>
__device__ __forceinline__ void sq_load_row(float (&dst)[N], const float* __restrict__ p) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * i);
        dst[4 * i] = v.x; dst[4 * i + 1] = v.y; dst[4 * i + 2] = v.z; dst[4 * i + 3] = v.w;
    }
}

// D[i = tile row][j = owned row] += sum_d tile[i][d] * reg[j][d]: `trow` = this lane's tile row at the first column of its
// half of the head, reg = the owned row's same half
template <int KH>
__device__ __forceinline__ f32x16 sq_rows_dot(const float* __restrict__ trow, const float (&reg)[KH]) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t4 = 0; t4 < KH / 4; ++t4) {
        const float4 a = *reinterpret_cast<const float4*>(trow + 4 * t4);
        s = mfma32(a.x, reg[4 * t4 + 0], s);
        s = mfma32(a.y, reg[4 * t4 + 1], s);
        s = mfma32(a.z, reg[4 * t4 + 2], s);
        s = mfma32(a.w, reg[4 * t4 + 3], s);
    }
    return s;
}

// acc[dt][i = head column][j = owned row] += sum over the 32 tile rows of tile[row][column] * w[row][j], w in accumulator layout;
// `tcol` = the sub-tile's first row at this lane's head column
template <int DT>
__device__ __forceinline__ void sq_cols_acc(f32x16 (&acc)[DT], const float* __restrict__ tcol, int hh, const f32x16& w) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int t = 0; t < 16; ++t)
            acc[dt] = mfma32(tcol[acc_row(t, hh) * SQ_LD + 32 * dt], w[t], acc[dt]);
}

// the lane's owned row of a transposed accumulator -> global: dst = the row's first column of the head
template <int HD>
__device__ __forceinline__ void sq_store_T(float* __restrict__ dst, int hh, const f32x16 (&acc)[(HD + 31) / 32], float mul) {
    store_acc_T<HD>(dst, hh, acc, mul);
}

// the last key tile a pass of queries [.., qend) needs under the causal mask ends at its last query
__device__ __forceinline__ int sq_key_end(int S, int qend) { return qend < S ? qend : S; }

// the causal mask: key `key` is admitted for query `q` iff it lies inside the list and not behind the query
__device__ __forceinline__ bool sq_admit(int key, int q, int S) { return key < S && key <= q; }

template <int HD>
struct SeqGeom {
    static constexpr int HPG = 64 / HD;           // heads per workgroup
    static constexpr int OWN = 32 * (4 / HPG);    // rows the workgroup owns per pass (128: four wavefronts of one head; 32)
    static constexpr int DT = (HD + 31) / 32;
    static constexpr int KH = HD / 2;             // columns of a head per lane half
};

// RLT_E_ARG, then RLT_E_SHAPE; the pointers are the caller's to check
inline int seq_check_dims(int S, int B, int H, int HD, float drop_p) {
    RLT_CHECK_ARG(S > 0 && B > 0 && H > 0);
    RLT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f);
    RLT_CHECK_SHAPE(HD == 16 || HD == 64);
    RLT_CHECK_SHAPE(S <= SQ_MAX_S);
    // element offsets are 64-bit in the kernels; refuse what no buffer can hold (2^40 floats) before any product can wrap, and a
    // grid beyond what one launch dimension takes (2^32 - 1 threads: 2^24 - 1 workgroups of 256)
    const long long lim = 1LL << 40;
    const long long row = 3LL * H * HD;                       // < 2^40
    RLT_CHECK_SHAPE(row < lim && (long long)S * B < lim / row);
    const long long ngrp = ((long long)H + 64 / HD - 1) / (64 / HD);
    RLT_CHECK_SHAPE((long long)B * ngrp < (1LL << 24));
    return 0;
}

}  // namespace
