// Sparse input projection of BiLSTM layer 0 and its weight gradient: BiCut on its bag-of-words document input
// (models/Bicut.py:6,10 of the reference, input_size = 231449; data_prep/document_statics.ipynb "Bicut输入数据";
// dataloader/split_bicut_data.py:21-24; dataloader/bicut_dataloader.py).  The reference densifies every ranked document to
// a row of 3 + 231,448 numbers; here a token row is `Dn` dense columns plus one CSR row of a device-resident table, and the
// two layer-0 input weights are kept column-major - (I, 512) per direction, I = Dn + V - so that one nonzero reads, and one
// gradient column writes, 2 KB contiguous per direction.
//
//   forward   one workgroup per token row: 256 lanes x 4 floats = the 2 x 512 gate columns; bias, the dense columns, then the
//             row's nonzeros in table order, one fp32 fma chain per gate.
//   backward  per destination column (= term), from the table's static term -> rows index (CSC, built once by the host) and
//             the batch's occurrence lists (token rows sorted by table row: `perm`; `occ[d]` = first position of row d in it,
//             found here by binary search): a column's entries are cut into chunks of SPARSE_CH, one workgroup per chunk;
//             chunk 0 writes the gradient column (=), later chunks write partial sums that a finishing launch adds in chunk
//             order.  The dense columns and the bias gradient: partial sums over blocks of 32 token rows, then the fixed-order
//             column reduction of common.h.  No float atomics anywhere: bitwise reproducible.
// A table row outside [0, n_docs), a term outside [0, V) or a `perm` entry outside [0, S*B) is never dereferenced: it
// contributes nothing.
#include "common.h"

namespace {

constexpr int SPARSE_CH = RLT_SPARSE_CHUNK;      // entries per chunk = lanes per workgroup (in the header: the host builds the chunk table)
static_assert(SPARSE_CH == 256, "one entry per lane of a 256-lane workgroup");
constexpr int DENSE_ROWS = 32;        // token rows per partial sum of the dense-column / bias gradient
constexpr int MAX_DN = 16;
constexpr size_t WS_ALIGN = 256;
inline size_t rup(size_t b) { return (b + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

__device__ __forceinline__ f32x4 fma4(float a, f32x4 x, f32x4 acc) {
    acc.x = fmaf(a, x.x, acc.x); acc.y = fmaf(a, x.y, acc.y); acc.z = fmaf(a, x.z, acc.z); acc.w = fmaf(a, x.w, acc.w);
    return acc;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void sparse_inproj_fwd_kernel(
    const float* __restrict__ dense, int Dn, const int32_t* __restrict__ ids, int S, int B, int n_docs, int V,
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const float* __restrict__ values,
    const float* __restrict__ wt0, const float* __restrict__ wt1,
    const float* __restrict__ bi0, const float* __restrict__ bh0, const float* __restrict__ bi1, const float* __restrict__ bh1,
    float* __restrict__ gates) {
    const int t = blockIdx.x;                 // token row s*B + b
    const int s = t / B, b = t - s * B;
    const size_t src = (size_t)b * S + s;     // the same position in the (B,S) user layout
    const int dir = threadIdx.x >> 7, g = (threadIdx.x & 127) * 4;
    const float* __restrict__ w = (dir ? wt1 : wt0) + g;
    f32x4 acc = ld4((dir ? bi1 : bi0) + g) + ld4((dir ? bh1 : bh0) + g);
    for (int c = 0; c < Dn; ++c) acc = fma4(dense[src * Dn + c], ld4(w + (size_t)c * 512), acc);
    const int d = ids[src];
    if ((unsigned)d < (unsigned)n_docs) {
        const int64_t j1 = indptr[d + 1];
        int64_t j = indptr[d];
        w += (size_t)Dn * 512;
        for (; j + 8 <= j1; j += 8) {          // eight 2 KB rows in flight, added in table order
            f32x4 x[8]; float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int term = indices[j + u];
                const bool ok = (unsigned)term < (unsigned)V;
                v[u] = ok ? values[j + u] : 0.f;
                x[u] = ld4(w + (size_t)(ok ? term : 0) * 512);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fma4(v[u], x[u], acc);
        }
        for (; j < j1; ++j) {
            const int term = indices[j];
            if ((unsigned)term < (unsigned)V) acc = fma4(values[j], ld4(w + (size_t)term * 512), acc);
        }
    }
    st4(gates + (size_t)t * 1024 + threadIdx.x * 4, acc);
}

// ------------------------------------------------------------------------------------------------ backward
// occ[d] = number of entries of perm whose table row is < d, d in [0, n_docs]: rows below 0 sort first, rows >= n_docs last
__global__ __launch_bounds__(256) void sparse_occ_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ perm,
                                                         int S, int B, int n_docs, int32_t* __restrict__ occ) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d > n_docs) return;
    const int T = S * B;
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int t = perm[mid];
        int row = n_docs;                                   // a perm entry outside [0, T) ranks with the rows that are skipped
        if ((unsigned)t < (unsigned)T) { const int s = t / B, b = t - s * B; row = ids[(size_t)b * S + s]; }
        if (row < d) lo = mid + 1; else hi = mid;
    }
    occ[d] = lo;
}

// dense columns and bias: partial[blk][dir][c][512], c = Dn is the bias row
__global__ __launch_bounds__(256) void sparse_dense_dw_kernel(const float* __restrict__ dense, int Dn, int S, int B,
                                                              const float* __restrict__ dg, float* __restrict__ partial) {
    const int T = S * B;
    const int t0 = blockIdx.x * DENSE_ROWS, t1 = t0 + DENSE_ROWS < T ? t0 + DENSE_ROWS : T;
    f32x4 acc[MAX_DN + 1];
#pragma unroll
    for (int c = 0; c <= MAX_DN; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = t0; t < t1; ++t) {
        const int s = t / B, b = t - s * B;
        const float* __restrict__ xr = dense + ((size_t)b * S + s) * Dn;
        const f32x4 x = ld4(dg + (size_t)t * 1024 + threadIdx.x * 4);
        acc[MAX_DN] += x;
#pragma unroll
        for (int c = 0; c < MAX_DN; ++c)
            if (c < Dn) acc[c] = fma4(xr[c], x, acc[c]);
    }
    const int dir = threadIdx.x >> 7, g = (threadIdx.x & 127) * 4;
    float* __restrict__ p = partial + ((size_t)blockIdx.x * 2 + dir) * (Dn + 1) * 512 + g;
#pragma unroll
    for (int c = 0; c < MAX_DN; ++c)
        if (c < Dn) st4(p + (size_t)c * 512, acc[c]);
    st4(p + (size_t)Dn * 512, acc[MAX_DN]);
}

__global__ __launch_bounds__(256) void sparse_term_dw_kernel(
    const int32_t* __restrict__ perm, int T, int n_docs, int Dn, int V, int n_extra,
    const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ col_rows, const float* __restrict__ col_vals,
    const int32_t* __restrict__ chunk_col, const int32_t* __restrict__ chunk_ptr,
    const int32_t* __restrict__ occ, const float* __restrict__ dg,
    float* __restrict__ dwt0, float* __restrict__ dwt1, float* __restrict__ extra) {
    __shared__ int h_start[SPARSE_CH], h_n[SPARSE_CH], h_t0[SPARSE_CH];
    __shared__ float h_val[SPARSE_CH];
    __shared__ int w_cnt[4];
    const int c = blockIdx.x, v = chunk_col[c];
    if ((unsigned)v >= (unsigned)V) return;                  // (a chunk table that does not belong to this table: nothing is written)
    const int ci = c - chunk_ptr[v];
    if (ci < 0 || (ci > 0 && (unsigned)(c - v - 1) >= (unsigned)n_extra)) return;
    const int64_t e0 = col_ptr[v] + (int64_t)ci * SPARSE_CH;
    const int64_t left = col_ptr[v + 1] - e0;
    const int len = left < SPARSE_CH ? (left > 0 ? (int)left : 0) : SPARSE_CH;
    // every lane looks one entry up, then the entries that occur in this batch are compacted in entry order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int st = 0, n = 0, t0 = 0; float val = 0.f;
    if ((int)threadIdx.x < len) {
        const int d = col_rows[e0 + threadIdx.x];
        if ((unsigned)d < (unsigned)n_docs) {
            st = occ[d];
            n = occ[d + 1] - st;
            if (n > 0) { val = col_vals[e0 + threadIdx.x]; t0 = perm[st]; }
        }
    }
    const unsigned long long m = __ballot(n > 0);
    if (lane == 0) w_cnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0, nh = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (k < wv) base += w_cnt[k]; nh += w_cnt[k]; }
    if (n > 0) {
        const int r = base + __popcll(m & ((1ull << lane) - 1ull));
        h_start[r] = st; h_n[r] = n; h_t0[r] = t0; h_val[r] = val;
    }
    __syncthreads();
    const float* __restrict__ src = dg + threadIdx.x * 4;
    f32x4 acc{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < nh; i += 4) {            // four 4 KB gradient rows in flight, added in entry order
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = i + u < nh ? h_t0[i + u] : -1;
            x[u] = (unsigned)t < (unsigned)T ? ld4(src + (size_t)t * 1024) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i + u >= nh) break;
            const float a = h_val[i + u];
            acc = fma4(a, x[u], acc);
            const int cnt = h_n[i + u], s0 = h_start[i + u];
            for (int k = 1; k < cnt; ++k) {       // the same document at further token rows
                const int t = perm[s0 + k];
                if ((unsigned)t < (unsigned)T) acc = fma4(a, ld4(src + (size_t)t * 1024), acc);
            }
        }
    }
    const int dir = threadIdx.x >> 7, g = (threadIdx.x & 127) * 4;
    if (ci == 0) st4((dir ? dwt1 : dwt0) + ((size_t)Dn + v) * 512 + g, acc);
    else st4(extra + (size_t)(c - v - 1) * 1024 + threadIdx.x * 4, acc);
}

// columns of more than one chunk: column = ((chunk 0 + chunk 1) + chunk 2) + ...
__global__ __launch_bounds__(256) void sparse_term_finish_kernel(const int32_t* __restrict__ multi_cols,
                                                                 const int32_t* __restrict__ chunk_ptr, int Dn, int V, int n_extra,
                                                                 const float* __restrict__ extra,
                                                                 float* __restrict__ dwt0, float* __restrict__ dwt1) {
    const int v = multi_cols[blockIdx.x];
    if ((unsigned)v >= (unsigned)V) return;
    const int c0 = chunk_ptr[v], k = chunk_ptr[v + 1] - c0;
    if (k <= 1 || c0 < v || (long long)c0 - v + k - 1 > n_extra) return;
    const int dir = threadIdx.x >> 7, g = (threadIdx.x & 127) * 4;
    float* dst = (dir ? dwt1 : dwt0) + ((size_t)Dn + v) * 512 + g;
    f32x4 acc = ld4(dst);
    const float* __restrict__ p = extra + (size_t)(c0 - v) * 1024 + threadIdx.x * 4;
    for (int i = 1; i < k; ++i) acc += ld4(p + (size_t)(i - 1) * 1024);
    st4(dst, acc);
}

struct BwdWs { int32_t* occ; float *partial, *extra; int blocks; size_t bytes; };
inline BwdWs bwd_ws(int S, int B, int Dn, int n_docs, int V, int n_chunks, void* base) {
    BwdWs w{};
    uint8_t* p = (uint8_t*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += rup(bytes); return r; };
    w.blocks = rlt_cdiv((long long)S * B, DENSE_ROWS);
    w.occ = (int32_t*)take(((size_t)n_docs + 1) * sizeof(int32_t));
    w.partial = (float*)take((size_t)w.blocks * 2 * (Dn + 1) * 512 * sizeof(float));
    w.extra = (float*)take((size_t)(n_chunks - V) * 1024 * sizeof(float));
    w.bytes = off;
    return w;
}

inline int batch_ok(const rlt_sparse_batch* sb, int S, int B, bool bwd) {
    RLT_CHECK_ARG(sb && S > 0 && B > 0);
    RLT_CHECK_ARG(sb->dense && sb->ids && sb->indptr && sb->indices && sb->values && sb->n_docs > 0 && sb->V > 0 && sb->Dn > 0);
    RLT_CHECK_SHAPE(sb->Dn <= MAX_DN);
    RLT_CHECK_SHAPE((long long)S * B < (1ll << 31));
    RLT_CHECK_SHAPE((long long)sb->Dn + sb->V < (1ll << 31));
    if ((((uintptr_t)sb->dense | (uintptr_t)sb->ids | (uintptr_t)sb->indices | (uintptr_t)sb->values) & 3u) != 0) return RLT_E_ALIGN;
    if (((uintptr_t)sb->indptr & 7u) != 0) return RLT_E_ALIGN;
    if (bwd) {
        RLT_CHECK_ARG(sb->perm && sb->col_ptr && sb->col_rows && sb->col_vals && sb->chunk_col && sb->chunk_ptr);
        RLT_CHECK_ARG(sb->n_chunks >= sb->V && sb->n_multi >= 0 && sb->n_multi <= sb->V && (sb->n_multi == 0 || sb->multi_cols));
        RLT_CHECK_ARG((sb->n_chunks > sb->V) == (sb->n_multi > 0));
        if ((((uintptr_t)sb->perm | (uintptr_t)sb->col_rows | (uintptr_t)sb->col_vals | (uintptr_t)sb->chunk_col |
              (uintptr_t)sb->chunk_ptr | (uintptr_t)sb->multi_cols) & 3u) != 0) return RLT_E_ALIGN;
        if (((uintptr_t)sb->col_ptr & 7u) != 0) return RLT_E_ALIGN;
    }
    return 0;
}

}  // namespace

extern "C" {

size_t rlt_sparse_inproj_workspace(int S, int B, int Dn, int n_docs, int V, int n_chunks) {
    if (S <= 0 || B <= 0 || Dn <= 0 || Dn > MAX_DN || n_docs <= 0 || V <= 0 || n_chunks < V || (long long)S * B >= (1ll << 31)) return 0;
    return bwd_ws(S, B, Dn, n_docs, V, n_chunks, nullptr).bytes;
}

int rlt_sparse_inproj_fwd(const rlt_sparse_batch* sb, int S, int B, const float* wt_fwd, const float* wt_rev,
                          const float* b_ih_fwd, const float* b_hh_fwd, const float* b_ih_rev, const float* b_hh_rev,
                          float* gates, void* stream) {
    int rc = batch_ok(sb, S, B, false);
    if (rc) return rc;
    RLT_CHECK_ARG(wt_fwd && wt_rev && b_ih_fwd && b_hh_fwd && b_ih_rev && b_hh_rev && gates);
    if (!rlt_aligned16(wt_fwd) || !rlt_aligned16(wt_rev) || !rlt_aligned16(b_ih_fwd) || !rlt_aligned16(b_hh_fwd) ||
        !rlt_aligned16(b_ih_rev) || !rlt_aligned16(b_hh_rev) || !rlt_aligned16(gates)) return RLT_E_ALIGN;
    hipLaunchKernelGGL(sparse_inproj_fwd_kernel, dim3((unsigned)(S * B)), dim3(256), 0, rlt_stream(stream), sb->dense, sb->Dn,
                       sb->ids, S, B, sb->n_docs, sb->V, sb->indptr, sb->indices, sb->values, wt_fwd, wt_rev,
                       b_ih_fwd, b_hh_fwd, b_ih_rev, b_hh_rev, gates);
    return RLT_LAUNCH_RESULT();
}

int rlt_sparse_inproj_bwd(const rlt_sparse_batch* sb, int S, int B, const float* dgates, float* dwt_fwd, float* dwt_rev,
                          float* db_ih_fwd, float* db_hh_fwd, float* db_ih_rev, float* db_hh_rev,
                          void* ws, size_t ws_bytes, void* stream) {
    int rc = batch_ok(sb, S, B, true);
    if (rc) return rc;
    RLT_CHECK_ARG(dgates && dwt_fwd && dwt_rev && db_ih_fwd && db_hh_fwd && db_ih_rev && db_hh_rev && ws);
    if (!rlt_aligned16(dgates) || !rlt_aligned16(dwt_fwd) || !rlt_aligned16(dwt_rev) || !rlt_aligned16(ws)) return RLT_E_ALIGN;
    if ((((uintptr_t)db_ih_fwd | (uintptr_t)db_hh_fwd | (uintptr_t)db_ih_rev | (uintptr_t)db_hh_rev) & 3u) != 0) return RLT_E_ALIGN;
    const int Dn = sb->Dn, T = S * B;
    if (ws_bytes < bwd_ws(S, B, Dn, sb->n_docs, sb->V, sb->n_chunks, nullptr).bytes) return RLT_E_WORKSPACE;
    const BwdWs w = bwd_ws(S, B, Dn, sb->n_docs, sb->V, sb->n_chunks, ws);
    hipStream_t st = rlt_stream(stream);
    hipLaunchKernelGGL(sparse_occ_kernel, dim3((unsigned)rlt_cdiv((long long)sb->n_docs + 1, 256)), dim3(256), 0, st,
                       sb->ids, sb->perm, S, B, sb->n_docs, w.occ);
    hipLaunchKernelGGL(sparse_dense_dw_kernel, dim3((unsigned)w.blocks), dim3(256), 0, st, sb->dense, Dn, S, B, dgates, w.partial);
    const int ncol = (Dn + 1) * 512;
    for (int dir = 0; dir < 2; ++dir)
        hipLaunchKernelGGL(rlt_rows_reduce_kernel, dim3((unsigned)rlt_cdiv(ncol, 16)), dim3(256), 0, st,
                           w.partial + (size_t)dir * ncol, w.blocks, 2 * ncol, ncol, Dn * 512,
                           dir ? dwt_rev : dwt_fwd, dir ? db_ih_rev : db_ih_fwd, 0);
    rc = (int)hipMemcpyAsync(db_hh_fwd, db_ih_fwd, 512 * sizeof(float), hipMemcpyDeviceToDevice, st);      // d b_hh = d b_ih
    if (rc) return rc;
    rc = (int)hipMemcpyAsync(db_hh_rev, db_ih_rev, 512 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sparse_term_dw_kernel, dim3((unsigned)sb->n_chunks), dim3(256), 0, st, sb->perm, T, sb->n_docs, Dn, sb->V, sb->n_chunks - sb->V,
                       sb->col_ptr, sb->col_rows, sb->col_vals, sb->chunk_col, sb->chunk_ptr, w.occ, dgates, dwt_fwd, dwt_rev, w.extra);
    if (sb->n_multi > 0)
        hipLaunchKernelGGL(sparse_term_finish_kernel, dim3((unsigned)sb->n_multi), dim3(256), 0, st, sb->multi_cols, sb->chunk_ptr,
                           Dn, sb->V, sb->n_chunks - sb->V, w.extra, dwt_fwd, dwt_rev);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
