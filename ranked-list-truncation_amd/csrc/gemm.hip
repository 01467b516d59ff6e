// The host side of the GEMM family: rlt_gemm / rlt_gemm_ex / rlt_gemm_bits check the call, have it planned (gemm_plan.hip) and hand
// the plan to the launcher of the family it names - one file per family: gemm_f32.hip (exact fp32 on the f32 MFMA), gemm3.hip
// (bf16x3), gemm6.hip / gemm6c.hip / gemm6e.hip / gemm6s.hip (bf16x6); what the tiled kernels share is gemm_common.h.  Here
// too: the deterministic split-K slab reduction that follows a split product (no float atomics), and the small kernels around
// the products - column sums (bias gradients), the narrow weight gradient, ReLU backward, scale.
#include "gemm_common.h"
#include "gemm6s.h"

namespace {

// C = sum_z slab[z] (+bias, relu, accumulate); fixed order => deterministic.  Four independent partial sums per
// element keep four slab loads in flight (the z loop is otherwise one dependent chain of L2/HBM latencies).
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs g, int nsplit) {
    const size_t mn = (size_t)g.M * g.N;
    const size_t stride = (size_t)gridDim.x * 256;
    if ((g.N & 3) == 0) {                     // rows hold whole float4s: a vector never straddles two rows
        const float4* slab4 = reinterpret_cast<const float4*>(g.slab);
        const size_t mn4 = mn / 4;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < mn4; i += stride) {
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
            int z = 0;
            for (; z + 3 < nsplit; z += 4) {
                a0 = f4add(a0, slab4[(size_t)z * mn4 + i]);
                a1 = f4add(a1, slab4[(size_t)(z + 1) * mn4 + i]);
                a2 = f4add(a2, slab4[(size_t)(z + 2) * mn4 + i]);
                a3 = f4add(a3, slab4[(size_t)(z + 3) * mn4 + i]);
            }
            for (; z < nsplit; ++z) a0 = f4add(a0, slab4[(size_t)z * mn4 + i]);
            const float4 v4 = f4add(f4add(a0, a1), f4add(a2, a3));
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            const int row = (int)((4 * i) / g.N), col0 = (int)(4 * i - (size_t)row * g.N);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = col0 + e;
                float bv = 0.f;
                if (g.bias) bv += g.bias[col];
                if (g.bias2) bv += g.bias2[col];
                float* dst = g.C + (size_t)row * g.ldc + col;
                *dst = gemm_epilogue(g, v[e], bv, row, col, dst);
            }
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < mn; i += stride) {
            float v = 0.f;
            for (int z = 0; z < nsplit; ++z) v += g.slab[(size_t)z * mn + i];
            const int row = (int)(i / g.N), col = (int)(i - (size_t)row * g.N);
            float bv = 0.f;
            if (g.bias) bv += g.bias[col];
            if (g.bias2) bv += g.bias2[col];
            float* dst = g.C + (size_t)row * g.ldc + col;
            *dst = gemm_epilogue(g, v, bv, row, col, dst);
        }
    }
    if (g.cs_slab)
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)g.M; i += stride) {
            float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
            int z = 0;
            for (; z + 3 < nsplit; z += 4) {
                c0 += g.cs_slab[(size_t)z * g.M + i];
                c1 += g.cs_slab[(size_t)(z + 1) * g.M + i];
                c2 += g.cs_slab[(size_t)(z + 2) * g.M + i];
                c3 += g.cs_slab[(size_t)(z + 3) * g.M + i];
            }
            for (; z < nsplit; ++z) c0 += g.cs_slab[(size_t)z * g.M + i];
            g.colsum[i] = (c0 + c1) + (c2 + c3);
        }
}
// ---- column sums (bias gradients) ------------------------------------------------------------------
constexpr int CS_ROWS_PER_WG = 512;
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ X, int ldx, int T, int N,
                                                             float* __restrict__ partial) {
    // block = (column block of 256, row chunk); thread = one column, 4 row phases via... keep simple:
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rphase = threadIdx.x >> 6;
    const int r0 = blockIdx.y * CS_ROWS_PER_WG, r1 = min(T, r0 + CS_ROWS_PER_WG);
    float acc = 0.f;
    if (col < N)
        for (int r = r0 + rphase; r < r1; r += 4) acc += X[(size_t)r * ldx + col];
    __shared__ float sm[4][64];
    sm[rphase][threadIdx.x & 63] = acc;
    __syncthreads();
    if (threadIdx.x < 64 && col < N)
        partial[(size_t)blockIdx.y * N + col] = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
}
__global__ __launch_bounds__(256) void segment_colsum_kernel(const float* __restrict__ X, int ldx, int R, int N,
                                                             float* __restrict__ out, int ldo, int accumulate) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x & 63, rphase = threadIdx.x >> 6;
    __shared__ float sm[4][64];
    for (int c0 = 0; c0 < N; c0 += 64) {
        const int col = c0 + lane;
        float acc = 0.f;
        if (col < N)
            for (int r = rphase; r < R; r += 4) acc += X[((size_t)g * R + r) * ldx + col];
        sm[rphase][lane] = acc;
        __syncthreads();
        if (threadIdx.x < 64 && col < N) {
            const float v = sm[0][lane] + sm[1][lane] + sm[2][lane] + sm[3][lane];
            float* dst = out + (size_t)g * ldo + col;
            *dst = accumulate ? *dst + v : v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void relu_bwd_kernel(float* __restrict__ dX, const float* __restrict__ Y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        if (!(Y[i] > 0.f)) dX[i] = 0.f;
}
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, const float* __restrict__ s, size_t n) {
    const float f = s[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) x[i] *= f;
}

// ---- narrow weight gradient: dW[M][I] = A^T X, db[M] = column sums of A, for I <= 3 ------------------------
// The LSTM layer-0 input weights (I = 3 features): as a GEMM this is a 128x128-tile product with N = 3, one pass
// over A (the 5 GB gate-gradient stash) per direction at ~2 TB/s.  Here one streaming pass covers all M columns of
// both directions: a 256-thread workgroup owns whole rows (thread = 4 consecutive columns, 16-byte loads), a chunk of
// rows, and 16 register accumulators; fixed-order two-level reduction (bitwise reproducible).
constexpr int NDW_CHUNKS = 2048;
__global__ __launch_bounds__(256) void narrow_dw_partial_kernel(const float* __restrict__ A, int lda, const float* __restrict__ X,
                                                                int ldx, int I, int T, int M, int rows_per_wg,
                                                                float* __restrict__ partial) {
    const int m4 = blockIdx.y * 256 + threadIdx.x;          // float4 column index
    const int t0 = blockIdx.x * rows_per_wg, t1 = min(T, t0 + rows_per_wg);
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, ab = a0;
    if (4 * m4 < M) {
        const float* ap = A + 4 * m4;
        for (int t = t0; t < t1; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(ap + (size_t)t * lda);
            const float* xr = X + (size_t)t * ldx;
            const float x0 = xr[0], x1 = I > 1 ? xr[1] : 0.f, x2 = I > 2 ? xr[2] : 0.f;
            a0.x += v.x * x0; a0.y += v.y * x0; a0.z += v.z * x0; a0.w += v.w * x0;
            a1.x += v.x * x1; a1.y += v.y * x1; a1.z += v.z * x1; a1.w += v.w * x1;
            a2.x += v.x * x2; a2.y += v.y * x2; a2.z += v.z * x2; a2.w += v.w * x2;
            ab.x += v.x; ab.y += v.y; ab.z += v.z; ab.w += v.w;
        }
        float* pr = partial + (size_t)blockIdx.x * 4 * M + 4 * m4;   // [chunk][f][m], f = 3 holds the column sums
        *reinterpret_cast<float4*>(pr) = a0;
        *reinterpret_cast<float4*>(pr + M) = a1;
        *reinterpret_cast<float4*>(pr + 2 * M) = a2;
        *reinterpret_cast<float4*>(pr + 3 * M) = ab;
    }
}
__global__ __launch_bounds__(256) void narrow_dw_scatter_kernel(const float* __restrict__ sums, int M, int I,
                                                                float* __restrict__ dW, float* __restrict__ db) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    for (int f = 0; f < I; ++f) dW[(size_t)m * I + f] = sums[(size_t)f * M + m];
    if (db) db[m] = sums[(size_t)3 * M + m];
}

int ew_grid(size_t n) { size_t g = (n + 1023) / 1024; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

// rlt_gemm_last_dispatch: reset to RLT_GEMM_NONE where a call enters gemm_run, set to the plan's record by the launcher right before
// its launch
thread_local rlt_gemm_dispatch rlt_gemm_dispatch_rec = {};

}  // namespace

extern "C" {

int rlt_gemm_last_dispatch(rlt_gemm_dispatch* out) {
    RLT_CHECK_ARG(out);
    *out = rlt_gemm_dispatch_rec;
    return 0;
}

int rlt_gemm(int ta, int tb, int M, int N, int K,
             const float* A, int lda, const float* B, int ldb, float* C, int ldc,
             const float* bias, const float* bias2, int flags,
             void* ws, size_t ws_bytes, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    return rlt_gemm_ex(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, bias2, flags, nullptr, 0, 1.0f, nullptr,
                       0.0f, 0u, ws, ws_bytes, RLT_PRECISION_DEFAULT, stream);
}

// check the arguments, describe the call, plan (csrc/gemm_plan.hip: every choice, and the family's switches), launch
static int gemm_run(int ta, int tb, int M, int N, int K,
                    const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                    const float* bias, const float* bias2, int flags,
                    const float* relu_mask, int ldmask, float mask_scale, float* colsum_a,
                    float drop_p, uint32_t seed, uint32_t* bits_out, const uint32_t* bits_in,
                    void* ws, size_t ws_bytes, void* stream) {
    rlt_gemm_dispatch_rec = rlt_gemm_dispatch{};
    RLT_CHECK_ARG(A && B && C && M > 0 && N > 0 && K > 0);
    RLT_CHECK_ARG(lda >= (ta ? M : K) && ldb >= (tb ? K : N) && ldc >= N);
    RLT_CHECK_ARG(!relu_mask || ldmask >= N);
    RLT_CHECK_ARG(!colsum_a || ta);          // the side column sum needs A stored [K,M]
    RLT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f);

    GemmCall c{};
    c.ta = ta; c.tb = tb; c.M = M; c.N = N; c.K = K; c.lda = lda; c.ldb = ldb; c.ldc = ldc; c.flags = flags;
    auto bit = [](bool on, int b) { return on ? b : 0; };
    c.aligned16 = bit(rlt_aligned16(A), RLT_GEMM_PTR_A) | bit(rlt_aligned16(B), RLT_GEMM_PTR_B) | bit(rlt_aligned16(C), RLT_GEMM_PTR_C) |
                  bit(rlt_aligned16(bias), RLT_GEMM_PTR_BIAS) | bit(rlt_aligned16(bias2), RLT_GEMM_PTR_BIAS2) |
                  bit(rlt_aligned16(bits_out), RLT_GEMM_PTR_BITS_OUT) | bit(rlt_aligned16(bits_in), RLT_GEMM_PTR_BITS_IN);
    c.present = bit(bias, RLT_GEMM_PTR_BIAS) | bit(bias2, RLT_GEMM_PTR_BIAS2) | bit(bits_out, RLT_GEMM_PTR_BITS_OUT) |
                bit(bits_in, RLT_GEMM_PTR_BITS_IN) | bit(relu_mask, RLT_GEMM_PTR_RELU_MASK) | bit(colsum_a, RLT_GEMM_PTR_COLSUM);
    c.drop = drop_p > 0.f; c.ws_null = ws == nullptr; c.ws_bytes = ws_bytes;

    const GemmPlan p = gemm_plan(c);
    if (p.rc) return p.rc;

    hipStream_t st = rlt_stream(stream);
    if (p.d.family == RLT_GEMM_6S) {
        const Gemm6sArgs s6{A, B, C, bias, bias2, M, N, K, lda, ldb, ldc, bits_out, bits_in, mask_scale};
        const int rc = rlt_gemm6s_launch(s6, p, &rlt_gemm_dispatch_rec, st);
        return rc ? rc : RLT_LAUNCH_RESULT();
    }
    const int ns = p.d.ns;
    GemmArgs g;
    g.mask = relu_mask; g.ldmask = ldmask; g.colsum = colsum_a;
    g.bits_out = bits_out; g.bits_in = bits_in; g.ldbits = N;
    g.mask_scale = mask_scale; g.drop_p = drop_p; g.drop_thr = rlt_drop_threshold(drop_p); g.seed = seed;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.bias2 = bias2;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.vecA = (lda % 4 == 0) && rlt_aligned16(A);
    g.vecB = (ldb % 4 == 0) && rlt_aligned16(B);
    g.flags = flags;
    g.tiles_m = p.tiles_m; g.tiles_n = p.tiles_n;
    g.kchunk = p.d.kchunk;
    g.slab_xcd = p.d.slab_xcd;
    g.slab = ns > 1 ? (float*)ws : nullptr;
    g.cs_slab = (ns > 1 && colsum_a) ? (float*)ws + (size_t)ns * M * N : nullptr;
    rlt_gemm_dispatch* rec = &rlt_gemm_dispatch_rec;
    int rc = (int)RLT_E_ARG;
    switch (p.d.family) {
    case RLT_GEMM_6E: rc = rlt_gemm6e_launch(p, g, rec, st); break;
    case RLT_GEMM_6C: rc = rlt_gemm6c_launch(p, g, rec, st); break;
    case RLT_GEMM_6B:
    case RLT_GEMM_6: rc = rlt_gemm6_launch(p, g, rec, st); break;
    case RLT_GEMM_3B:
    case RLT_GEMM_3: rc = rlt_gemm3_launch(p, g, rec, st); break;
    case RLT_GEMM_F32: rc = rlt_gemm_f32_launch(p, g, rec, st); break;
    }
    if (rc) return rc;
    if (p.reduce)
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(ew_grid((size_t)M * N)), dim3(256), 0, st, g, ns);
    return RLT_LAUNCH_RESULT();
}

int rlt_gemm_ex(int ta, int tb, int M, int N, int K,
                const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                const float* bias, const float* bias2, int flags,
                const float* relu_mask, int ldmask, float mask_scale, float* colsum_a,
                float drop_p, uint32_t seed,
                void* ws, size_t ws_bytes, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    return gemm_run(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, bias2, flags, relu_mask, ldmask, mask_scale, colsum_a,
                    drop_p, seed, nullptr, nullptr, ws, ws_bytes, stream);
}

size_t rlt_gemm_bits_words(int M, int N) { return M > 0 && N > 0 ? (size_t)rlt_cdiv(M, 32) * N : 0; }

int rlt_gemm_bits(int ta, int tb, int M, int N, int K,
                  const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, int flags, float drop_p, uint32_t seed,
                  uint32_t* relu_bits_out, const uint32_t* mask_bits_in, float mask_scale,
                  int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG((relu_bits_out != nullptr) != (mask_bits_in != nullptr));
    RLT_CHECK_ARG(!relu_bits_out || (flags & RLT_GEMM_RELU));
    RLT_CHECK_ARG(drop_p == 0.f || relu_bits_out);
    RLT_CHECK_SHAPE(N % 32 == 0);
    return gemm_run(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias, nullptr, flags, nullptr, 0, mask_scale, nullptr,
                    drop_p, seed, relu_bits_out, mask_bits_in, nullptr, 0, stream);
}

size_t rlt_colsum_workspace(int T, int N) {
    if (T <= 0 || N <= 0) return 0;
    return (size_t)rlt_cdiv(T, CS_ROWS_PER_WG) * N * sizeof(float);
}

int rlt_colsum(const float* X, int ldx, int T, int N, float* out, int accumulate,
               void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(X && out && ws && T > 0 && N > 0 && ldx >= N);
    if (ws_bytes < rlt_colsum_workspace(T, N)) return RLT_E_WORKSPACE;
    const int nchunk = rlt_cdiv(T, CS_ROWS_PER_WG);
    hipStream_t st = rlt_stream(stream);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(rlt_cdiv(N, 64), nchunk), dim3(256), 0, st, X, ldx, T, N, (float*)ws);
    hipLaunchKernelGGL(rlt_rows_reduce_kernel, dim3(rlt_cdiv(N, 16)), dim3(256), 0, st, (const float*)ws, nchunk, N, N, N, out, out, accumulate);
    return RLT_LAUNCH_RESULT();
}

int rlt_segment_colsum(const float* X, int ldx, int G, int R, int N, float* out, int ldo,
                       int accumulate, void* stream) {
    RLT_CHECK_ARG(X && out && G > 0 && R > 0 && N > 0 && ldx >= N && ldo >= N);
    hipLaunchKernelGGL(segment_colsum_kernel, dim3(G), dim3(256), 0, rlt_stream(stream), X, ldx, R, N, out, ldo, accumulate);
    return RLT_LAUNCH_RESULT();
}

size_t rlt_narrow_dw_workspace(int T, int M) {
    if (T <= 0 || M <= 0) return 0;
    const int rows = rlt_cdiv(T, NDW_CHUNKS);
    const int nchunk = rlt_cdiv(T, rows);
    return ((size_t)nchunk * 4 * M + (size_t)4 * M) * sizeof(float);
}

int rlt_narrow_dw(const float* A, int lda, const float* X, int ldx, int I, int T, int M,
                  float* dW, float* db, void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(A && X && dW && ws && T > 0 && M > 0 && lda >= M && ldx >= I);
    RLT_CHECK_SHAPE(I >= 1 && I <= 3 && M % 4 == 0 && lda % 4 == 0);
    if (!rlt_aligned16(A)) return RLT_E_ALIGN;
    if (ws_bytes < rlt_narrow_dw_workspace(T, M)) return RLT_E_WORKSPACE;
    const int rows = rlt_cdiv(T, NDW_CHUNKS);
    const int nchunk = rlt_cdiv(T, rows);
    float* partial = (float*)ws;
    float* sums = partial + (size_t)nchunk * 4 * M;
    hipStream_t st = rlt_stream(stream);
    hipLaunchKernelGGL(narrow_dw_partial_kernel, dim3(nchunk, rlt_cdiv(M, 1024)), dim3(256), 0, st, A, lda, X, ldx, I, T, M, rows, partial);
    hipLaunchKernelGGL(rlt_rows_reduce_kernel, dim3(rlt_cdiv(4 * M, 16)), dim3(256), 0, st, (const float*)partial, nchunk, 4 * M,
                       4 * M, 4 * M, sums, sums, 0);
    hipLaunchKernelGGL(narrow_dw_scatter_kernel, dim3(rlt_cdiv(M, 256)), dim3(256), 0, st, (const float*)sums, M, I, dW, db);
    return RLT_LAUNCH_RESULT();
}

int rlt_relu_bwd(float* dX, const float* Y, size_t n, void* stream) {
    RLT_CHECK_ARG(dX && Y && n > 0);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, rlt_stream(stream), dX, Y, n);
    return RLT_LAUNCH_RESULT();
}

int rlt_scale(float* x, const float* scale, size_t n, void* stream) {
    RLT_CHECK_ARG(x && scale && n > 0);
    hipLaunchKernelGGL(scale_kernel, dim3(ew_grid(n)), dim3(256), 0, rlt_stream(stream), x, scale, n);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
