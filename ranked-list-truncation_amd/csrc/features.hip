// Neighbour-similarity input features of the AttnCut family (the reference's data_prep/data_review.ipynb simi_list and
// data_prep/document_statics.ipynb neighbor_sim): per position of a ranked list the cosine similarity of its document to the
// documents ranked next to it, over the sparse tf-idf rows and over the dense doc2vec rows.
//
//   sim(a, b) = (a . b) / (|a| |b|), 0 when the denominator is 0 or the quotient is NaN;
//   position 0: sim(0, 1);  position S-1: sim(S-2, S-1);  position i in between: (sim(i-1, i) + sim(i, i+1)) / 2.
//
// A wavefront owns FEAT_CH = 64 positions of one list and walks the documents of those positions, plus one on either side, in
// rank order: up to 66 documents, 65 pairs.  Lane j of the wavefront is position i0 + j; every pair's similarity is computed by
// the whole wavefront (the same value in every lane) and kept by the two lanes it belongs to, as `left` or `right`.
//   dense row:  element r * 64 + lane in register r (coalesced 256-byte loads), the next document's row loaded before the
//               current one is reduced; |x|^2 and x . previous from float64 products, two wavefront sums (DPP, fixed order);
//   sparse row: lanes take the entries of the current row, 64 at a time, square them for the norm and look their term up in
//               the PREVIOUS row by a binary search of uniform depth - in LDS where the previous row was staged (rows of up to
//               FEAT_CAP entries, which is nearly all of robust04), in global memory otherwise; the current row is staged for
//               the next pair as it is read, so every row is fetched once per list chunk.
// Everything is float64 up to the one rounding of the result.  No atomics, no workspace, one launch.
//
// Algorithmic bytes per position: 4 (id) + 4 D + 12 nnz + 8 (two float32 outputs).
#include "common.h"

namespace {

constexpr int FEAT_CH = 64;        // positions per wavefront
constexpr int FEAT_WAVES = 4;      // wavefronts per workgroup
constexpr int FEAT_CAP = 128;      // sparse entries staged in LDS per row (2 rows x 12 B x 128 = 3 KiB per wavefront)
constexpr int FEAT_MAX_D = 1024;

struct FeatArgs {
    const int32_t* ids;             // (B, S)
    int B, S, cpl;                  // cpl: chunks per list
    const float* d2v;               // (n_docs, D), row stride ldd; null: no dense column
    int D;
    long long ldd;
    const int64_t* indptr;          // null: no sparse column
    const int32_t* indices;
    const double* values;
    float* out;
    long long ldo;
    int col_sparse, col_dense;      // columns of the two results
};

__device__ __forceinline__ double cos_sim(double dot, double na, double nb) {
    const double denom = sqrt(na) * sqrt(nb);
    const double s = denom != 0.0 ? dot / denom : 0.0;      // a NaN denominator is "not 0": the quotient is NaN
    return s != s ? 0.0 : s;
}

// R: dense registers per lane, ceil(D / 64); 0 without a dense table
template <int R>
__global__ __launch_bounds__(256) void neighbor_features_kernel(FeatArgs a) {
    __shared__ int32_t s_idx[FEAT_WAVES][2][FEAT_CAP];
    __shared__ double s_val[FEAT_WAVES][2][FEAT_CAP];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long chunk = (long long)blockIdx.x * FEAT_WAVES + wv;
    if (chunk >= (long long)a.B * a.cpl) return;                    // whole wavefronts leave; no workgroup barrier below
    const int b = (int)(chunk / a.cpl), c = (int)(chunk % a.cpl);
    const int S = a.S;
    const int i0 = c * FEAT_CH, i1 = min(i0 + FEAT_CH, S);
    const int t0 = max(i0 - 1, 0), t1 = min(i1, S - 1);             // documents t0..t1: at most 66
    const int32_t* ids = a.ids + (size_t)b * S;
    const int id_a = t0 + lane <= t1 ? ids[t0 + lane] : 0;
    const int id_b = t0 + 64 + lane <= t1 ? ids[t0 + 64 + lane] : 0;
    const auto doc = [&](int t) {      // a scalar: t is the same in every lane
        const int j = t - t0;
        return __builtin_amdgcn_readfirstlane(j < 64 ? __shfl(id_a, j) : __shfl(id_b, j - 64));
    };
    const bool sparse = a.indptr != nullptr;

    float cur[R > 0 ? R : 1] = {}, nxt[R > 0 ? R : 1] = {};
    const auto load_row = [&](int id, float* dst) {
        const float* row = a.d2v + (size_t)id * a.ldd;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = r * 64 + lane;
            dst[r] = (r + 1 < R || k < a.D) ? row[k] : 0.f;      // only the last register can be partial
        }
    };
    if constexpr (R > 0) load_row(doc(t0), nxt);

    double d_nrm_prev = 0.0, s_nrm_prev = 0.0;
    long long p_beg = 0;
    int p_n = 0;
    double left_s = 0.0, right_s = 0.0, left_d = 0.0, right_d = 0.0;
    for (int t = t0; t <= t1; ++t) {
        const int id = doc(t);
        const int buf = (t - t0) & 1;
        double d_nrm = 0.0, d_dot = 0.0, s_nrm = 0.0, s_dot = 0.0;
        if constexpr (R > 0) {
            float prev[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { prev[r] = cur[r]; cur[r] = nxt[r]; }
            if (t < t1) load_row(doc(t + 1), nxt);
            double pn = 0.0, pd = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double x = (double)cur[r];
                pn += x * x;
                if (t > t0) pd += x * (double)prev[r];
            }
            d_nrm = wave_sum(pn);
            d_dot = wave_sum(pd);
        }
        long long beg = 0;
        int n = 0;
        if (sparse) {
            beg = a.indptr[id];
            n = (int)(a.indptr[id + 1] - beg);
            const bool prev_lds = p_n <= FEAT_CAP;
            const int32_t* p_idx_g = a.indices + p_beg;
            const double* p_val_g = a.values + p_beg;
            const int32_t* p_idx_s = s_idx[wv][buf ^ 1];
            const double* p_val_s = s_val[wv][buf ^ 1];
            int top = 0;                                            // the largest power of two <= p_n
            if (t > t0 && p_n > 0) top = 1 << (31 - __builtin_clz(p_n));
            double pn = 0.0, pd = 0.0;
            for (int base = 0; base < n; base += 64) {
                const int k = base + lane;
                const bool live = k < n;
                const int32_t ix = live ? a.indices[beg + k] : 0;
                const double v = live ? a.values[beg + k] : 0.0;
                pn += v * v;
                if (top) {
                    // lower bound of ix in the previous row, the same number of steps in every lane
                    int lo = 0;
                    for (int s = top; s > 0; s >>= 1) {
                        const int m = lo + s - 1;
                        if (m < p_n) {
                            const int32_t pv = prev_lds ? p_idx_s[m] : p_idx_g[m];
                            if (pv < ix) lo = m + 1;
                        }
                    }
                    if (live && lo < p_n) {
                        const int32_t pv = prev_lds ? p_idx_s[lo] : p_idx_g[lo];
                        if (pv == ix) pd += v * (prev_lds ? p_val_s[lo] : p_val_g[lo]);
                    }
                }
                if (live && n <= FEAT_CAP) {                        // n <= FEAT_CAP: k < FEAT_CAP
                    s_idx[wv][buf][k] = ix;
                    s_val[wv][buf][k] = v;
                }
            }
            __builtin_amdgcn_wave_barrier();      // LDS is in-order per wavefront: the next pair's reads see these stores
            s_nrm = wave_sum(pn);
            s_dot = wave_sum(pd);
        }
        if (t > t0) {
            const int i = i0 + lane;
            if (sparse) {
                const double sim = cos_sim(s_dot, s_nrm_prev, s_nrm);
                if (i == t - 1) right_s = sim;
                if (i == t) left_s = sim;
            }
            if constexpr (R > 0) {
                const double sim = cos_sim(d_dot, d_nrm_prev, d_nrm);
                if (i == t - 1) right_d = sim;
                if (i == t) left_d = sim;
            }
        }
        d_nrm_prev = d_nrm;
        s_nrm_prev = s_nrm;
        p_beg = beg;
        p_n = n;
    }
    const int i = i0 + lane;
    if (i < i1) {
        float* o = a.out + ((size_t)b * S + i) * a.ldo;
        if (sparse) o[a.col_sparse] = (float)(i == 0 ? right_s : i == S - 1 ? left_s : (left_s + right_s) / 2.0);
        if constexpr (R > 0) o[a.col_dense] = (float)(i == 0 ? right_d : i == S - 1 ? left_d : (left_d + right_d) / 2.0);
    }
}

template <int R>
void launch_features(const FeatArgs& a, hipStream_t st) {
    const long long chunks = (long long)a.B * a.cpl;
    hipLaunchKernelGGL((neighbor_features_kernel<R>), dim3((unsigned)((chunks + FEAT_WAVES - 1) / FEAT_WAVES)), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int rlt_neighbor_features(const int32_t* doc_ids, int B, int S, int n_docs, const float* d2v, int D, int ld_d2v,
                          const int64_t* indptr, const int32_t* indices, const double* values,
                          float* out, int ld_out, int col, void* stream) {
    RLT_CHECK_ARG(doc_ids && out && B > 0 && S >= 2 && n_docs > 0 && col >= 0);
    const bool sparse = indptr || indices || values;
    RLT_CHECK_ARG(d2v || sparse);
    if (sparse) RLT_CHECK_ARG(indptr && indices && values);
    RLT_CHECK_SHAPE((long long)B * S < (1ll << 31));
    if (d2v) {
        RLT_CHECK_ARG(D > 0);
        RLT_CHECK_SHAPE(D <= FEAT_MAX_D);
        RLT_CHECK_ARG(ld_d2v >= D);
    }
    const int ncol = (sparse ? 1 : 0) + (d2v ? 1 : 0);
    RLT_CHECK_ARG(ld_out >= col + ncol);
    if ((((uintptr_t)doc_ids | (uintptr_t)out | (uintptr_t)d2v | (uintptr_t)indices) & 3u) != 0) return RLT_E_ALIGN;
    if ((((uintptr_t)indptr | (uintptr_t)values) & 7u) != 0) return RLT_E_ALIGN;
    FeatArgs a{doc_ids, B, S, rlt_cdiv(S, FEAT_CH), d2v, d2v ? D : 0, ld_d2v, sparse ? indptr : nullptr, indices, values,
               out, ld_out, col, col + (sparse ? 1 : 0)};
    hipStream_t st = rlt_stream(stream);
    switch (d2v ? rlt_cdiv(D, 64) : 0) {
        case 0: launch_features<0>(a, st); break;
        case 1: launch_features<1>(a, st); break;
        case 2: launch_features<2>(a, st); break;
        case 3: launch_features<3>(a, st); break;
        case 4: launch_features<4>(a, st); break;
        case 5: launch_features<5>(a, st); break;
        case 6: launch_features<6>(a, st); break;
        case 7: launch_features<7>(a, st); break;
        case 8: launch_features<8>(a, st); break;
        case 9: launch_features<9>(a, st); break;
        case 10: launch_features<10>(a, st); break;
        case 11: launch_features<11>(a, st); break;
        case 12: launch_features<12>(a, st); break;
        case 13: launch_features<13>(a, st); break;
        case 14: launch_features<14>(a, st); break;
        case 15: launch_features<15>(a, st); break;
        default: launch_features<16>(a, st); break;
    }
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
