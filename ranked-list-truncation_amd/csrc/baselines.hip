// Truncation baselines: the Oracle / Fixed-k / Greedy-k rows and the per-position analysis of the reference's Baseline/
// notebooks, from one pass over the labels that returns the whole truncation curve.
//
// For a list of S labels (0/1 in rank order), c_k = hits in the first k, N = hits in the list, k = 1..S:
//   F1@k  = 2 p r / (p + r), p = c_k / k, r = c_k / N (0 if N = 0), 0 if p + r = 0 - float64, the notebooks' cal_F1 operation
//           order, correctly rounded division (no fast-math, no contraction): exactly tied values come out bit-identical, so
//           the first maximum is the one np.argmax finds;
//   DCG@k = sum_{i<k} (label == 1 ? 1 : penalty) / log2(i + 2) in float64 (cal_DCG), coefficients from the caller's DCG table;
//   k = 0 is an entry of every curve, value 0 (the notebooks' `per_k_F1, per_k_DCG = [0], [0]`).
// Outputs: the sums over lists of F1@k, DCG@k and c_k for k = 0..S (the mean curves once divided by the list count), each
// list's best F1 / DCG over k = 0..S with its first-maximum k, and the sums of those bests.
//
// A wavefront owns whole lists (one per wavefront, or four - one per row of 16 lanes - at S <= 64: mq2007's 40 positions then
// fill 48 lane slots instead of 64) and keeps its running sums for every k in registers, ceil(S / 64) (ceil(S / 16)) per lane
// and curve.  Position j of a list sits in lane j % L of round j / L (L = 64 or 16): loads are coalesced, and the prefix sums
// are one DPP scan per round plus the carry of the rounds before.  The workgroup's four wavefronts add their sums in LDS in a
// fixed order and write one record; a second launch adds the records column by column in a fixed order into the caller's
// curves (or onto them: `accumulate`).  No atomics: the same inputs give bitwise identical outputs.
//
// Algorithmic bytes: 4 S per list read (+ 24 B of per-list results when asked for).
#include "common.h"

namespace {

constexpr int CURVES_MAX_S = 1024;      // the DCG table's length, as for the other metric entry points
constexpr int CURVES_WAVES = 4;         // wavefronts per workgroup
constexpr int CURVES_MAX_GRID = 1024;   // workgroups (4 per CU); beyond that they stride over the lists

__host__ __device__ constexpr int curves_cols(int S) { return 3 * S + 2; }   // record: F1, DCG, c sums for k = 1..S, sum best F1, sum best DCG

struct CurvesArgs {
    const float* y;         // (B, S) labels
    const double* tab;      // DCG table: [j] = 1 / log2(j + 2)
    int B, S;
    double penalty;
    double* best_f1;        // (B) or null
    int32_t* best_f1_k;     // (B) or null
    double* best_dcg;       // (B) or null
    int32_t* best_dcg_k;    // (B) or null
    double* records;        // (grid, curves_cols(S))
};

template <int L, int R>
__global__ __launch_bounds__(256) void truncation_curves_kernel(CurvesArgs a) {
    constexpr int G = 64 / L;                   // lists per wavefront
    extern __shared__ double red[];             // curves_cols(S)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane / L, l = lane % L;
    const int S = a.S;
    const auto add = [](double x, double z) { return x + z; };
    double coef[R], f1s[R], dcgs[R], cs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = r * L + l;
        coef[r] = j < S ? a.tab[j] : 0.0;
        f1s[r] = dcgs[r] = cs[r] = 0.0;
    }
    double sum_bf = 0.0, sum_bd = 0.0;          // this lane's lists (lane l == 0 of a group)
    const long long waves = (long long)gridDim.x * CURVES_WAVES;
    for (long long w = (long long)blockIdx.x * CURVES_WAVES + wv; w * G < a.B; w += waves) {
        const long long b = w * G + grp;
        const bool live = b < a.B;
        const float* row = a.y + (size_t)(live ? b : 0) * S;
        float yv[R];
        double n_lane = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = r * L + l;
            yv[r] = (live && j < S) ? row[j] : 0.f;
            n_lane += (double)yv[r];
        }
        const double N = rlt_group_reduce<L>(n_lane, 0.0, add, lane);          // hits in the list
        double c_carry = 0.0, d_carry = 0.0;
        double bf = 0.0, bd = 0.0;              // k = 0: value 0
        int kf = 0, kd = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = r * L + l;
            const bool valid = live && j < S;
            const double gain = valid ? ((yv[r] == 1.f) ? 1.0 : a.penalty) * coef[r] : 0.0;
            const double ci = rlt_group_scan<L>((double)yv[r], 0.0, add);
            const double di = rlt_group_scan<L>(gain, 0.0, add);
            const double c = c_carry + ci, dcg = d_carry + di;
            if (r + 1 < R) {
                c_carry += rlt_group_last<L>(ci, lane);
                d_carry += rlt_group_last<L>(di, lane);
            }
            // cal_F1, operation for operation
            const double p = c / (double)(j + 1);
            const double rc = (N != 0.0) ? c / N : 0.0;
            const double f1 = (p + rc != 0.0) ? 2.0 * p * rc / (p + rc) : 0.0;
            if (valid) {
                f1s[r] += f1;
                dcgs[r] += dcg;
                cs[r] += c;
                if (f1 > bf) { bf = f1; kf = j + 1; }       // a lane's positions rise with r: its first maximum
                if (dcg > bd) { bd = dcg; kd = j + 1; }
            }
        }
        // first maximum over the list: the group's maximum, then the smallest k among the lanes that hold it (a lane that never
        // rose above 0 holds k = 0)
        const auto mx = [](double x, double z) { return x > z ? x : z; };
        const auto mn = [](int x, int z) { return x < z ? x : z; };
        const double mf = rlt_group_reduce<L>(bf, 0.0, mx, lane), md = rlt_group_reduce<L>(bd, 0.0, mx, lane);
        const int kfm = rlt_group_reduce<L>(bf == mf ? kf : 0x7fffffff, 0x7fffffff, mn, lane);
        const int kdm = rlt_group_reduce<L>(bd == md ? kd : 0x7fffffff, 0x7fffffff, mn, lane);
        if (live && l == 0) {
            if (a.best_f1) a.best_f1[b] = mf;
            if (a.best_f1_k) a.best_f1_k[b] = kfm;
            if (a.best_dcg) a.best_dcg[b] = md;
            if (a.best_dcg_k) a.best_dcg_k[b] = kdm;
            sum_bf += mf;
            sum_bd += md;
        }
    }
    if constexpr (G == 4) {                     // the four rows hold the same k: (row 0 + row 1) + (row 2 + row 3) into row 0
#pragma unroll
        for (int r = 0; r < R; ++r) {
            f1s[r] += __shfl_down(f1s[r], 16);
            dcgs[r] += __shfl_down(dcgs[r], 16);
            cs[r] += __shfl_down(cs[r], 16);
            f1s[r] += __shfl_down(f1s[r], 32);
            dcgs[r] += __shfl_down(dcgs[r], 32);
            cs[r] += __shfl_down(cs[r], 32);
        }
        sum_bf += __shfl_down(sum_bf, 16);
        sum_bd += __shfl_down(sum_bd, 16);
        sum_bf += __shfl_down(sum_bf, 32);
        sum_bd += __shfl_down(sum_bd, 32);
    }
    // the workgroup's record: wavefront 0, 1, 2, 3 in turn (fixed order)
    for (int w = 0; w < CURVES_WAVES; ++w) {
        if (wv == w && lane < L) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = r * L + lane;
                if (j < S) {
                    red[j] = w ? red[j] + f1s[r] : f1s[r];
                    red[S + j] = w ? red[S + j] + dcgs[r] : dcgs[r];
                    red[2 * S + j] = w ? red[2 * S + j] + cs[r] : cs[r];
                }
            }
            if (lane == 0) {
                red[3 * S] = w ? red[3 * S] + sum_bf : sum_bf;
                red[3 * S + 1] = w ? red[3 * S + 1] + sum_bd : sum_bd;
            }
        }
        __syncthreads();
    }
    const int ncol = curves_cols(S);
    for (int i = tid; i < ncol; i += 256) a.records[(size_t)blockIdx.x * ncol + i] = red[i];
}

// column sums of the records in a fixed order (16 row lanes x 16 columns per workgroup, four loads in flight per lane, then the
// row lanes in order) into curves (3, S + 1) at k = 1..S and sums[0..1]; k = 0 and the list count (sums[2]) from the arguments
__global__ __launch_bounds__(256) void truncation_curves_final_kernel(const double* __restrict__ rec, int rows, int S, int B,
                                                                      int accumulate, double* __restrict__ curves,
                                                                      double* __restrict__ sums) {
    __shared__ double part[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int ncol = curves_cols(S);
    const int col = blockIdx.x * 16 + cx;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (col < ncol) {
        const double* p = rec + col;
        int r = ry;
        for (; r + 48 < rows; r += 64) {
            a0 += p[(size_t)r * ncol];
            a1 += p[(size_t)(r + 16) * ncol];
            a2 += p[(size_t)(r + 32) * ncol];
            a3 += p[(size_t)(r + 48) * ncol];
        }
        for (; r < rows; r += 16) a0 += p[(size_t)r * ncol];
    }
    part[ry][cx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ry == 0 && col < ncol) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc += part[i][cx];
        double* dst = col < 3 * S ? curves + (size_t)(col / S) * (S + 1) + col % S + 1 : (sums ? sums + (col - 3 * S) : nullptr);
        if (dst) *dst = accumulate ? *dst + acc : acc;
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        if (!accumulate) curves[(size_t)threadIdx.x * (S + 1)] = 0.0;      // k = 0: 0 for every list (adding 0 changes nothing)
        if (threadIdx.x == 0 && sums) sums[2] = (accumulate ? sums[2] : 0.0) + (double)B;
    }
}

int curves_grid(int B, int S) {
    const int lists_per_wg = CURVES_WAVES * (S <= 64 ? 4 : 1);
    const int groups = rlt_cdiv(B, lists_per_wg);
    return groups < CURVES_MAX_GRID ? groups : CURVES_MAX_GRID;
}

template <int L, int R>
void launch_curves(const CurvesArgs& a, int grid, hipStream_t st) {
    hipLaunchKernelGGL((truncation_curves_kernel<L, R>), dim3(grid), dim3(256), (size_t)curves_cols(a.S) * sizeof(double), st, a);
}

void dispatch_curves(const CurvesArgs& a, int grid, hipStream_t st) {
    if (a.S <= 64) {
        switch (rlt_cdiv(a.S, 16)) {
            case 1: return launch_curves<16, 1>(a, grid, st);
            case 2: return launch_curves<16, 2>(a, grid, st);
            case 3: return launch_curves<16, 3>(a, grid, st);
            default: return launch_curves<16, 4>(a, grid, st);
        }
    }
    switch (rlt_cdiv(a.S, 64)) {
        case 2: return launch_curves<64, 2>(a, grid, st);
        case 3: return launch_curves<64, 3>(a, grid, st);
        case 4: return launch_curves<64, 4>(a, grid, st);
        case 5: return launch_curves<64, 5>(a, grid, st);
        case 6: return launch_curves<64, 6>(a, grid, st);
        case 7: return launch_curves<64, 7>(a, grid, st);
        case 8: return launch_curves<64, 8>(a, grid, st);
        case 9: return launch_curves<64, 9>(a, grid, st);
        case 10: return launch_curves<64, 10>(a, grid, st);
        case 11: return launch_curves<64, 11>(a, grid, st);
        case 12: return launch_curves<64, 12>(a, grid, st);
        case 13: return launch_curves<64, 13>(a, grid, st);
        case 14: return launch_curves<64, 14>(a, grid, st);
        case 15: return launch_curves<64, 15>(a, grid, st);
        default: return launch_curves<64, 16>(a, grid, st);
    }
}

}  // namespace

extern "C" {

size_t rlt_truncation_curves_workspace(int B, int S) {
    if (B <= 0 || S <= 0 || S > CURVES_MAX_S) return 0;
    return ((size_t)curves_grid(B, S) * curves_cols(S) * sizeof(double) + 15) / 16 * 16;     // one record per workgroup
}

int rlt_truncation_curves(const float* labels, int B, int S, double penalty, const void* dcg_table, int accumulate,
                          double* curves, double* best_f1, int32_t* best_f1_k, double* best_dcg, int32_t* best_dcg_k,
                          double* sums, void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(labels && curves && dcg_table && ws && B > 0 && S > 0);
    RLT_CHECK_SHAPE(S <= CURVES_MAX_S);
    if ((((uintptr_t)dcg_table | (uintptr_t)ws | (uintptr_t)curves) & 7u) != 0 || ((uintptr_t)labels & 3u) != 0) return RLT_E_ALIGN;
    if (ws_bytes < rlt_truncation_curves_workspace(B, S)) return RLT_E_WORKSPACE;
    const int grid = curves_grid(B, S);
    CurvesArgs a{labels, (const double*)dcg_table, B, S, penalty, best_f1, best_f1_k, best_dcg, best_dcg_k, (double*)ws};
    hipStream_t st = rlt_stream(stream);
    dispatch_curves(a, grid, st);
    hipLaunchKernelGGL(truncation_curves_final_kernel, dim3(rlt_cdiv(curves_cols(S), 16)), dim3(256), 0, st, (const double*)ws, grid,
                       S, B, accumulate ? 1 : 0, curves, sums);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
