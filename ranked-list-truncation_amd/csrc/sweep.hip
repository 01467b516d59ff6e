// Cut sweep: T threshold cut rules evaluated at once from one read of a per-position value array v and of the labels - the
// effectiveness / cost curve of a trained cut distribution (QUANTILE), of a per-position stop probability (FIRST_ABOVE) and of
// the retrieval scores themselves (FIRST_BELOW, the tuned score-threshold baseline).  The reference only ever takes the argmax.
//
// Rules, positions j = 1..S, threshold tau (float64; v is widened to float64 before every comparison, a NaN compares false):
//   QUANTILE     C_j = the float64 inclusive prefix sum of v;  k = 1 + #{ j in 1..S-1 : C_j < tau * C_S }  (1..S): the smallest k
//                whose mass reaches the share tau.  tau * C_S is one float64 multiply.  A list whose total is 0 or NaN gets k = 1.
//   FIRST_BELOW  k = the number of leading positions with v_j >= tau  (0..S; k = 0 keeps nothing and every metric is 0).
//   FIRST_ABOVE  k = the first j with v_j >= tau, S if there is none  (1..S).
// Per (list, threshold), with c_k = the number of labels equal to 1 among the first k and N = their number in the list:
//   P = c_k / k (0 at k = 0), R = c_k / N (0 if N = 0), F1 = 2 P R / (P + R) (0 if P + R = 0) - rlt_cut_metrics_ex's operation
//   order on the same integers, so bit-identical to it for k >= 1 -, F_beta = ((1 + beta^2) P) R / (beta^2 P + R) (0 if the
//   denominator is 0), DCG@k = sum_{j <= k} (label == 1 ? 1 : penalty) * tab[j] with tab the caller's 1 / log2(j + 1) table.
//
// Layout: a wavefront owns whole lists, position j - 1 sits in lane (j - 1) % 64 of round (j - 1) / 64 (R rounds, a template
// parameter, so the list stays in registers).  Per list: one 64-lane inclusive scan per round, carried across the rounds in
// position order, of v (QUANTILE; the other rules compare v itself), of the relevant count (int32) and of the DCG terms
// (float64).  C stays in registers - a lane's k never indexes it -; the count and DCG prefixes go to the wavefront's own LDS
// rows (12 bytes per position: 12 KB per wavefront at S = 1024).  The count that defines k is taken per threshold over the
// whole wavefront (compare, ballot, population count: T * R compares per list, fewer than the S a lane of its own would
// need); then the T thresholds are finished in parallel, lane t reading the two prefixes at its own k and adding the eight
// values into its registers.  The four wavefronts of a workgroup are combined in wavefront order into one float64 record of
// 8 * T values in the workspace and a second launch sums the records per column in a fixed order.  No atomics, no allocation,
// no host synchronisation: the same inputs give bitwise identical outputs.
//
// One list per wavefront at every S: at S <= 64 three quarters of the scan lanes idle, but the per-threshold tail (T lanes)
// does not shrink with S, so the four-lists-per-wavefront form of the sibling passes was not built.
//
// Algorithmic bytes per list: 8 S read (4 S without labels) + 4 T of cuts written.
#include "common.h"

namespace {

constexpr int SWEEP_MAX_S = 1024;
constexpr int SWEEP_MAX_T = 64;
constexpr int SWEEP_WAVES = 4;
constexpr int SWEEP_MAX_GRID = 2048;

struct SweepArgs {
    const float* v;         // (B, S) read at element stride `stride`
    const float* y;         // (B, S); not read without LABELS
    const double* thr;      // (T)
    const double* tab;      // DCG table: [j] = 1 / log2(j + 2)
    int B, S, T, stride, rule;
    double penalty, beta2;
    int32_t* k;             // (B, T) or null
    double* records;        // (grid, RLT_SWEEP_COLS * T)
};

template <int R, bool LABELS>
__global__ __launch_bounds__(256) void cut_sweep_kernel(SweepArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sh[];     // DCG prefixes (4 x R*64 float64), count prefixes (4 x R*64 int32); then the record
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.S, T = a.T;
    double* const dpre = sh + wv * (R * 64);
    int* const cpre = reinterpret_cast<int*>(sh + SWEEP_WAVES * (R * 64)) + wv * (R * 64);
    const double tau = lane < T ? a.thr[lane] : 0.0;
    const bool quantile = a.rule == RLT_SWEEP_QUANTILE, below = a.rule == RLT_SWEEP_FIRST_BELOW;
    const int last_r = (S - 1) >> 6, last_lane = (S - 1) & 63;
    double cf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = r * 64 + lane;
        cf[r] = (LABELS && j < S) ? a.tab[j] : 0.0;
    }
    double acc[RLT_SWEEP_COLS];
#pragma unroll
    for (int i = 0; i < RLT_SWEEP_COLS; ++i) acc[i] = 0.0;
    const long long waves = (long long)gridDim.x * SWEEP_WAVES;
    for (long long b = (long long)blockIdx.x * SWEEP_WAVES + wv; b < a.B; b += waves) {
        const size_t base = (size_t)b * S;
        float xv[R], yv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = r * 64 + lane;
            xv[r] = yv[r] = 0.f;
            if (j < S) {
                xv[r] = a.v[(base + j) * a.stride];
                if constexpr (LABELS) yv[r] = a.y[base + j];
            }
        }
        // ---- the value each position is compared by: C_j (QUANTILE) or v_j ---------------------------------------------
        double x[R], cs = 0.0;
        if (quantile) {
            double carry = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double s = wave_scan_incl((double)xv[r], lane);
                x[r] = carry + s;
                if (r + 1 < R) carry += rlt_readlane(s, 63);
                if (r == last_r) cs = rlt_readlane(x[r], last_lane);        // C_S: the prefix at the last position itself
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = (double)xv[r];
        }
        // ---- the cut of every threshold: a wavefront-wide count / first position, kept by lane t ------------------------
        int k = 0;
        if (quantile) {
            const double tc = tau * cs;
            for (int t = 0; t < T; ++t) {
                const double th = rlt_readlane(tc, t);
                int n = 1;
#pragma unroll
                for (int r = 0; r < R; ++r) n += __popcll(__ballot(r * 64 + lane < S - 1 && x[r] < th));
                if (lane == t) k = n;
            }
        } else {
            for (int t = 0; t < T; ++t) {
                const double th = rlt_readlane(tau, t);
                int first = -1;                     // 0-based: FIRST_BELOW the first position that is not >= tau, FIRST_ABOVE the first that is
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const unsigned long long m = __ballot(r * 64 + lane < S && (x[r] >= th) != below);
                    if (m != 0ull && first < 0) first = r * 64 + (__ffsll((long long)m) - 1);
                }
                const int n = first < 0 ? S : (below ? first : first + 1);
                if (lane == t) k = n;
            }
        }
        if (a.k && lane < T) a.k[(size_t)b * T + lane] = k;
        if constexpr (LABELS) {
            // ---- prefixes of the relevant count and of the DCG terms into this wavefront's LDS rows --------------------------
            int c_carry = 0;
            double d_carry = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = r * 64 + lane;
                const bool rel = yv[r] == 1.f;      // lanes beyond S hold 0
                const double gain = j < S ? (rel ? cf[r] : a.penalty * cf[r]) : 0.0;
                const int ci = wave_scan_incl(rel ? 1 : 0, lane);
                const double di = wave_scan_incl(gain, lane);
                cpre[j] = c_carry + ci;
                dpre[j] = d_carry + di;
                c_carry += rlt_readlane(ci, 63);
                if (r + 1 < R) d_carry += rlt_readlane(di, 63);
            }
            const int n_rel = c_carry;
            __builtin_amdgcn_wave_barrier();
            if (lane < T) {                         // k in 0..S by construction: k - 1 stays inside the rows
                const double hits = k > 0 ? (double)cpre[k - 1] : 0.0;
                const double dcg = k > 0 ? dpre[k - 1] : 0.0;
                const double prec = k > 0 ? hits / (double)k : 0.0;
                const double rec = n_rel != 0 ? hits / (double)n_rel : 0.0;
                const double f1 = (prec + rec != 0.0) ? 2.0 * prec * rec / (prec + rec) : 0.0;
                const double den = a.beta2 * prec + rec;
                const double fb = den != 0.0 ? (1.0 + a.beta2) * prec * rec / den : 0.0;
                acc[0] += (double)k;
                acc[1] += f1;
                acc[2] += dcg;
                acc[3] += prec;
                acc[4] += rec;
                acc[5] += fb;
                acc[6] += k == S ? 1.0 : 0.0;
                acc[7] += 1.0;
            }
            __builtin_amdgcn_wave_barrier();        // the next list's stores come after these loads
        }
    }
    if constexpr (LABELS) {
        __syncthreads();                            // the prefix rows are done with: their space becomes the record
        double* const red = sh;
        for (int w = 0; w < SWEEP_WAVES; ++w) {     // wavefront 0, 1, 2, 3 in turn (fixed order)
            if (wv == w && lane < T) {
#pragma unroll
                for (int i = 0; i < RLT_SWEEP_COLS; ++i) red[i * 64 + lane] = w ? red[i * 64 + lane] + acc[i] : acc[i];
            }
            __syncthreads();
        }
        const int ncol = RLT_SWEEP_COLS * T;
        for (int i = tid; i < ncol; i += 256) a.records[(size_t)blockIdx.x * ncol + i] = red[(i / T) * 64 + i % T];
    }
}

// column sums of the records in a fixed order (as cut_report_final_kernel) into curve (RLT_SWEEP_COLS, T)
__global__ __launch_bounds__(256) void cut_sweep_final_kernel(const double* __restrict__ rec, int rows, int ncol, int accumulate,
                                                              double* __restrict__ curve) {
    __shared__ double part[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
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
        curve[col] = accumulate ? curve[col] + acc : acc;
    }
}

int sweep_grid(int B) {
    const int groups = rlt_cdiv(B, SWEEP_WAVES);
    return groups < SWEEP_MAX_GRID ? groups : SWEEP_MAX_GRID;
}

size_t sweep_lds(int S) {
    const size_t rows = (size_t)SWEEP_WAVES * rlt_cdiv(S, 64) * 64 * (sizeof(double) + sizeof(int));
    const size_t record = (size_t)RLT_SWEEP_COLS * 64 * sizeof(double);
    return rows > record ? rows : record;
}

template <int R>
void launch_sweep(const SweepArgs& a, bool labels, int grid, hipStream_t st) {
    if (labels) hipLaunchKernelGGL((cut_sweep_kernel<R, true>), dim3(grid), dim3(256), sweep_lds(a.S), st, a);
    else hipLaunchKernelGGL((cut_sweep_kernel<R, false>), dim3(grid), dim3(256), 0, st, a);
}

void dispatch_sweep(const SweepArgs& a, bool labels, int grid, hipStream_t st) {
    switch (rlt_cdiv(a.S, 64)) {
        case 1: return launch_sweep<1>(a, labels, grid, st);
        case 2: return launch_sweep<2>(a, labels, grid, st);
        case 3: return launch_sweep<3>(a, labels, grid, st);
        case 4: return launch_sweep<4>(a, labels, grid, st);
        case 5: return launch_sweep<5>(a, labels, grid, st);
        case 6: return launch_sweep<6>(a, labels, grid, st);
        case 7: return launch_sweep<7>(a, labels, grid, st);
        case 8: return launch_sweep<8>(a, labels, grid, st);
        case 9: return launch_sweep<9>(a, labels, grid, st);
        case 10: return launch_sweep<10>(a, labels, grid, st);
        case 11: return launch_sweep<11>(a, labels, grid, st);
        case 12: return launch_sweep<12>(a, labels, grid, st);
        case 13: return launch_sweep<13>(a, labels, grid, st);
        case 14: return launch_sweep<14>(a, labels, grid, st);
        case 15: return launch_sweep<15>(a, labels, grid, st);
        default: return launch_sweep<16>(a, labels, grid, st);
    }
}

}  // namespace

extern "C" {

size_t rlt_cut_sweep_workspace(int B, int S, int T) {
    if (B <= 0 || S <= 0 || S > SWEEP_MAX_S || T <= 0 || T > SWEEP_MAX_T) return 0;
    return ((size_t)sweep_grid(B) * RLT_SWEEP_COLS * T * sizeof(double) + 15) / 16 * 16;
}

int rlt_cut_sweep(const float* v, int v_stride, int rule, const double* thresholds, int T, const float* labels, int B, int S,
                  double metric_penalty, double beta, const void* dcg_table, int accumulate, int32_t* k, double* curve,
                  void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(v && thresholds && B > 0 && S > 0 && T > 0);
    RLT_CHECK_ARG(rule == RLT_SWEEP_QUANTILE || rule == RLT_SWEEP_FIRST_BELOW || rule == RLT_SWEEP_FIRST_ABOVE);
    RLT_CHECK_ARG(v_stride == 1 || v_stride == 2);
    RLT_CHECK_ARG(k || curve);
    RLT_CHECK_ARG(!curve || (labels && dcg_table && ws));
    RLT_CHECK_SHAPE(S <= SWEEP_MAX_S && T <= SWEEP_MAX_T);
    if ((((uintptr_t)thresholds | (uintptr_t)curve) & 7u) != 0 || (((uintptr_t)v | (uintptr_t)labels | (uintptr_t)k) & 3u) != 0)
        return RLT_E_ALIGN;
    if (curve) {
        if ((((uintptr_t)dcg_table | (uintptr_t)ws) & 7u) != 0) return RLT_E_ALIGN;
        if (ws_bytes < rlt_cut_sweep_workspace(B, S, T)) return RLT_E_WORKSPACE;
    }
    const int grid = sweep_grid(B);
    const SweepArgs a{v, labels, thresholds, (const double*)dcg_table, B, S, T, v_stride, rule, metric_penalty, beta * beta,
                      k, (double*)ws};
    hipStream_t st = rlt_stream(stream);
    dispatch_sweep(a, curve != nullptr, grid, st);      // labels without a curve: only the cuts are asked for
    if (curve)
        hipLaunchKernelGGL(cut_sweep_final_kernel, dim3(rlt_cdiv(RLT_SWEEP_COLS * T, 16)), dim3(256), 0, st, (const double*)ws, grid,
                           RLT_SWEEP_COLS * T, accumulate ? 1 : 0, curve);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
