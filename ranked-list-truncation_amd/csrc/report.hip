// Cut report: what a trained model does with every list of a split, and the two curves behind the reference's `--draw`
// figure (run.py:242-298), from one pass over the model's output p and - when there are any - the labels.
//
// Per list: the cut k (RLT_CUT_ARGMAX: first maximum + 1, run.py:141-142; RLT_CUT_PAIR: BiCut's rule, run.py:131-136), the
// winning value and its margin; with labels F1@k / DCG@k (rlt_cut_metrics_ex, bit for bit), the list's best F1 / DCG over
// k = 0..S (rlt_truncation_curves, bit for bit) and `better`, the number of cut positions whose reward - the fp32 reward of
// rlt_reward_matrix_ex, bit for bit - is strictly greater than the reward at k.  Per split: the histogram of k, the sum over
// lists of softmax_j(p_j / sharpen) and of softmax_j(r_j / tau), and the sums of the four per-list metrics.
//
// Both softmaxes subtract the row maximum and work in float64.  The reference forms exp(p / 9e-4) in fp32 without the
// subtraction, which overflows once a p exceeds about 0.08 and then draws NaN; where the reference is finite the two agree to
// its own fp32 rounding, elsewhere this pass stays finite.  The `norm_s[-3:] = norm_s[-4]` overwrite of run.py:283 is
// presentation and is left to the caller (utils/report.py).
//
// Layout as in baselines.hip: a wavefront owns whole lists - four per wavefront, one per row of 16 lanes, at S <= 64 -
// position j sits in lane j % L of round j / L, and the per-position sums (histogram, prediction curve, reward curve) stay in
// registers.  The bit-for-bit contracts fix the summation orders:
//   * DCG@k repeats rlt_cut_metrics' order (lane-strided partial sums, then the 64-lane scan; at S <= 64 a list's rounds are the
//     rows of that scan, so the four row totals are combined as the scan combines them);
//   * the fp32 DCG reward repeats the reward kernel's order: a lane owns C consecutive positions (C as that kernel picks it),
//     so at S > 64 the labels are turned through the wavefront's own LDS rows and the reward curve is accumulated in that
//     layout; at S <= 64 (C = 1) the scan's row structure is again the list's rounds;
//   * the sums of F1@k and DCG@k repeat rlt_cut_metrics' single-workgroup order over the per-list values, which the pass keeps
//     in the workspace.
// Everything else goes through one float64 record per workgroup and a fixed-order column reduction.  No atomics, no
// allocation, no host synchronisation: the same inputs give bitwise identical outputs.
//
// Algorithmic bytes: 8 S per list read (4 S without labels, 12 S under the PAIR rule) + up to 60 B of per-list results.
#include "common.h"

namespace {

constexpr int REPORT_MAX_S = 1024;
constexpr int REPORT_WAVES = 4;
constexpr int REPORT_MAX_GRID = 1024;

__host__ __device__ constexpr int report_cols(int S) { return 3 * S + 2; }   // k counts, prediction, reward (S each), sum best F1, sum best DCG
// positions per lane of the reward kernel's general form (loss.hip, dispatch_reward_m) for ceil(S / 64) = R
__host__ __device__ constexpr int report_chunk(int R) { return R <= 6 ? R : R <= 8 ? 8 : R <= 12 ? 12 : 16; }

struct ReportArgs {
    const float* p;         // (B, S) or (B, S, 2)
    const float* y;         // (B, S) or null
    const float* coef;      // (S) fp32 log2(j + 2): the reward kernel's coefficients (DCG reward)
    const double* tab;      // DCG table
    int B, S, rule, metric;
    float penalty;          // reward curve
    double mpenalty;        // DCG@k, best DCG
    double tau, sharpen;
    int32_t* k;
    float* p_k;
    float* margin;
    double* f1;
    double* dcg;
    double* best_f1;
    int32_t* best_f1_k;
    double* best_dcg;
    int32_t* best_dcg_k;
    int32_t* better;
    double* ws_f1;          // (B) workspace copies for the ordered sums
    double* ws_dcg;
    double* records;        // (grid, report_cols(S))
};

// the tail every reward layout shares: the reward at the cut, the count of better cuts and softmax_j(r_j / tau) in float64 added
// into the lane's per-position sums.  Element i of the lane is position j0 + i * jstep.
template <int L, int NV>
__device__ __forceinline__ int reward_tail(const float (&rv)[NV], int j0, int jstep, bool live, int S, int k, double tau,
                                           double (&rc)[NV], int lane) {
    const auto fmx = [](float x, float z) { return x > z ? x : z; };
    const auto iadd = [](int x, int z) { return x + z; };
    const auto dadd = [](double x, double z) { return x + z; };
    float rk_l = -INFINITY, mx_l = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = j0 + i * jstep;
        if (j < S) {
            mx_l = fmx(mx_l, rv[i]);
            if (j == k - 1) rk_l = rv[i];
        }
    }
    const float rk = rlt_group_reduce<L>(rk_l, -INFINITY, fmx, lane);
    const float mx = rlt_group_reduce<L>(mx_l, -INFINITY, fmx, lane);
    const double xm = (double)mx / tau;
    int cnt = 0;
    double e[NV], z_l = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = j0 + i * jstep;
        const bool ok = j < S;
        cnt += (ok && rv[i] > rk) ? 1 : 0;
        e[i] = ok ? exp((double)rv[i] / tau - xm) : 0.0;
        z_l += e[i];
    }
    const double z = rlt_group_reduce<L>(z_l, 0.0, dadd, lane);
    if (live) {
#pragma unroll
        for (int i = 0; i < NV; ++i) rc[i] += e[i] / z;
    }
    return rlt_group_reduce<L>(cnt, 0, iadd, lane);
}

template <int L, int R, bool LABELS>
__global__ __launch_bounds__(256) void cut_report_kernel(ReportArgs a) {
    constexpr int G = 64 / L;                       // lists per wavefront
    constexpr int C = L == 64 ? report_chunk(R) : 1;        // reward layout: positions per lane
    constexpr int NR = L == 64 ? C : R;             // reward values per lane
    constexpr int STRIDE = C | 1;
    extern __shared__ double sh[];                  // tables q1, qp, cf (S each; LABELS), then the record; then the wavefronts' label rows
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane / L, l = lane % L;
    const int S = a.S;
    const bool pair = a.rule == RLT_CUT_PAIR;
    double* const q1 = sh;                          // 1 / log2(j + 2) and mpenalty / log2(j + 2): rlt_cut_metrics' gains
    double* const qp = sh + S;
    double* const cf = sh + 2 * S;                  // the table's coefficients: rlt_truncation_curves' gains
    float* const wy = reinterpret_cast<float*>(sh + report_cols(S)) + wv * (64 * STRIDE);
    if constexpr (LABELS) {
        for (int j = tid; j < S; j += 256) {
            const double lg = log2((double)(j + 2));
            q1[j] = 1.0 / lg;
            qp[j] = a.mpenalty / lg;
            cf[j] = a.tab[j];
        }
        __syncthreads();
    }
    const auto dadd = [](double x, double z) { return x + z; };
    const auto fmx = [](float x, float z) { return x > z ? x : z; };
    const auto imn = [](int x, int z) { return x < z ? x : z; };
    int hc[R];
    double pc[R], rc[NR];
    float icf[NR];                                  // the reward kernel's 1 / log2(j + 2): v_rcp_f32 of the caller's fp32 coefficients
#pragma unroll
    for (int r = 0; r < R; ++r) { hc[r] = 0; pc[r] = 0.0; }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        rc[i] = 0.0;
        const int j = L == 64 ? lane * C + i : i * L + l;
        icf[i] = (LABELS && a.metric == RLT_METRIC_DCG && j < S) ? __builtin_amdgcn_rcpf(a.coef[j]) : 0.f;
    }
    double sum_bf = 0.0, sum_bd = 0.0;
    const long long waves = (long long)gridDim.x * REPORT_WAVES;
    for (long long w = (long long)blockIdx.x * REPORT_WAVES + wv; w * G < a.B; w += waves) {
        const long long b = w * G + grp;
        const bool live = b < a.B;
        const size_t base = (size_t)(live ? b : 0) * S;
        float pv[R], gv[R], yv[R];                  // prediction (class 0 under PAIR), class gap (PAIR), labels
        unsigned cls0 = 0u;                         // PAIR: bit r = this lane's position of round r prefers class 0 (ties included)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = r * L + l;
            const bool valid = live && j < S;
            pv[r] = gv[r] = yv[r] = 0.f;
            if (valid) {
                if (pair) {
                    const float2 t = *reinterpret_cast<const float2*>(a.p + 2 * (base + j));
                    pv[r] = t.x;
                    gv[r] = t.x - t.y;
                    cls0 |= (t.y > t.x) ? 0u : (1u << r);
                } else {
                    pv[r] = a.p[base + j];
                }
                if constexpr (LABELS) yv[r] = a.y[base + j];
            }
        }
        // ---- the cut ----------------------------------------------------------------------------------------------
        float m1 = -INFINITY, m2 = -INFINITY;       // this lane's largest value and its runner-up
        int bi = 0x7fffffff, fi = 0x7fffffff;       // first maximum / first position that prefers class 0 (t.x >= t.y)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = r * L + l;
            if (live && j < S) {
                const float v = pv[r];
                if (v > m1) { m2 = m1; m1 = v; bi = j; }
                else if (v > m2) m2 = v;
                if (((cls0 >> r) & 1u) && fi == 0x7fffffff) fi = j;
            }
        }
        const float pmax = rlt_group_reduce<L>(m1, -INFINITY, fmx, lane);
        int k;
        float runner = 0.f;
        if (pair) {
            const int f = rlt_group_reduce<L>(fi, 0x7fffffff, imn, lane);
            k = f == 0x7fffffff ? S : f + 1;
        } else {
            const int f = rlt_group_reduce<L>(m1 == pmax ? bi : 0x7fffffff, 0x7fffffff, imn, lane);
            k = (f == 0x7fffffff ? 0 : f) + 1;
            runner = rlt_group_reduce<L>((k - 1) % L == l ? m2 : m1, -INFINITY, fmx, lane);
        }
        // ---- per-list results of the cut, the histogram and softmax_j(p_j / sharpen) ---------------------------------
        const double xm = (double)pmax / a.sharpen;
        double e[R], z_l = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = r * L + l;
            const bool valid = live && j < S;
            e[r] = valid ? exp((double)pv[r] / a.sharpen - xm) : 0.0;
            z_l += e[r];
            if (valid && j == k - 1) {
                hc[r] += 1;
                if (a.k) a.k[b] = k;
                if (a.p_k) a.p_k[b] = pv[r];
                if (a.margin) a.margin[b] = pair ? gv[r] : (S > 1 ? pv[r] - runner : 0.f);
            }
        }
        const double z = rlt_group_reduce<L>(z_l, 0.0, dadd, lane);
        if (live) {
#pragma unroll
            for (int r = 0; r < R; ++r) pc[r] += e[r] / z;
        }
        if constexpr (LABELS) {
            // ---- rlt_truncation_curves' scan: best F1 / DCG over k = 0..S; rlt_cut_metrics' sums at k -----------------
            double n_lane = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) n_lane += (double)yv[r];
            const double N = rlt_group_reduce<L>(n_lane, 0.0, dadd, lane);
            double c_carry = 0.0, d_carry = 0.0, bf = 0.0, bd = 0.0;
            int kf = 0, kd = 0;
            double hk_l = 0.0, dk_l = 0.0, dk_t[R];
            float cpre[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = r * L + l;
                const bool valid = live && j < S;
                const double gain = valid ? ((yv[r] == 1.f) ? 1.0 : a.mpenalty) * cf[j] : 0.0;
                const double ci = rlt_group_scan<L>((double)yv[r], 0.0, dadd);
                const double di = rlt_group_scan<L>(gain, 0.0, dadd);
                const double c = c_carry + ci, dcg = d_carry + di;
                if (r + 1 < R) {
                    c_carry += rlt_group_last<L>(ci, lane);
                    d_carry += rlt_group_last<L>(di, lane);
                }
                cpre[r] = (float)c;
                const double pr = c / (double)(j + 1);
                const double rcl = (N != 0.0) ? c / N : 0.0;
                const double f1 = (pr + rcl != 0.0) ? 2.0 * pr * rcl / (pr + rcl) : 0.0;
                if (valid) {
                    if (f1 > bf) { bf = f1; kf = j + 1; }
                    if (dcg > bd) { bd = dcg; kd = j + 1; }
                }
                const bool in = valid && j < k;
                const double gk = in ? ((yv[r] == 1.f) ? q1[j] : qp[j]) : 0.0;
                hk_l += in ? (double)yv[r] : 0.0;
                if constexpr (L == 64) dk_l += gk;
                else dk_t[r] = rlt_group_reduce<L>(gk, 0.0, dadd, lane);       // one row of rlt_cut_metrics' 64-lane scan
            }
            const auto dmx = [](double x, double z) { return x > z ? x : z; };
            const double mf = rlt_group_reduce<L>(bf, 0.0, dmx, lane), md = rlt_group_reduce<L>(bd, 0.0, dmx, lane);
            const int kfm = rlt_group_reduce<L>(bf == mf ? kf : 0x7fffffff, 0x7fffffff, imn, lane);
            const int kdm = rlt_group_reduce<L>(bd == md ? kd : 0x7fffffff, 0x7fffffff, imn, lane);
            const double hits = rlt_group_reduce<L>(hk_l, 0.0, dadd, lane);
            double dcgk;
            if constexpr (L == 64) {
                dcgk = rlt_group_reduce<L>(dk_l, 0.0, dadd, lane);
            } else {                                // rows 0..3 of the scan: (t3 + t2) + (t1 + t0), absent rows 0
                const double t0 = dk_t[0], t1 = R > 1 ? dk_t[R > 1 ? 1 : 0] : 0.0, t2 = R > 2 ? dk_t[R > 2 ? 2 : 0] : 0.0,
                             t3 = R > 3 ? dk_t[R > 3 ? 3 : 0] : 0.0;
                dcgk = (t3 + t2) + (t1 + t0);
            }
            const double prec = hits / (double)k;
            const double rec = (N != 0.0) ? hits / N : 0.0;
            const double f1k = (prec + rec != 0.0) ? 2.0 * prec * rec / (prec + rec) : 0.0;
            // ---- the fp32 reward of rlt_reward_matrix_ex and its softmax ------------------------------------------------
            float rv[NR];
            const float nf = (float)N;
            if constexpr (L == 64) {
                // a lane owns C consecutive positions, as in the reward kernel: the labels turn through this wavefront's LDS rows
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int j = r * 64 + lane;
                    if (j < 64 * C) wy[(j / C) * STRIDE + j % C] = yv[r];
                }
                if constexpr (C > R) {
#pragma unroll
                    for (int r = R; r < C; ++r) {
                        const int j = r * 64 + lane;
                        wy[(j / C) * STRIDE + j % C] = 0.f;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                float yc[C], pre[C], run = 0.f;
#pragma unroll
                for (int i = 0; i < C; ++i) yc[i] = wy[lane * STRIDE + i];
                __builtin_amdgcn_wave_barrier();    // the next list's stores come after these loads
                if (a.metric == RLT_METRIC_F1) {
#pragma unroll
                    for (int i = 0; i < C; ++i) { run += yc[i]; pre[i] = run; }
                    const float incl = wave_scan_incl(run, lane);
                    const float excl = incl - run;
                    const float n_rel = rlt_readlane(incl, 63);
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const float h = excl + pre[i];
                        const float kk = (float)(lane * C + i + 1);
                        rv[i] = (h > 0.f) ? (2.f * h) * __builtin_amdgcn_rcpf(kk + n_rel) : 0.f;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        float g = 0.f;
                        if (lane * C + i < S) g = (yc[i] == 1.f) ? icf[i] : icf[i] * a.penalty;
                        run += g;
                        pre[i] = run;
                    }
                    const float incl = wave_scan_incl(run, lane);
                    const float excl = incl - run;
#pragma unroll
                    for (int i = 0; i < C; ++i) rv[i] = excl + pre[i];
                }
            } else {
                // C = 1: position j is lane j of the reward kernel's 64-lane scan, i.e. row r = j / 16 of it
                if (a.metric == RLT_METRIC_F1) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float h = cpre[r];
                        rv[r] = (h > 0.f) ? (2.f * h) * __builtin_amdgcn_rcpf((float)(r * L + l + 1) + nf) : 0.f;
                    }
                } else {
                    const auto fadd = [](float x, float z) { return x + z; };
                    float g[R], s[R], t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int j = r * L + l;
                        g[r] = (live && j < S) ? ((yv[r] == 1.f) ? icf[r] : icf[r] * a.penalty) : 0.f;
                        s[r] = rlt_group_scan<L>(g[r], 0.f, fadd);
                        t[r] = rlt_group_last<L>(s[r], lane);
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float incl = r == 0 ? s[0] : r == 1 ? s[r] + t[0] : r == 2 ? s[r] + (t[1] + t[0]) : (s[r] + t[2]) + (t[1] + t[0]);
                        rv[r] = (incl - g[r]) + g[r];           // the kernel's excl + pre with one position per lane
                    }
                }
            }
            const int better = reward_tail<L, NR>(rv, L == 64 ? lane * C : l, L == 64 ? 1 : L, live, S, k, a.tau, rc, lane);
            if (live && l == 0) {
                if (a.f1) a.f1[b] = f1k;
                if (a.dcg) a.dcg[b] = dcgk;
                a.ws_f1[b] = f1k;
                a.ws_dcg[b] = dcgk;
                if (a.best_f1) a.best_f1[b] = mf;
                if (a.best_f1_k) a.best_f1_k[b] = kfm;
                if (a.best_dcg) a.best_dcg[b] = md;
                if (a.best_dcg_k) a.best_dcg_k[b] = kdm;
                if (a.better) a.better[b] = better;
                sum_bf += mf;
                sum_bd += md;
            }
        }
    }
    double hd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) hd[r] = (double)hc[r];
    if constexpr (G == 4) {                         // the four rows hold the same positions: (row 0 + row 1) + (row 2 + row 3) into row 0
#pragma unroll
        for (int r = 0; r < R; ++r) {
            hd[r] += __shfl_down(hd[r], 16);
            pc[r] += __shfl_down(pc[r], 16);
            rc[r] += __shfl_down(rc[r], 16);
            hd[r] += __shfl_down(hd[r], 32);
            pc[r] += __shfl_down(pc[r], 32);
            rc[r] += __shfl_down(rc[r], 32);
        }
        sum_bf += __shfl_down(sum_bf, 16);
        sum_bd += __shfl_down(sum_bd, 16);
        sum_bf += __shfl_down(sum_bf, 32);
        sum_bd += __shfl_down(sum_bd, 32);
    }
    __syncthreads();                                // the tables are done with: their space becomes the record
    double* const red = sh;
    for (int w = 0; w < REPORT_WAVES; ++w) {        // wavefront 0, 1, 2, 3 in turn (fixed order)
        if (wv == w) {
            if (lane < L) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int j = r * L + lane;
                    if (j < S) {
                        red[j] = w ? red[j] + hd[r] : hd[r];
                        red[S + j] = w ? red[S + j] + pc[r] : pc[r];
                    }
                }
            }
            if (L == 64 || lane < L) {
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int j = L == 64 ? lane * C + i : i * L + lane;
                    if (j < S) red[2 * S + j] = w ? red[2 * S + j] + rc[i] : rc[i];
                }
            }
            if (lane == 0) {
                red[3 * S] = w ? red[3 * S] + sum_bf : sum_bf;
                red[3 * S + 1] = w ? red[3 * S + 1] + sum_bd : sum_bd;
            }
        }
        __syncthreads();
    }
    const int ncol = report_cols(S);
    for (int i = tid; i < ncol; i += 256) a.records[(size_t)blockIdx.x * ncol + i] = red[i];
}

// column sums of the records in a fixed order (as truncation_curves_final_kernel) into hist[1..S], pred_curve, reward_curve and
// sums[2..3]; hist[0] (no rule cuts at 0) and the list count sums[4] from the arguments
__global__ __launch_bounds__(256) void cut_report_final_kernel(const double* __restrict__ rec, int rows, int S, int B, int labelled,
                                                               int accumulate, double* __restrict__ hist, double* __restrict__ pred,
                                                               double* __restrict__ reward, double* __restrict__ sums) {
    __shared__ double part[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int ncol = report_cols(S);
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
        double* dst = nullptr;
        if (col < S) dst = hist ? hist + col + 1 : nullptr;
        else if (col < 2 * S) dst = pred ? pred + (col - S) : nullptr;
        else if (col < 3 * S) dst = (reward && labelled) ? reward + (col - 2 * S) : nullptr;
        else dst = (sums && labelled) ? sums + 2 + (col - 3 * S) : nullptr;
        if (dst) *dst = accumulate ? *dst + acc : acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (hist && !accumulate) hist[0] = 0.0;
        if (sums && !accumulate && !labelled) sums[0] = sums[1] = sums[2] = sums[3] = 0.0;
        if (sums) sums[4] = (accumulate ? sums[4] : 0.0) + (double)B;
    }
}

// sums[0..1] = the sums of the per-list F1@k and DCG@k in the order of rlt_cut_metrics' own reduction: thread t of one workgroup
// adds lists t, t + 256, ... in turn, then the halving tree over the threads
__global__ __launch_bounds__(256) void cut_report_sum_kernel(const double* __restrict__ f1, const double* __restrict__ dcg, int n,
                                                             int accumulate, double* __restrict__ sums) {
    __shared__ double sa[256], sb[256];
    double x = 0.0, z = 0.0;
    int i = threadIdx.x;
    for (; i + 768 < n; i += 1024) {                // four loads of each in flight, added in list order
        const double x0 = f1[i], x1 = f1[i + 256], x2 = f1[i + 512], x3 = f1[i + 768];
        const double z0 = dcg[i], z1 = dcg[i + 256], z2 = dcg[i + 512], z3 = dcg[i + 768];
        x += x0; x += x1; x += x2; x += x3;
        z += z0; z += z1; z += z2; z += z3;
    }
    for (; i < n; i += 256) { x += f1[i]; z += dcg[i]; }
    sa[threadIdx.x] = x;
    sb[threadIdx.x] = z;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] = accumulate ? sums[0] + sa[0] : sa[0];
        sums[1] = accumulate ? sums[1] + sb[0] : sb[0];
    }
}

int report_grid(int B, int S) {
    const int lists_per_wg = REPORT_WAVES * (S <= 64 ? 4 : 1);
    const int groups = rlt_cdiv(B, lists_per_wg);
    return groups < REPORT_MAX_GRID ? groups : REPORT_MAX_GRID;
}

size_t report_lds(int S) {
    const int c = S <= 64 ? 1 : report_chunk(rlt_cdiv(S, 64));
    return (size_t)report_cols(S) * sizeof(double) + (size_t)REPORT_WAVES * 64 * (c | 1) * sizeof(float);
}

template <int L, int R>
void launch_report(const ReportArgs& a, int grid, hipStream_t st) {
    if (a.y) hipLaunchKernelGGL((cut_report_kernel<L, R, true>), dim3(grid), dim3(256), report_lds(a.S), st, a);
    else hipLaunchKernelGGL((cut_report_kernel<L, R, false>), dim3(grid), dim3(256), report_lds(a.S), st, a);
}

void dispatch_report(const ReportArgs& a, int grid, hipStream_t st) {
    if (a.S <= 64) {
        switch (rlt_cdiv(a.S, 16)) {
            case 1: return launch_report<16, 1>(a, grid, st);
            case 2: return launch_report<16, 2>(a, grid, st);
            case 3: return launch_report<16, 3>(a, grid, st);
            default: return launch_report<16, 4>(a, grid, st);
        }
    }
    switch (rlt_cdiv(a.S, 64)) {
        case 2: return launch_report<64, 2>(a, grid, st);
        case 3: return launch_report<64, 3>(a, grid, st);
        case 4: return launch_report<64, 4>(a, grid, st);
        case 5: return launch_report<64, 5>(a, grid, st);
        case 6: return launch_report<64, 6>(a, grid, st);
        case 7: return launch_report<64, 7>(a, grid, st);
        case 8: return launch_report<64, 8>(a, grid, st);
        case 9: return launch_report<64, 9>(a, grid, st);
        case 10: return launch_report<64, 10>(a, grid, st);
        case 11: return launch_report<64, 11>(a, grid, st);
        case 12: return launch_report<64, 12>(a, grid, st);
        case 13: return launch_report<64, 13>(a, grid, st);
        case 14: return launch_report<64, 14>(a, grid, st);
        case 15: return launch_report<64, 15>(a, grid, st);
        default: return launch_report<64, 16>(a, grid, st);
    }
}

size_t report_records_bytes(int B, int S) { return ((size_t)report_grid(B, S) * report_cols(S) * sizeof(double) + 15) / 16 * 16; }

}  // namespace

extern "C" {

size_t rlt_cut_report_workspace(int B, int S) {
    if (B <= 0 || S <= 0 || S > REPORT_MAX_S) return 0;
    return report_records_bytes(B, S) + ((size_t)2 * B * sizeof(double) + 15) / 16 * 16;    // records, then F1@k and DCG@k per list
}

int rlt_cut_report(const float* p, int rule, const float* labels, const float* dcg_coef, int B, int S, int metric, float penalty,
                   double metric_penalty, double tau, double sharpen, const void* dcg_table, int accumulate,
                   int32_t* k, float* p_k, float* margin, double* f1, double* dcg, double* best_f1, int32_t* best_f1_k,
                   double* best_dcg, int32_t* best_dcg_k, int32_t* better, double* hist, double* pred_curve, double* reward_curve,
                   double* sums, void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(p && ws && B > 0 && S > 0);
    RLT_CHECK_ARG(rule == RLT_CUT_ARGMAX || rule == RLT_CUT_PAIR);
    RLT_CHECK_ARG(sharpen > 0.0);
    if (labels) {
        RLT_CHECK_ARG(metric == RLT_METRIC_F1 || metric == RLT_METRIC_DCG);
        RLT_CHECK_ARG(dcg_table && tau > 0.0 && (metric == RLT_METRIC_F1 || dcg_coef));
    } else {
        RLT_CHECK_ARG(!f1 && !dcg && !best_f1 && !best_f1_k && !best_dcg && !best_dcg_k && !better && !reward_curve);
    }
    RLT_CHECK_SHAPE(S <= REPORT_MAX_S);
    if ((((uintptr_t)dcg_table | (uintptr_t)ws | (uintptr_t)hist | (uintptr_t)pred_curve | (uintptr_t)reward_curve |
          (uintptr_t)sums) & 7u) != 0 || ((uintptr_t)p & (rule == RLT_CUT_PAIR ? 7u : 3u)) != 0 || ((uintptr_t)labels & 3u) != 0)
        return RLT_E_ALIGN;
    if (ws_bytes < rlt_cut_report_workspace(B, S)) return RLT_E_WORKSPACE;
    const int grid = report_grid(B, S);
    double* const ws_f1 = reinterpret_cast<double*>((char*)ws + report_records_bytes(B, S));
    ReportArgs a{p, labels, dcg_coef, (const double*)dcg_table, B, S, rule, metric, penalty, metric_penalty, tau, sharpen,
                 k, p_k, margin, f1, dcg, best_f1, best_f1_k, best_dcg, best_dcg_k, better, ws_f1, ws_f1 + B, (double*)ws};
    hipStream_t st = rlt_stream(stream);
    dispatch_report(a, grid, st);
    hipLaunchKernelGGL(cut_report_final_kernel, dim3(rlt_cdiv(report_cols(S), 16)), dim3(256), 0, st, (const double*)ws, grid, S, B,
                       labels ? 1 : 0, accumulate ? 1 : 0, hist, pred_curve, reward_curve, sums);
    if (labels && sums)
        hipLaunchKernelGGL(cut_report_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)ws_f1, (const double*)(ws_f1 + B), B,
                           accumulate ? 1 : 0, sums);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
