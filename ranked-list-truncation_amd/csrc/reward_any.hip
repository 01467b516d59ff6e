// Reward losses for ANY cut reward: a reward spec (F_beta, graded gain / nDCG) built from the labels in registers, or a
// caller-supplied (B,S) reward matrix.  loss.hip knows two rewards, both formed from `label == 1` in fp32; this file makes
// the reward an argument and leaves that one as it is.
//
// The pass is the one of rlt_loss_metrics: a wavefront owns whole lists - four (one per row of 16 lanes), two (one per
// 32-lane half) or one, picked by S and S % 4 exactly as dispatch_reward_m picks them - rows of S % 4 == 0 floats are read
// and written 16 bytes at a time (a lane holds 4 consecutive positions per round), other rows one position per lane and
// round.  The grid is sized to the chip and strides over the lists.  Nothing is turned through LDS: the prefix sums run round
// by round (a serial scan of the lane's own positions, a DPP scan over the list's lanes, the running total of the rounds
// before).
//
// Arithmetic.  The reward is formed in float64 and rounded to fp32 ONCE (rlt_hip.h): integer hit counts and one float64
// division for F_beta, a float64 prefix sum of gain[grade] * discount for the gain family, divided by the list's ideal value
// when the spec normalises.  q = softmax(r / tau) with the row maximum subtracted, the loss terms and d(loss)/dp are float64
// too (the device library's exp and log), rounded to fp32 where they are stored: the outputs are the fp32 neighbours of the
// float64 restatement at every shape, whatever the span of the reward.  That costs vector time (see DESIGN.md section 7 for
// what it measures against rlt_loss_metrics at equal bytes).
//
// Every workgroup leaves ONE float64 record {sum of loss terms, sum r_k, sum r_best, lists cut at their best reward} in ws;
// a one-workgroup launch adds the records in a fixed order.  No atomics, no allocation, no host synchronisation: two calls
// give the same bits.
//
// Algorithmic bytes per list: read p + labels (or p + r) 8 S, write dp 4 S, + up to 20 B of per-list results.
#include "common.h"
#include <cmath>
#include <initializer_list>

namespace {

constexpr int ANY_MAX_S = 1024;
constexpr int ANY_WAVES = 4;
constexpr int ANY_MAX_GRID = 256 * 8;           // as loss.hip: up to 8 workgroups per CU, beyond that the workgroups stride
constexpr int ANY_REC = 4;                      // doubles per workgroup record
constexpr int SRC_FBETA = 0, SRC_GAIN = 1, SRC_MATRIX = 2;

struct AnyArgs {
    const float* p;             // (B,S) or null (rlt_reward_spec_matrix)
    const float* y;             // (B,S) labels, spec sources
    const float* r_in;          // (B,S) reward, matrix source
    const float* disc;          // (S) discounts or null: the table's 1 / log2(j + 2)
    const double* tab;          // DCG table (rlt_dcg_table_init)
    float* loss_per_list;       // (B) or null
    float* dp;                  // (B,S) or null
    float* r_out;               // (B,S) or null
    float* q_out;               // (B,S) or null
    int32_t* k_out;             // (B) or null
    float* r_k;                 // (B) or null
    float* r_best;              // (B) or null
    int32_t* best_k;            // (B) or null
    double* records;            // (grid, ANY_REC) or null
    int B, S, src, kind;
    int n_grades, normalize, n_take;
    int order[RLT_REWARD_MAX_GRADES];     // the grades of positive gain in the order the ideal list takes them
    double gain[RLT_REWARD_MAX_GRADES];
    double beta2, tau, gscale;
};

// inclusive scan over each group of LL lanes (16: a DPP row; 32: a half; 64: the wavefront)
template <int LL, typename T, typename Op>
__device__ __forceinline__ T any_scan(T v, T id, Op op) {
    v = op(v, rlt_dpp<0x111, 0xf>(id, v));
    v = op(v, rlt_dpp<0x112, 0xf>(id, v));
    v = op(v, rlt_dpp<0x114, 0xf>(id, v));
    v = op(v, rlt_dpp<0x118, 0xf>(id, v));
    if (LL >= 32) v = op(v, rlt_dpp<0x142, 0xa>(id, v));      // row_bcast:15 into rows 1 and 3
    if (LL == 64) v = op(v, rlt_dpp<0x143, 0xc>(id, v));      // row_bcast:31 into rows 2 and 3
    return v;
}
// the value of the last lane of the caller's group, in every lane of the group
template <int LL, typename T>
__device__ __forceinline__ T any_last(T v, bool upper) {
    if (LL == 16) return rlt_dpp<0x15F, 0xf>(v, v);           // lane 15 of the row to every lane of the row
    if (LL == 64) return rlt_readlane(v, 63);
    const T lo = rlt_readlane(v, 31), hi = rlt_readlane(v, 63);
    return upper ? hi : lo;
}
template <int LL, typename T, typename Op>
__device__ __forceinline__ T any_reduce(T v, T id, Op op, bool upper) { return any_last<LL>(any_scan<LL>(v, id, op), upper); }

// LL lanes per list, R rounds, V consecutive positions per lane and round (4: 16-byte accesses, S % 4 == 0; 1 otherwise):
// element (r, i) of a lane is position r * V * LL + V * hl + i
template <int LL, int R, int V>
__global__ __launch_bounds__(256) void reward_any_kernel(AnyArgs a) {
    constexpr int N = R * V, PR = V * LL, LPW = 64 / LL;
    __shared__ double sd[ANY_MAX_S];            // d_j
    __shared__ double sD[ANY_MAX_S + 1];        // D[k] = sum_{j<k} d_j
    __shared__ double sg[RLT_REWARD_MAX_GRADES];
    __shared__ double srec[ANY_WAVES][ANY_REC];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool upper = lane >= 32;
    const int hl = lane & (LL - 1), grp = lane / LL;
    const int S = a.S, B = a.B;
    const auto iadd = [](int x, int z) { return x + z; };
    const auto dadd = [](double x, double z) { return x + z; };
    const auto fmx = [](float x, float z) { return x > z ? x : z; };
    const auto imn = [](int x, int z) { return x < z ? x : z; };
    if (a.src == SRC_GAIN) {
        for (int j = tid; j < S; j += 256) sd[j] = a.disc ? (double)a.disc[j] : a.tab[j];
        if (tid < RLT_REWARD_MAX_GRADES) sg[tid] = a.gain[tid];
        if (a.normalize) {
            if (!a.disc) {
                for (int k = tid; k <= S; k += 256) sD[k] = a.tab[ANY_MAX_S + k];
            } else {
                __syncthreads();
                if (tid == 0) {                 // the sums a sequential float64 loop produces
                    double acc = 0.0;
                    sD[0] = 0.0;
                    for (int k = 0; k < S; ++k) { acc += sd[k]; sD[k + 1] = acc; }
                }
            }
        }
        __syncthreads();
    }
    bool ok[R];                                 // rounds before the last lie inside the list when V == 4; V == 1: per round
#pragma unroll
    for (int r = 0; r < R; ++r) ok[r] = r * PR + V * hl < S;
    double part[ANY_REC] = {0.0, 0.0, 0.0, 0.0};
    const int nwaves = gridDim.x * ANY_WAVES;
    for (int pb = LPW * (blockIdx.x * ANY_WAVES + wv); pb < B; pb += LPW * nwaves) {
        const bool live = pb + grp < B;         // lists beyond B: the idle group shadows the first one, stores masked
        const int b = live ? pb + grp : pb;
        const size_t base = (size_t)b * S;
        float p[N], rv[N];
        // ---- load ------------------------------------------------------------------------------------------------
        {
            const float* src = a.src == SRC_MATRIX ? a.r_in : a.y;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t at = base + (ok[r] ? r * PR + V * hl : 0);
                if constexpr (V == 4) {
                    const float4 vy = *reinterpret_cast<const float4*>(src + at);
                    float4 vp = make_float4(1.f, 1.f, 1.f, 1.f);
                    if (a.p) vp = *reinterpret_cast<const float4*>(a.p + at);
                    rv[4 * r] = vy.x; rv[4 * r + 1] = vy.y; rv[4 * r + 2] = vy.z; rv[4 * r + 3] = vy.w;
                    p[4 * r] = vp.x; p[4 * r + 1] = vp.y; p[4 * r + 2] = vp.z; p[4 * r + 3] = vp.w;
                } else {
                    rv[r] = src[at];
                    p[r] = a.p ? a.p[at] : 1.f;
                }
            }
        }
        // ---- the reward r_k, k = j + 1: float64, rounded to fp32 once -----------------------------------------------
        if (a.src == SRC_FBETA) {
            int c[N];
            int off = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                int run = 0;
#pragma unroll
                for (int i = 0; i < V; ++i) { run += (ok[r] && rv[V * r + i] >= 1.f) ? 1 : 0; c[V * r + i] = run; }
                const int incl = any_scan<LL>(run, 0, iadd);
                const int ex = (incl - run) + off;
#pragma unroll
                for (int i = 0; i < V; ++i) c[V * r + i] += ex;
                off += any_last<LL>(incl, upper);
            }
            const double num = 1.0 + a.beta2, bn = a.beta2 * (double)off;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const int k = r * PR + V * hl + i + 1;
                    rv[V * r + i] = c[V * r + i] > 0 ? (float)(num * (double)c[V * r + i] / (bn + (double)k)) : 0.f;
                }
        } else if (a.src == SRC_GAIN) {
            int g[N];
            const float gmax = (float)(a.n_grades - 1);
#pragma unroll
            for (int n = 0; n < N; ++n) g[n] = (int)fminf(fmaxf(rintf(rv[n]), 0.f), gmax);     // NaN: fmaxf gives 0
            double inv = 1.0;
            bool zero = false;
            if (a.normalize) {
                double ideal = 0.0;
                int at = 0;
                for (int t = 0; t < a.n_take; ++t) {
                    const int gr = a.order[t];
                    int cnt = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int i = 0; i < V; ++i) cnt += (ok[r] && g[V * r + i] == gr) ? 1 : 0;
                    cnt = any_reduce<LL>(cnt, 0, iadd, upper);
                    ideal += sg[gr] * (sD[at + cnt] - sD[at]);
                    at += cnt;
                }
                zero = !(ideal > 0.0);
                inv = ideal;
            }
            double off = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double cum[V];
                double run = 0.0;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    run += ok[r] ? sg[g[V * r + i]] * sd[r * PR + V * hl + i] : 0.0;
                    cum[i] = run;
                }
                const double incl = any_scan<LL>(run, 0.0, dadd);
                const double ex = (incl - run) + off;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const double v = ex + cum[i];
                    rv[V * r + i] = a.normalize ? (zero ? 0.f : (float)(v / inv)) : (float)v;
                }
                off += any_last<LL>(incl, upper);
            }
        }
        // ---- the row's best reward and the cut -------------------------------------------------------------------------
        float mx_l = -INFINITY, pm_l = -INFINITY;
        int bi = 0x7fffffff, pi = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int j = r * PR + V * hl + i;
                if (ok[r]) {
                    if (rv[V * r + i] > mx_l) { mx_l = rv[V * r + i]; bi = j; }
                    if (p[V * r + i] > pm_l) { pm_l = p[V * r + i]; pi = j; }
                }
            }
        const float mx = any_reduce<LL>(mx_l, -INFINITY, fmx, upper);
        const int bk = any_reduce<LL>(mx_l == mx ? bi : 0x7fffffff, 0x7fffffff, imn, upper);
        const int best_k = (bk == 0x7fffffff ? 0 : bk) + 1;
        int k = 1;
        float rk = mx;
        if (a.p) {
            const float pm = any_reduce<LL>(pm_l, -INFINITY, fmx, upper);
            const int pk = any_reduce<LL>(pm_l == pm ? pi : 0x7fffffff, 0x7fffffff, imn, upper);
            k = (pk == 0x7fffffff ? 0 : pk) + 1;
            float rk_l = -INFINITY;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (ok[r] && r * PR + V * hl + i == k - 1) rk_l = rv[V * r + i];
            rk = any_reduce<LL>(rk_l, -INFINITY, fmx, upper);
        }
        // ---- q = softmax(r / tau), the row maximum subtracted ------------------------------------------------------------
        double e[N];
        double lz = 0.0, iz = 0.0;
        const bool need_q = a.q_out || (a.p && a.kind != RLT_LOSS_EXPECT);
        if (need_q) {
            double z_l = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    e[V * r + i] = ok[r] ? exp(((double)rv[V * r + i] - (double)mx) / a.tau) : 0.0;
                    z_l += e[V * r + i];
                }
            const double z = any_reduce<LL>(z_l, 0.0, dadd, upper);
            iz = 1.0 / z;
            lz = log(z);
        }
        // ---- loss terms and d(loss)/dp ---------------------------------------------------------------------------------
        if (a.p) {
            float dpv[N];
            double t_l = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const int n = V * r + i;
                    const double pd = (double)p[n], rd = (double)rv[n];
                    double term, g;
                    if (a.kind == RLT_LOSS_EXPECT) {
                        term = -(pd * rd);
                        g = -rd;
                    } else {
                        const double q = e[n] * iz;
                        const double lq = (rd - (double)mx) / a.tau - lz;          // ln q from the exponent it was formed with
                        const double lp = log(pd);
                        if (a.kind == RLT_LOSS_CE) {
                            term = q > 0.0 ? -(q * lp) : 0.0;
                            g = -q / pd;
                        } else if (a.kind == RLT_LOSS_KL) {
                            term = q > 0.0 ? q * lq - q * lp : 0.0;
                            g = -q / pd;
                        } else {                              // JS: the gradient flows through ln m AND the target p
                            const double lm = log((pd + q) * 0.5);
                            term = 0.5 * ((q > 0.0 ? q * lq - q * lm : 0.0) + (pd > 0.0 ? pd * lp - pd * lm : 0.0));
                            g = 0.5 * (lp - lm);
                        }
                    }
                    t_l += ok[r] ? term : 0.0;
                    dpv[n] = (float)(g * a.gscale);
                }
            const double tot = any_reduce<LL>(t_l, 0.0, dadd, upper);
            if (live && hl == 0) {
                if (a.loss_per_list) a.loss_per_list[b] = (float)tot;
                if (a.k_out) a.k_out[b] = k;
                if (a.r_k) a.r_k[b] = rk;
                if (a.r_best) a.r_best[b] = mx;
                if (a.best_k) a.best_k[b] = best_k;
                part[0] += tot;
                part[1] += (double)rk;
                part[2] += (double)mx;
                part[3] += rk == mx ? 1.0 : 0.0;
            }
            if (a.dp) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (live && ok[r]) {
                        float* dst = a.dp + base + r * PR + V * hl;
                        if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(dpv[4 * r], dpv[4 * r + 1], dpv[4 * r + 2], dpv[4 * r + 3]);
                        else *dst = dpv[r];
                    }
            }
        }
        // ---- the matrices themselves (rlt_reward_spec_matrix) -----------------------------------------------------------
        if (a.r_out || a.q_out) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (live && ok[r]) {
                    const size_t at = base + r * PR + V * hl;
                    if constexpr (V == 4) {
                        if (a.r_out) *reinterpret_cast<float4*>(a.r_out + at) = make_float4(rv[4 * r], rv[4 * r + 1], rv[4 * r + 2], rv[4 * r + 3]);
                        if (a.q_out)
                            *reinterpret_cast<float4*>(a.q_out + at) = make_float4((float)(e[4 * r] * iz), (float)(e[4 * r + 1] * iz),
                                                                                   (float)(e[4 * r + 2] * iz), (float)(e[4 * r + 3] * iz));
                    } else {
                        if (a.r_out) a.r_out[at] = rv[r];
                        if (a.q_out) a.q_out[at] = (float)(e[r] * iz);
                    }
                }
        }
    }
    // ---- one record per workgroup: the groups of a wavefront in lane order, then the wavefronts in turn ------------------
    if (a.records) {
#pragma unroll
        for (int c = 0; c < ANY_REC; ++c) {
            double t = rlt_readlane(part[c], 0);
            if (LL == 16) t += rlt_readlane(part[c], 16);
            if (LL <= 32) t += rlt_readlane(part[c], 32);
            if (LL == 16) t += rlt_readlane(part[c], 48);
            if (lane == 0) srec[wv][c] = t;
        }
        __syncthreads();
        if (tid < ANY_REC)
            a.records[(size_t)blockIdx.x * ANY_REC + tid] = ((srec[0][tid] + srec[1][tid]) + srec[2][tid]) + srec[3][tid];
    }
}

// the records in a fixed order: thread t adds records t, t + 256, ... in turn, then the halving tree over the threads
__global__ __launch_bounds__(256) void reward_any_final_kernel(const double* __restrict__ rec, int n, double B,
                                                               float* __restrict__ loss_out, double* __restrict__ sums) {
    __shared__ double sm[ANY_REC][256];
    double v[ANY_REC] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
        for (int c = 0; c < ANY_REC; ++c) v[c] += rec[(size_t)i * ANY_REC + c];
    for (int c = 0; c < ANY_REC; ++c) sm[c][threadIdx.x] = v[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int c = 0; c < ANY_REC; ++c) sm[c][threadIdx.x] += sm[c][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (loss_out) loss_out[0] = (float)(sm[0][0] / B);
        if (sums) { sums[0] = sm[1][0]; sums[1] = sm[2][0]; sums[2] = sm[3][0]; sums[3] = B; }
    }
}

// lanes per list, as dispatch_reward_m of loss.hip picks them: S % 4 == 0 and S <= 384: four lists per wavefront where rounds
// of 64 positions waste fewer lane slots than rounds of 128 (an odd number of them, up to five), two otherwise; one list per
// wavefront beyond that and for every S % 4 != 0
int any_lanes(int S) {
    if ((S & 3) != 0 || S > 384) return 64;
    const int r16 = rlt_cdiv(S, 64);
    return ((r16 & 1) && r16 <= 5) ? 16 : 32;
}
int any_grid(int B, int S) {
    const int groups = rlt_cdiv(B, ANY_WAVES * (64 / any_lanes(S)));
    return groups < ANY_MAX_GRID ? groups : ANY_MAX_GRID;
}

template <int LL, int R, int V>
void launch_any(const AnyArgs& a, int grid, hipStream_t st) {
    hipLaunchKernelGGL((reward_any_kernel<LL, R, V>), dim3(grid), dim3(256), 0, st, a);
}

void dispatch_any(const AnyArgs& a, int grid, hipStream_t st) {
    const int S = a.S;
    if ((S & 3) == 0) {
        const int ll = any_lanes(S);
        if (ll == 16) {
            switch (rlt_cdiv(S, 64)) {
                case 1: return launch_any<16, 1, 4>(a, grid, st);
                case 3: return launch_any<16, 3, 4>(a, grid, st);
                default: return launch_any<16, 5, 4>(a, grid, st);
            }
        }
        if (ll == 32) {
            switch (rlt_cdiv(S, 128)) {
                case 1: return launch_any<32, 1, 4>(a, grid, st);
                case 2: return launch_any<32, 2, 4>(a, grid, st);
                default: return launch_any<32, 3, 4>(a, grid, st);
            }
        }
        switch (rlt_cdiv(S, 256)) {
            case 2: return launch_any<64, 2, 4>(a, grid, st);
            case 3: return launch_any<64, 3, 4>(a, grid, st);
            default: return launch_any<64, 4, 4>(a, grid, st);
        }
    }
    const int c = rlt_cdiv(S, 64);              // the chunk sizes of the general reward kernel
    if (c <= 1) return launch_any<64, 1, 1>(a, grid, st);
    if (c <= 2) return launch_any<64, 2, 1>(a, grid, st);
    if (c <= 3) return launch_any<64, 3, 1>(a, grid, st);
    if (c <= 4) return launch_any<64, 4, 1>(a, grid, st);
    if (c <= 5) return launch_any<64, 5, 1>(a, grid, st);
    if (c <= 6) return launch_any<64, 6, 1>(a, grid, st);
    if (c <= 8) return launch_any<64, 8, 1>(a, grid, st);
    if (c <= 12) return launch_any<64, 12, 1>(a, grid, st);
    return launch_any<64, 16, 1>(a, grid, st);
}

// spec -> the kernel's arguments; RLT_E_ARG for a spec outside rlt_hip.h's ranges
int any_spec(const rlt_reward_spec* spec, const void* dcg_table, AnyArgs& a) {
    RLT_CHECK_ARG(spec);
    RLT_CHECK_ARG(spec->family == RLT_REWARD_FBETA || spec->family == RLT_REWARD_GAIN);
    if (spec->family == RLT_REWARD_FBETA) {
        RLT_CHECK_ARG(spec->beta > 0.f && std::isfinite(spec->beta));
        a.src = SRC_FBETA;
        a.beta2 = (double)spec->beta * (double)spec->beta;
        return 0;
    }
    RLT_CHECK_ARG(spec->n_grades >= 2 && spec->n_grades <= RLT_REWARD_MAX_GRADES);
    RLT_CHECK_ARG(spec->discount || dcg_table);
    if (!spec->discount && ((uintptr_t)dcg_table & 7u) != 0) return RLT_E_ALIGN;
    if (((uintptr_t)spec->discount & 3u) != 0) return RLT_E_ALIGN;
    a.src = SRC_GAIN;
    a.n_grades = spec->n_grades;
    a.normalize = spec->normalize ? 1 : 0;
    a.disc = spec->discount;
    a.tab = (const double*)dcg_table;
    a.n_take = 0;
    for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) {
        RLT_CHECK_ARG(g >= spec->n_grades || std::isfinite(spec->gain[g]));
        a.gain[g] = g < spec->n_grades ? (double)spec->gain[g] : 0.0;
    }
    // descending gain, ties: the higher grade first (insertion from the highest grade down keeps that order)
    for (int g = spec->n_grades - 1; g >= 0; --g) {
        if (!(spec->gain[g] > 0.f)) continue;
        int at = a.n_take++;
        while (at > 0 && spec->gain[a.order[at - 1]] < spec->gain[g]) { a.order[at] = a.order[at - 1]; --at; }
        a.order[at] = g;
    }
    return 0;
}

int any_rows_aligned(int S, std::initializer_list<const float*> rows) {
    const uintptr_t mask = (S & 3) == 0 ? 15u : 3u;
    for (const float* r : rows)
        if (r && ((uintptr_t)r & mask) != 0) return RLT_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" {

size_t rlt_reward_any_workspace(int B) {
    if (B <= 0) return 0;
    const int groups = rlt_cdiv(B, ANY_WAVES);                  // the largest grid of any layout
    return (size_t)(groups < ANY_MAX_GRID ? groups : ANY_MAX_GRID) * ANY_REC * sizeof(double);
}

int rlt_reward_spec_matrix(const float* labels, int B, int S, const rlt_reward_spec* spec, float tau, const void* dcg_table,
                           float* r_out, float* q_out, void* stream) {
    RLT_CHECK_ARG(labels && B > 0 && S > 0 && (r_out || q_out));
    RLT_CHECK_ARG(tau > 0.f && std::isfinite(tau));
    AnyArgs a{};
    int rc = any_spec(spec, dcg_table, a);
    if (rc) return rc;
    RLT_CHECK_SHAPE(S <= ANY_MAX_S);
    rc = any_rows_aligned(S, {labels, r_out, q_out});
    if (rc) return rc;
    a.y = labels; a.r_out = r_out; a.q_out = q_out;
    a.B = B; a.S = S; a.kind = RLT_LOSS_KL;
    a.tau = (double)tau; a.gscale = 1.0;
    dispatch_any(a, any_grid(B, S), rlt_stream(stream));
    return RLT_LAUNCH_RESULT();
}

int rlt_reward_any_loss(const float* p, const float* labels, const rlt_reward_spec* spec, const float* r_in, int B, int S,
                        int kind, float tau, float* loss_per_list, float* loss_out, float* dp,
                        int32_t* k_out, float* r_k, float* r_best, int32_t* best_k, double* sums,
                        const void* dcg_table, void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(p && ws && B > 0 && S > 0);
    RLT_CHECK_ARG((labels && spec && !r_in) || (r_in && !labels && !spec));      // exactly one reward source
    RLT_CHECK_ARG(kind >= RLT_LOSS_EXPECT && kind <= RLT_LOSS_JS);
    RLT_CHECK_ARG(tau > 0.f && std::isfinite(tau));
    AnyArgs a{};
    if (spec) {
        const int rc = any_spec(spec, dcg_table, a);
        if (rc) return rc;
    } else {
        a.src = SRC_MATRIX;
    }
    RLT_CHECK_SHAPE(S <= ANY_MAX_S);
    int rc = any_rows_aligned(S, {p, labels, r_in, dp});
    if (rc) return rc;
    if ((((uintptr_t)ws | (uintptr_t)sums) & 7u) != 0 || (((uintptr_t)loss_per_list | (uintptr_t)loss_out | (uintptr_t)k_out |
          (uintptr_t)r_k | (uintptr_t)r_best | (uintptr_t)best_k) & 3u) != 0)
        return RLT_E_ALIGN;
    if (ws_bytes < rlt_reward_any_workspace(B)) return RLT_E_WORKSPACE;
    a.p = p; a.y = labels; a.r_in = r_in;
    a.loss_per_list = loss_per_list; a.dp = dp;
    a.k_out = k_out; a.r_k = r_k; a.r_best = r_best; a.best_k = best_k;
    a.records = (double*)ws;
    a.B = B; a.S = S; a.kind = kind;
    a.tau = (double)tau; a.gscale = 1.0 / (double)B;
    hipStream_t st = rlt_stream(stream);
    const int grid = any_grid(B, S);
    dispatch_any(a, grid, st);
    rc = RLT_LAUNCH_RESULT();
    if (rc) return rc;
    if (loss_out || sums) {
        hipLaunchKernelGGL(reward_any_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, grid, (double)B, loss_out, sums);
        rc = RLT_LAUNCH_RESULT();
    }
    return rc;
}

}  // extern "C"
