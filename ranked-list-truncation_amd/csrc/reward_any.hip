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
#include "reward_form.h"

namespace {

constexpr int ANY_MAX_GRID = 256 * 8;           // as loss.hip: up to 8 workgroups per CU, beyond that the workgroups stride
constexpr int ANY_REC = 4;                      // doubles per workgroup record

struct AnyArgs {
    RewardSrc s;                // the reward: labels + spec, or r_in (reward_form.h)
    const float* p;             // (B,S) or null (rlt_reward_spec_matrix)
    float* loss_per_list;       // (B) or null
    float* dp;                  // (B,S) or null
    float* r_out;               // (B,S) or null
    float* q_out;               // (B,S) or null
    int32_t* k_out;             // (B) or null
    float* r_k;                 // (B) or null
    float* r_best;              // (B) or null
    int32_t* best_k;            // (B) or null
    double* records;            // (grid, ANY_REC) or null
    int B, S, kind;
    double tau, gscale;
};

// LL lanes per list, R rounds, V consecutive positions per lane and round (4: 16-byte accesses, S % 4 == 0; 1 otherwise):
// element (r, i) of a lane is position r * V * LL + V * hl + i
template <int LL, int R, int V>
__global__ __launch_bounds__(256) void reward_any_kernel(AnyArgs a) {
    constexpr int N = R * V, PR = V * LL, LPW = 64 / LL;
    __shared__ RewardTables tb;
    __shared__ double srec[ANY_WAVES][ANY_REC];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool upper = lane >= 32;
    const int hl = lane & (LL - 1), grp = lane / LL;
    const int S = a.S, B = a.B;
    const auto dadd = [](double x, double z) { return x + z; };
    const auto fmx = [](float x, float z) { return x > z ? x : z; };
    const auto imn = [](int x, int z) { return x < z ? x : z; };
    reward_tables(a.s, S, tid, tb);
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
            const float* src = a.s.src == SRC_MATRIX ? a.s.r_in : a.s.y;
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
        // ---- the reward r_k, k = j + 1: float64, rounded to fp32 once (reward_form.h) --------------------------------------
        reward_form<LL, R, V>(a.s, tb, ok, hl, upper, rv);
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

int any_grid(int B, int S) {
    const int groups = rlt_cdiv(B, ANY_WAVES * (64 / any_lanes(S)));
    return groups < ANY_MAX_GRID ? groups : ANY_MAX_GRID;
}

void dispatch_any(const AnyArgs& a, int grid, hipStream_t st) {
    any_dispatch(a.S, [&](auto f) {
        hipLaunchKernelGGL((reward_any_kernel<f.LL, f.R, f.V>), dim3(grid), dim3(256), 0, st, a);
    });
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
    int rc = any_spec(spec, dcg_table, a.s);
    if (rc) return rc;
    RLT_CHECK_SHAPE(S <= ANY_MAX_S);
    rc = any_rows_aligned(S, {labels, r_out, q_out});
    if (rc) return rc;
    a.s.y = labels; a.r_out = r_out; a.q_out = q_out;
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
        const int rc = any_spec(spec, dcg_table, a.s);
        if (rc) return rc;
    } else {
        a.s.src = SRC_MATRIX;
    }
    RLT_CHECK_SHAPE(S <= ANY_MAX_S);
    int rc = any_rows_aligned(S, {p, labels, r_in, dp});
    if (rc) return rc;
    if ((((uintptr_t)ws | (uintptr_t)sums) & 7u) != 0 || (((uintptr_t)loss_per_list | (uintptr_t)loss_out | (uintptr_t)k_out |
          (uintptr_t)r_k | (uintptr_t)r_best | (uintptr_t)best_k) & 3u) != 0)
        return RLT_E_ALIGN;
    if (ws_bytes < rlt_reward_any_workspace(B)) return RLT_E_WORKSPACE;
    a.p = p; a.s.y = labels; a.s.r_in = r_in;
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
