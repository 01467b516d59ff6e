// Evaluation in ANY cut reward: what the truncation baselines, the cut report, the cut sweep and the paired comparison need
// from a reward row, in one pass.  reward_any.hip trains on a reward spec or a caller's matrix; this file answers, for the same
// reward, what the best cut of every list reaches (Oracle), what every fixed k reaches (Fixed-k, Greedy-k), what T given cuts
// per list reach and on how many positions each of them is beaten.
//
// The reward r[b,k], k = 1..S, is the row reward_form.h builds - the text rlt_reward_spec_matrix compiles, so the fp32 values
// are the same bits - with r[b,0] = 0 in front: cutting before the first document keeps nothing.
//
// The pass has the layout of reward_any_kernel: a wavefront owns whole lists - four (one per row of 16 lanes), two or one by S
// and S % 4 - rows of S % 4 == 0 floats are read 16 bytes at a time, the grid is sized to the chip and strides over the lists.
// The reward row stays in registers; the sums per position (the reward curve, the histogram of the best cut) are kept per lane.
// The T cuts of a list are served from a copy of the row in the wavefront's own LDS (entry 0 = 0), one lane per cut; `better`
// compares the whole row in registers against one cut at a time: with one list per wavefront the comparison is a ballot and the
// scalar unit counts its bits, with two or four lists the lanes count and a DPP sum over the list's lanes adds them.
//
// Every workgroup leaves ONE float64 record {curve (S), best_hist (S+1), sum best, clamped cuts, 3 per cut} in ws - the lists
// of a wavefront in lane order, then the wavefronts in turn - and a second launch adds the records column by column in a fixed
// order into the caller's sums (or onto them: `accumulate`).  No atomics, no allocation, no host synchronisation: two calls give
// the same bits.
//
// Algorithmic bytes per list: read 4 S + 4 T, write up to 8 T + 8 B of per-list results.
#include "reward_form.h"

namespace {

constexpr int EVAL_MAX_T = 64;
constexpr int EVAL_MAX_GRID = 1024;             // workgroups (4 per CU); beyond that they stride over the lists

// the record: [0, S) sum r[., k] for k = 1..S; [S, 2S + 1) lists whose best cut is k = 0..S; 2S + 1: sum best; 2S + 2: clamped
// cuts; from 2S + 3, per cut t: sum r_at, #(r_at == best), sum better
__host__ __device__ constexpr int eval_cols(int S, int T) { return 2 * S + 3 + 3 * T; }

struct EvalArgs {
    RewardSrc s;                // the reward: labels + spec, or r_in (reward_form.h)
    const int32_t* k_in;        // (B,T) or null
    float* r_at;                // (B,T) or null
    int32_t* better;            // (B,T) or null
    float* best;                // (B) or null
    int32_t* best_k;            // (B) or null
    double* records;            // (grid, eval_cols(S, T)) or null: no split output asked for
    int B, S, T, allow_empty;
    int need_better;            // better itself or the sums over it
};

template <int LL, int R, int V>
__global__ __launch_bounds__(256) void reward_eval_kernel(EvalArgs a) {
    constexpr int N = R * V, PR = V * LL, LPW = 64 / LL;
    constexpr int TI = 64 / LL;                 // cuts per lane: lane hl of a list serves the cuts hl, hl + LL, ...
    constexpr int ROWF = LPW * (R * PR + 1);    // a wavefront's rows with the k = 0 entry in front of each
    constexpr int ROW_BYTES = ANY_WAVES * ROWF * 4, REC_BYTES = eval_cols(R * PR, EVAL_MAX_T) * 8;
    constexpr int POOL = ((ROW_BYTES > REC_BYTES ? ROW_BYTES : REC_BYTES) + 7) / 8;
    __shared__ RewardTables tb;
    __shared__ double pool[POOL];               // the rows while the lists stream, then the record
    __shared__ float srat[ANY_WAVES][LPW][EVAL_MAX_T];
    __shared__ int sbet[ANY_WAVES][LPW][EVAL_MAX_T];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool upper = lane >= 32;
    const int hl = lane & (LL - 1), grp = lane / LL;
    const int S = a.S, B = a.B, T = a.T;
    const auto iadd = [](int x, int z) { return x + z; };
    const auto fmx = [](float x, float z) { return x > z ? x : z; };
    const auto imn = [](int x, int z) { return x < z ? x : z; };
    reward_tables(a.s, S, tid, tb);
    bool ok[R];                                 // rounds before the last lie inside the list when V == 4; V == 1: per round
#pragma unroll
    for (int r = 0; r < R; ++r) ok[r] = r * PR + V * hl < S;
    float* const srow = reinterpret_cast<float*>(pool) + wv * ROWF + grp * (S + 1);
    double cs[N];                               // this lane's positions: sum of r
    int hs[N];                                  // ... lists whose best cut they are
#pragma unroll
    for (int n = 0; n < N; ++n) { cs[n] = 0.0; hs[n] = 0; }
    double srt[TI], seq[TI], sbt[TI];           // this lane's cuts: sum r_at, #(r_at == best), sum better
#pragma unroll
    for (int i = 0; i < TI; ++i) srt[i] = seq[i] = sbt[i] = 0.0;
    double sum_best = 0.0, n_empty = 0.0, n_clamped = 0.0;
    const float* const src = a.s.src == SRC_MATRIX ? a.s.r_in : a.s.y;
    const long long step = (long long)LPW * gridDim.x * ANY_WAVES;
    for (long long pb = LPW * (blockIdx.x * ANY_WAVES + wv); pb < B; pb += step) {      // 64-bit: B up to INT_MAX
        const bool live = pb + grp < B;         // lists beyond B: the idle group shadows the first one, stores and sums masked
        const int b = (int)(live ? pb + grp : pb);
        const size_t base = (size_t)b * S;
        float rv[N];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const size_t at = base + (ok[r] ? r * PR + V * hl : 0);
            if constexpr (V == 4) {
                const float4 vy = *reinterpret_cast<const float4*>(src + at);
                rv[4 * r] = vy.x; rv[4 * r + 1] = vy.y; rv[4 * r + 2] = vy.z; rv[4 * r + 3] = vy.w;
            } else {
                rv[r] = src[at];
            }
        }
        reward_form<LL, R, V>(a.s, tb, ok, hl, upper, rv);
        // ---- the row's best reward over kmin..S and its first position (np.argmax: k = 0 wins a tie) -------------------------
        float mx_l = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (ok[r] && rv[V * r + i] > mx_l) { mx_l = rv[V * r + i]; bi = r * PR + V * hl + i; }
        const float gmx = any_reduce<LL>(mx_l, -INFINITY, fmx, upper);
        const int bk = any_reduce<LL>(mx_l == gmx ? bi : 0x7fffffff, 0x7fffffff, imn, upper);
        const bool empty = a.allow_empty && !(gmx > 0.f);
        const float best = empty ? 0.f : gmx;
        const int best_k = empty ? 0 : (bk == 0x7fffffff ? 0 : bk) + 1;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (live && ok[r]) {
                    cs[V * r + i] += (double)rv[V * r + i];
                    hs[V * r + i] += (r * PR + V * hl + i + 1 == best_k) ? 1 : 0;
                }
        if (live && hl == 0) {
            if (a.best) a.best[b] = best;
            if (a.best_k) a.best_k[b] = best_k;
            sum_best += (double)best;
            n_empty += empty ? 1.0 : 0.0;
        }
        // ---- the T cuts of the list: one lane each from the row in LDS ---------------------------------------------------------
        if (T > 0) {
            if (hl == 0) srow[0] = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (ok[r]) srow[1 + r * PR + V * hl + i] = rv[V * r + i];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int t = hl + LL * i;
                if (t < T) {
                    const int k = a.k_in[(size_t)b * T + t];
                    const int kc = k < 0 ? 0 : (k > S ? S : k);
                    const float x = srow[kc];
                    srat[wv][grp][t] = x;
                    if (live) {
                        if (a.r_at) a.r_at[(size_t)b * T + t] = x;
                        srt[i] += (double)x;
                        seq[i] += x == best ? 1.0 : 0.0;
                        n_clamped += k != kc ? 1.0 : 0.0;
                    }
                }
            }
            if (a.need_better) {
                __builtin_amdgcn_wave_barrier();
                for (int t = 0; t < T; ++t) {
                    const float x = srat[wv][grp][t];
                    int cnt = 0;
                    if constexpr (LL == 64) {   // one list: a ballot per register, counted on the scalar unit
#pragma unroll
                        for (int n = 0; n < N; ++n) cnt += __popcll(__ballot(ok[n / V] && rv[n] > x));
                    } else {
#pragma unroll
                        for (int n = 0; n < N; ++n) cnt += (ok[n / V] && rv[n] > x) ? 1 : 0;
                        cnt = any_reduce<LL>(cnt, 0, iadd, upper);
                    }
                    cnt += (a.allow_empty && 0.f > x) ? 1 : 0;
                    if (hl == 0) sbet[wv][grp][t] = cnt;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int t = hl + LL * i;
                    if (t < T && live) {
                        const int c = sbet[wv][grp][t];
                        if (a.better) a.better[(size_t)b * T + t] = c;
                        sbt[i] += (double)c;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();    // the next list's stores come after these loads
        }
    }
    if (!a.records) return;
    // ---- one record per workgroup: the lists of a wavefront in lane order, then the wavefronts in turn --------------------------
    double hd[N];
#pragma unroll
    for (int n = 0; n < N; ++n) hd[n] = (double)hs[n];
    if constexpr (LL == 16) {                   // the four rows hold the same positions: (row 0 + row 1) + (row 2 + row 3) into row 0
#pragma unroll
        for (int n = 0; n < N; ++n) { cs[n] += __shfl_down(cs[n], 16); hd[n] += __shfl_down(hd[n], 16); }
#pragma unroll
        for (int i = 0; i < TI; ++i) { srt[i] += __shfl_down(srt[i], 16); seq[i] += __shfl_down(seq[i], 16); sbt[i] += __shfl_down(sbt[i], 16); }
    }
    if constexpr (LL <= 32) {
#pragma unroll
        for (int n = 0; n < N; ++n) { cs[n] += __shfl_down(cs[n], 32); hd[n] += __shfl_down(hd[n], 32); }
#pragma unroll
        for (int i = 0; i < TI; ++i) { srt[i] += __shfl_down(srt[i], 32); seq[i] += __shfl_down(seq[i], 32); sbt[i] += __shfl_down(sbt[i], 32); }
    }
    sum_best = wave_sum(sum_best);
    n_empty = wave_sum(n_empty);
    n_clamped = wave_sum(n_clamped);
    __syncthreads();                            // the rows are done with: their space becomes the record
    double* const red = pool;
    for (int w = 0; w < ANY_WAVES; ++w) {
        if (wv == w && lane < LL) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const int j = r * PR + V * lane + i;
                    if (j < S) {
                        red[j] = w ? red[j] + cs[V * r + i] : cs[V * r + i];
                        red[S + 1 + j] = w ? red[S + 1 + j] + hd[V * r + i] : hd[V * r + i];
                    }
                }
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int t = lane + LL * i;
                if (t < T) {
                    double* const c = red + 2 * S + 3 + 3 * t;
                    c[0] = w ? c[0] + srt[i] : srt[i];
                    c[1] = w ? c[1] + seq[i] : seq[i];
                    c[2] = w ? c[2] + sbt[i] : sbt[i];
                }
            }
            if (lane == 0) {
                red[S] = w ? red[S] + n_empty : n_empty;
                red[2 * S + 1] = w ? red[2 * S + 1] + sum_best : sum_best;
                red[2 * S + 2] = w ? red[2 * S + 2] + n_clamped : n_clamped;
            }
        }
        __syncthreads();
    }
    const int ncol = eval_cols(S, T);
    for (int i = tid; i < ncol; i += 256) a.records[(size_t)blockIdx.x * ncol + i] = red[i];
}

// column sums of the records in a fixed order (16 row lanes x 16 columns per workgroup, four loads in flight per lane, then the
// row lanes in order) into curve at k = 1..S, best_hist and sums[1..]; curve[0] and the list count (sums[0]) from the arguments
__global__ __launch_bounds__(256) void reward_eval_final_kernel(const double* __restrict__ rec, int rows, int S, int T, int B,
                                                                int accumulate, double* __restrict__ curve,
                                                                double* __restrict__ best_hist, double* __restrict__ sums) {
    __shared__ double part[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int ncol = eval_cols(S, T);
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
        double* dst = col < S ? (curve ? curve + col + 1 : nullptr)
                    : col < 2 * S + 1 ? (best_hist ? best_hist + (col - S) : nullptr)
                                      : (sums ? sums + (col - 2 * S) : nullptr);
        if (dst) *dst = accumulate ? *dst + acc : acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (curve && !accumulate) curve[0] = 0.0;                  // k = 0: 0 for every list (adding 0 changes nothing)
        if (sums) sums[0] = (accumulate ? sums[0] : 0.0) + (double)B;
    }
}

int eval_grid(int B, int S) {
    const int groups = rlt_cdiv(B, ANY_WAVES * (64 / any_lanes(S)));
    return groups < EVAL_MAX_GRID ? groups : EVAL_MAX_GRID;
}

}  // namespace

extern "C" {

size_t rlt_reward_eval_workspace(int B, int S, int T) {
    if (B <= 0 || S <= 0 || S > ANY_MAX_S || T < 0 || T > EVAL_MAX_T) return 0;
    const int groups = rlt_cdiv(B, ANY_WAVES);                  // the largest grid of any layout
    return ((size_t)(groups < EVAL_MAX_GRID ? groups : EVAL_MAX_GRID) * eval_cols(S, T) * sizeof(double) + 15) / 16 * 16;
}

int rlt_reward_eval(const float* labels, const rlt_reward_spec* spec, const float* r_in, int B, int S,
                    const int32_t* k_in, int T, int allow_empty, const void* dcg_table, int accumulate,
                    float* r_at, int32_t* better, float* best, int32_t* best_k,
                    double* curve, double* best_hist, double* sums,
                    void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG((labels && spec && !r_in) || (r_in && !labels && !spec));      // exactly one reward source
    RLT_CHECK_ARG(B > 0 && S > 0);
    RLT_CHECK_ARG(T >= 0 && T <= EVAL_MAX_T);
    RLT_CHECK_ARG(T == 0 || k_in);
    RLT_CHECK_ARG(T > 0 || (!r_at && !better));
    RLT_CHECK_ARG(r_at || better || best || best_k || curve || best_hist || sums);
    RLT_CHECK_ARG(ws);
    EvalArgs a{};
    if (spec) {                                 // a misaligned table is RLT_E_ALIGN, which comes after RLT_E_SHAPE
        const int rc = any_spec(spec, dcg_table, a.s);
        if (rc == RLT_E_ARG) return rc;
        RLT_CHECK_SHAPE(S <= ANY_MAX_S);
        if (rc) return rc;
    } else {
        RLT_CHECK_SHAPE(S <= ANY_MAX_S);
        a.s.src = SRC_MATRIX;
    }
    const int rc = any_rows_aligned(S, {labels, r_in});
    if (rc) return rc;
    if ((((uintptr_t)ws | (uintptr_t)curve | (uintptr_t)best_hist | (uintptr_t)sums) & 7u) != 0 ||
        (((uintptr_t)k_in | (uintptr_t)r_at | (uintptr_t)better | (uintptr_t)best | (uintptr_t)best_k) & 3u) != 0)
        return RLT_E_ALIGN;
    if (ws_bytes < rlt_reward_eval_workspace(B, S, T)) return RLT_E_WORKSPACE;
    const bool split = curve || best_hist || sums;
    a.s.y = labels; a.s.r_in = r_in;
    a.k_in = T > 0 ? k_in : nullptr;
    a.r_at = r_at; a.better = better; a.best = best; a.best_k = best_k;
    a.records = split ? (double*)ws : nullptr;
    a.B = B; a.S = S; a.T = T; a.allow_empty = allow_empty ? 1 : 0;
    a.need_better = (T > 0 && (better || sums)) ? 1 : 0;
    hipStream_t st = rlt_stream(stream);
    const int grid = eval_grid(B, S);
    any_dispatch(S, [&](auto f) {
        hipLaunchKernelGGL((reward_eval_kernel<f.LL, f.R, f.V>), dim3(grid), dim3(256), 0, st, a);
    });
    int lrc = RLT_LAUNCH_RESULT();
    if (lrc) return lrc;
    if (split) {
        hipLaunchKernelGGL(reward_eval_final_kernel, dim3(rlt_cdiv(eval_cols(S, T), 16)), dim3(256), 0, st, (const double*)ws, grid,
                           S, T, B, accumulate ? 1 : 0, curve, best_hist, sums);
        lrc = RLT_LAUNCH_RESULT();
    }
    return lrc;
}

}  // extern "C"
