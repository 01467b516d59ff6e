// The reward row of a cut-reward spec, formed in registers: the ONE definition behind rlt_reward_spec_matrix,
// rlt_reward_any_loss (reward_any.hip) and rlt_reward_eval (reward_eval.hip).  Their bit-for-bit contract - the evaluation
// pass sees exactly the fp32 reward the training pass saw - rests on both files compiling this text.
//
// Layout (as rlt_loss_metrics): a wavefront owns whole lists, LL = 16, 32 or 64 lanes per list, R rounds, V consecutive
// positions per lane and round (4: 16-byte accesses, S % 4 == 0; 1 otherwise): element (r, i) of a lane is position
// r * V * LL + V * hl + i.  The prefix sums run round by round: a serial scan of the lane's own positions, a DPP scan over the
// list's lanes, the running total of the rounds before.  The reward is formed in float64 and rounded to fp32 ONCE (rlt_hip.h).
#pragma once
#include "common.h"
#include <cmath>
#include <initializer_list>

namespace {

constexpr int ANY_MAX_S = 1024;
constexpr int ANY_WAVES = 4;
constexpr int SRC_FBETA = 0, SRC_GAIN = 1, SRC_MATRIX = 2;

// where the reward comes from: the kernel-argument form of rlt_reward_spec (any_spec), or a caller's matrix
struct RewardSrc {
    const float* y;             // (B,S) labels, spec sources
    const float* r_in;          // (B,S) reward, matrix source
    const float* disc;          // (S) discounts or null: the table's 1 / log2(j + 2)
    const double* tab;          // DCG table (rlt_dcg_table_init)
    int src;
    int n_grades, normalize, n_take;
    int order[RLT_REWARD_MAX_GRADES];     // the grades of positive gain in the order the ideal list takes them
    double gain[RLT_REWARD_MAX_GRADES];
    double beta2;
};

// the workgroup's copy of what a GAIN spec reads per position
struct RewardTables {
    double sd[ANY_MAX_S];            // d_j
    double sD[ANY_MAX_S + 1];        // D[k] = sum_{j<k} d_j
    double sg[RLT_REWARD_MAX_GRADES];
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

// fills t for a GAIN source; every thread of the 256-thread workgroup calls it, and it ends on a barrier
__device__ __forceinline__ void reward_tables(const RewardSrc& s, int S, int tid, RewardTables& t) {
    if (s.src == SRC_GAIN) {
        for (int j = tid; j < S; j += 256) t.sd[j] = s.disc ? (double)s.disc[j] : s.tab[j];
        if (tid < RLT_REWARD_MAX_GRADES) t.sg[tid] = s.gain[tid];
        if (s.normalize) {
            if (!s.disc) {
                for (int k = tid; k <= S; k += 256) t.sD[k] = s.tab[ANY_MAX_S + k];
            } else {
                __syncthreads();
                if (tid == 0) {                 // the sums a sequential float64 loop produces
                    double acc = 0.0;
                    t.sD[0] = 0.0;
                    for (int k = 0; k < S; ++k) { acc += t.sd[k]; t.sD[k + 1] = acc; }
                }
            }
        }
        __syncthreads();
    }
}

// rv: the list's labels on entry (spec sources), the reward r_k, k = j + 1, on return: float64, rounded to fp32 once.  A matrix
// source is left as it was loaded.  ok[r]: round r of this lane lies inside the list.
template <int LL, int R, int V>
__device__ __forceinline__ void reward_form(const RewardSrc& s, const RewardTables& t, const bool (&ok)[R], int hl, bool upper,
                                            float (&rv)[R * V]) {
    constexpr int N = R * V, PR = V * LL;
    const auto iadd = [](int x, int z) { return x + z; };
    const auto dadd = [](double x, double z) { return x + z; };
    if (s.src == SRC_FBETA) {
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
        const double num = 1.0 + s.beta2, bn = s.beta2 * (double)off;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int k = r * PR + V * hl + i + 1;
                rv[V * r + i] = c[V * r + i] > 0 ? (float)(num * (double)c[V * r + i] / (bn + (double)k)) : 0.f;
            }
    } else if (s.src == SRC_GAIN) {
        int g[N];
        const float gmax = (float)(s.n_grades - 1);
#pragma unroll
        for (int n = 0; n < N; ++n) g[n] = (int)fminf(fmaxf(rintf(rv[n]), 0.f), gmax);     // NaN: fmaxf gives 0
        double inv = 1.0;
        bool zero = false;
        if (s.normalize) {
            double ideal = 0.0;
            int at = 0;
            for (int tk = 0; tk < s.n_take; ++tk) {
                const int gr = s.order[tk];
                int cnt = 0;
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int i = 0; i < V; ++i) cnt += (ok[r] && g[V * r + i] == gr) ? 1 : 0;
                cnt = any_reduce<LL>(cnt, 0, iadd, upper);
                ideal += t.sg[gr] * (t.sD[at + cnt] - t.sD[at]);
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
                run += ok[r] ? t.sg[g[V * r + i]] * t.sd[r * PR + V * hl + i] : 0.0;
                cum[i] = run;
            }
            const double incl = any_scan<LL>(run, 0.0, dadd);
            const double ex = (incl - run) + off;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const double v = ex + cum[i];
                rv[V * r + i] = s.normalize ? (zero ? 0.f : (float)(v / inv)) : (float)v;
            }
            off += any_last<LL>(incl, upper);
        }
    }
}

// lanes per list, as dispatch_reward_m of loss.hip picks them: S % 4 == 0 and S <= 384: four lists per wavefront where rounds
// of 64 positions waste fewer lane slots than rounds of 128 (an odd number of them, up to five), two otherwise; one list per
// wavefront beyond that and for every S % 4 != 0
inline int any_lanes(int S) {
    if ((S & 3) != 0 || S > 384) return 64;
    const int r16 = rlt_cdiv(S, 64);
    return ((r16 & 1) && r16 <= 5) ? 16 : 32;
}

// the (LL, R, V) instance of a kernel template for lists of S positions: launch(Tag<LL, R, V>{})
template <int LL_, int R_, int V_> struct AnyForm { static constexpr int LL = LL_, R = R_, V = V_; };
template <typename F>
void any_dispatch(int S, F&& launch) {
    if ((S & 3) == 0) {
        const int ll = any_lanes(S);
        if (ll == 16) {
            switch (rlt_cdiv(S, 64)) {
                case 1: return launch(AnyForm<16, 1, 4>{});
                case 3: return launch(AnyForm<16, 3, 4>{});
                default: return launch(AnyForm<16, 5, 4>{});
            }
        }
        if (ll == 32) {
            switch (rlt_cdiv(S, 128)) {
                case 1: return launch(AnyForm<32, 1, 4>{});
                case 2: return launch(AnyForm<32, 2, 4>{});
                default: return launch(AnyForm<32, 3, 4>{});
            }
        }
        switch (rlt_cdiv(S, 256)) {
            case 2: return launch(AnyForm<64, 2, 4>{});
            case 3: return launch(AnyForm<64, 3, 4>{});
            default: return launch(AnyForm<64, 4, 4>{});
        }
    }
    const int c = rlt_cdiv(S, 64);              // the chunk sizes of the general reward kernel
    if (c <= 1) return launch(AnyForm<64, 1, 1>{});
    if (c <= 2) return launch(AnyForm<64, 2, 1>{});
    if (c <= 3) return launch(AnyForm<64, 3, 1>{});
    if (c <= 4) return launch(AnyForm<64, 4, 1>{});
    if (c <= 5) return launch(AnyForm<64, 5, 1>{});
    if (c <= 6) return launch(AnyForm<64, 6, 1>{});
    if (c <= 8) return launch(AnyForm<64, 8, 1>{});
    if (c <= 12) return launch(AnyForm<64, 12, 1>{});
    return launch(AnyForm<64, 16, 1>{});
}

// spec -> the kernel's arguments; RLT_E_ARG for a spec outside rlt_hip.h's ranges
inline int any_spec(const rlt_reward_spec* spec, const void* dcg_table, RewardSrc& a) {
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

inline int any_rows_aligned(int S, std::initializer_list<const float*> rows) {
    const uintptr_t mask = (S & 3) == 0 ? 15u : 3u;
    for (const float* r : rows)
        if (r && ((uintptr_t)r & mask) != 0) return RLT_E_ALIGN;
    return 0;
}

}  // namespace
