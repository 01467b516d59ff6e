// Pairwise ranking losses on the scores of a rerank head: RankNet (every pair of unequal grade weighs 1) and LambdaRank (a pair
// weighs the change in nDCG that swapping it would cause), their gradient, and the counting rank of every document - the O(S^2)
// rank the pass needs for the discounts, delivered as an output.  Definitions: include/rlt_hip.h.
//
// A group of L lanes inside one wavefront owns a list (16 lanes for S <= 64: four lists per wavefront; 32 for S <= 128: two; 64
// beyond), lane hl holding the R documents hl, hl + L, ... in registers (N = L * R slots).  The list's {score, grade, D(pi)}
// records sit in the wavefront's own LDS, 16 bytes per document, and every step of the two walks over j reads ONE record with a
// group-uniform address - a broadcast.  Walk 1 counts pi_i (two compares per visit); walk 2 forms the pair terms: a lane adds
// what each of its pairs gives to ITS document from whichever side it stands on, so dscore needs no sum across lanes and no
// atomics; the loss is summed by the lane of the pair's higher grade, then over the group in a fixed butterfly.
//
// Arithmetic.  s_i - s_j (exact), x = sigma (s_i - s_j), the weight and all sums over j are float64: |D(pi_i) - D(pi_j)| cancels
// up to 13 bits at the tail of a long list.  exp, log1p and the sigmoid's division are fp32 library calls on the fp32 head of
// a = |x|; the float64 tail a - (float)a enters as the factor 1 - tail, which keeps exp(-a) to a few ulp on the saturated branch,
// where an fp32 x alone would lose a * 2^-24 of it.  Pairs of equal grade branch around all of that.
//
// Every workgroup leaves ONE float64 record (the sum of its lists' losses, in a fixed order) in ws; a one-workgroup launch adds
// the records in a fixed order.  No atomics, no allocation, no host synchronisation: two calls give the same bits.
//
// Algorithmic bytes per list: read 8 S, write up to 8 S + 8.  The pass is bound by the vector ALU, not by memory: S^2 visits,
// and a wavefront pays the transcendental path of a visit when ANY of its lanes holds a document of another grade than j's.
#include "reward_form.h"

namespace {

constexpr int PR_MAX_S = 1024;
constexpr int PR_MAX_GRID = 2048;               // workgroups (8 per CU); beyond that they stride over the lists

struct PairDoc {                                // one LDS record, read as a 16-byte broadcast
    float s;
    int g;
    double D;
};

struct PairArgs {
    const float* score;
    const float* labels;
    const double* tab;          // DCG table (rlt_dcg_table_init) or null (RANKNET)
    const float* gscale;        // device scalar or null
    float* loss_per_list;
    float* dscore;
    int32_t* rank_out;
    int32_t* n_pairs;
    double* records;            // (grid)
    int B, S, kind, n_grades, normalize, n_take;
    int want_loss;              // loss_per_list or loss_out is asked for
    int order[RLT_REWARD_MAX_GRADES];           // the grades of positive gain in the order the ideal list takes them (any_spec)
    double gain[RLT_REWARD_MAX_GRADES];
    double sigma;
};

// the same value in every lane of each group of L lanes; a fixed butterfly, so a fixed order
template <int L, typename T>
__device__ __forceinline__ T pair_group_sum(T v) {
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, L);
    return v;
}

template <int L, int R, int W>
__global__ __launch_bounds__(64 * W) void pair_rank_kernel(PairArgs a) {
    constexpr int N = L * R, LPW = 64 / L, STRIDE = N + 1;      // + 1 record: the lists of a wavefront start on different banks
    __shared__ PairDoc sdoc[W][LPW][STRIDE];
    __shared__ double srec[W];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int hl = lane & (L - 1), grp = lane / L;
    const int S = a.S, B = a.B;
    const bool lambda = a.kind == RLT_PAIR_LAMBDARANK;
    const bool need_rank = lambda || a.rank_out != nullptr;
    const float gmax = (float)(a.n_grades - 1);
    PairDoc* const sd = sdoc[wv][grp];
    double wave_loss = 0.0;
    const long long step = (long long)LPW * gridDim.x * W;
    for (long long pb = (long long)LPW * (blockIdx.x * W + wv); pb < B; pb += step) {       // 64-bit: B up to INT_MAX
        const bool live = pb + grp < B;         // lists beyond B: the idle group shadows the first one, its stores are masked
        const size_t base = (size_t)(live ? pb + grp : pb) * S;
        float si[R];
        int gi[R];
        double Gi[R];
        int cnt[RLT_REWARD_MAX_GRADES];
#pragma unroll
        for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) cnt[g] = 0;
        int has_nan = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = hl + r * L;
            const bool ok = i < S;
            si[r] = ok ? a.score[base + i] : 0.f;
            const float y = ok ? a.labels[base + i] : 0.f;
            gi[r] = (int)fminf(fmaxf(rintf(y), 0.f), gmax);         // NaN: fmaxf gives 0
            Gi[r] = 0.0;
#pragma unroll
            for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) {
                const bool is = ok && gi[r] == g;
                cnt[g] += is ? 1 : 0;
                Gi[r] = is ? a.gain[g] : Gi[r];
            }
            has_nan |= (si[r] != si[r]) ? 1 : 0;
            if (ok) { sd[i].s = si[r]; sd[i].g = gi[r]; sd[i].D = 0.0; }
        }
#pragma unroll
        for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) cnt[g] = pair_group_sum<L>(cnt[g]);
        has_nan = pair_group_sum<L>(has_nan);
        int npairs = 0, below = 0;
#pragma unroll
        for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) { npairs += cnt[g] * below; below += cnt[g]; }
        __builtin_amdgcn_wave_barrier();
        // ---- walk 1: the counting rank, and D(pi) into the records ----------------------------------------------------------
        double Di[R];
#pragma unroll
        for (int r = 0; r < R; ++r) Di[r] = 0.0;
        if (need_rank) {
            int pi[R];
#pragma unroll
            for (int r = 0; r < R; ++r) pi[r] = 0;
            for (int j = 0; j < S; ++j) {
                const float sj = sd[j].s;
#pragma unroll
                for (int r = 0; r < R; ++r) pi[r] += (sj > si[r] || (sj == si[r] && j < hl + r * L)) ? 1 : 0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = hl + r * L;
                if (i < S) {
                    if (live && a.rank_out) a.rank_out[base + i] = pi[r];
                    if (lambda) { Di[r] = a.tab[pi[r]]; sd[i].D = Di[r]; }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- the list's ideal value, in the order rlt_reward_spec takes the grades --------------------------------------------
        double wnorm = 1.0;
        if (lambda && a.normalize) {
            double ideal = 0.0;
            int at = 0;
            for (int tk = 0; tk < a.n_take; ++tk) {
                const int gr = a.order[tk];
                int c = 0;
#pragma unroll
                for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) c = gr == g ? cnt[g] : c;
                ideal += a.gain[gr] * (a.tab[PR_MAX_S + at + c] - a.tab[PR_MAX_S + at]);
                at += c;
            }
            if (ideal > 0.0) wnorm = 1.0 / ideal;
        }
        // ---- walk 2: the pairs ------------------------------------------------------------------------------------------------
        double acc[R];                          // sum over the pairs of document i of +- w sigmoid(-x)
        double lsum = 0.0;                      // sum of w softplus(-x) over the pairs this lane's documents lead
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        if (npairs > 0 && (a.dscore || a.want_loss)) {
            for (int j = 0; j < S; ++j) {
                const PairDoc dj = sd[j];
                double Gj = 0.0;
#pragma unroll
                for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) Gj = dj.g == g ? a.gain[g] : Gj;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (gi[r] != dj.g && hl + r * L < S) {
                        const bool lead = gi[r] > dj.g;                     // this lane's document is the pair's i
                        const double d = (double)si[r] - (double)dj.s;
                        const double x = a.sigma * (lead ? d : -d);
                        const double w = lambda ? fabs(Gi[r] - Gj) * fabs(Di[r] - dj.D) * wnorm : 1.0;
                        const double ab = fabs(x);
                        const float ah = (float)ab;
                        const float al = (float)(ab - (double)ah);
                        const float e = expf(-ah) * (1.f - al);             // exp(-|x|)
                        const float den = 1.f + e;
                        const float sg = (x >= 0.0 ? e : 1.f) / den;        // sigmoid(-x)
                        const double ws = w * (double)sg;
                        acc[r] += lead ? ws : -ws;
                        if (lead) lsum += w * ((x < 0.0 ? ab : 0.0) + (double)log1pf(e));
                    }
                }
            }
        }
        // ---- results ----------------------------------------------------------------------------------------------------------
        const bool ranknet = !lambda;
        const double inv_np = (ranknet && npairs > 0) ? 1.0 / (double)npairs : 1.0;
        double lloss = pair_group_sum<L>(lsum) * inv_np;
        const double qnan = __builtin_nan("");
        if (has_nan) lloss = qnan;
        if (npairs == 0 && !has_nan) lloss = 0.0;
        if (a.dscore) {
            const double gs = a.gscale ? (double)a.gscale[0] : 1.0;
            const double c = -a.sigma * (gs / (double)B) * inv_np;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = hl + r * L;
                if (live && i < S) a.dscore[base + i] = has_nan ? (float)qnan : (npairs > 0 ? (float)(c * acc[r]) : 0.f);
            }
        }
        if (live && hl == 0) {
            if (a.loss_per_list) a.loss_per_list[pb + grp] = (float)lloss;
            if (a.n_pairs) a.n_pairs[pb + grp] = npairs;
        }
#pragma unroll
        for (int g = 0; g < LPW; ++g) {         // the wavefront's lists in their order
            const double lg = __shfl(lloss, g * L);
            if (pb + g < B) wave_loss += lg;
        }
        __builtin_amdgcn_wave_barrier();        // the next list's records come after these reads
    }
    if (lane == 0) srec[wv] = wave_loss;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) t += srec[w];
        a.records[blockIdx.x] = t;
    }
}

// the records in a fixed order: thread t adds records t, t + 256, ... in turn, then the halving tree over the threads
__global__ __launch_bounds__(256) void pair_rank_final_kernel(const double* __restrict__ rec, int n, double B,
                                                              float* __restrict__ loss_out) {
    __shared__ double sm[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += rec[i];
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = (float)(sm[0] / B);
}

// lists per workgroup: 16 (S <= 64), 8 (<= 128), 4 (<= 512), 2 (<= 1024)
int pair_lists_per_group(int S) { return S <= 64 ? 16 : S <= 128 ? 8 : S <= 512 ? 4 : 2; }
int pair_grid(int B, int S) {
    const int groups = rlt_cdiv(B, pair_lists_per_group(S));
    return groups < PR_MAX_GRID ? groups : PR_MAX_GRID;
}

}  // namespace

extern "C" {

size_t rlt_pair_rank_workspace(int B, int S) {
    if (B <= 0 || S <= 0 || S > PR_MAX_S) return 0;
    const int groups = rlt_cdiv(B, 2);                          // the largest grid of any layout
    return (size_t)(groups < PR_MAX_GRID ? groups : PR_MAX_GRID) * sizeof(double);
}

int rlt_pair_rank_loss(const float* score, const float* labels, int B, int S, int kind, float sigma,
                       const float* gain, int n_grades, int normalize,
                       const void* dcg_table, const float* gscale,
                       float* loss_per_list, float* loss_out, float* dscore,
                       int32_t* rank_out, int32_t* n_pairs, void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(score && labels && ws);
    RLT_CHECK_ARG(B > 0 && S > 0);
    RLT_CHECK_ARG(kind == RLT_PAIR_RANKNET || kind == RLT_PAIR_LAMBDARANK);
    RLT_CHECK_ARG(std::isfinite(sigma) && sigma > 0.f);
    RLT_CHECK_ARG(n_grades >= 2 && n_grades <= RLT_REWARD_MAX_GRADES);
    rlt_reward_spec spec{};
    spec.family = RLT_REWARD_GAIN;
    spec.n_grades = n_grades;
    spec.normalize = normalize ? 1 : 0;
    for (int g = 0; g < n_grades; ++g) {
        spec.gain[g] = gain ? gain[g] : (float)((1 << g) - 1);
        RLT_CHECK_ARG(std::isfinite(spec.gain[g]));
    }
    RLT_CHECK_ARG(kind == RLT_PAIR_RANKNET || dcg_table);
    RLT_CHECK_ARG(loss_per_list || loss_out || dscore || rank_out || n_pairs);
    RLT_CHECK_SHAPE(S <= PR_MAX_S);
    if ((((uintptr_t)ws | (uintptr_t)dcg_table) & 7u) != 0 ||
        (((uintptr_t)score | (uintptr_t)labels | (uintptr_t)gscale | (uintptr_t)loss_per_list | (uintptr_t)loss_out |
          (uintptr_t)dscore | (uintptr_t)rank_out | (uintptr_t)n_pairs) & 3u) != 0)
        return RLT_E_ALIGN;
    if (ws_bytes < rlt_pair_rank_workspace(B, S)) return RLT_E_WORKSPACE;
    // the order in which the ideal list takes the grades: the one definition of rlt_reward_spec (reward_form.h)
    // (RANKNET reads no table; any_spec only wants to see one)
    RewardSrc rs{};
    static const double no_table[1] = {0.0};
    const int rc0 = any_spec(&spec, dcg_table ? dcg_table : (const void*)no_table, rs);
    if (rc0) return rc0;
    PairArgs a{};
    a.score = score; a.labels = labels;
    a.tab = kind == RLT_PAIR_LAMBDARANK ? (const double*)dcg_table : nullptr;
    a.gscale = gscale;
    a.loss_per_list = loss_per_list; a.dscore = dscore; a.rank_out = rank_out; a.n_pairs = n_pairs;
    a.records = (double*)ws;
    a.B = B; a.S = S; a.kind = kind; a.n_grades = n_grades; a.normalize = spec.normalize; a.n_take = rs.n_take;
    for (int g = 0; g < RLT_REWARD_MAX_GRADES; ++g) { a.order[g] = rs.order[g]; a.gain[g] = rs.gain[g]; }
    a.sigma = (double)sigma;
    a.want_loss = (loss_per_list || loss_out) ? 1 : 0;
    hipStream_t st = rlt_stream(stream);
    const int grid = pair_grid(B, S);
    if (S <= 64) hipLaunchKernelGGL((pair_rank_kernel<16, 4, 4>), dim3(grid), dim3(256), 0, st, a);
    else if (S <= 128) hipLaunchKernelGGL((pair_rank_kernel<32, 4, 4>), dim3(grid), dim3(256), 0, st, a);
    else if (S <= 256) hipLaunchKernelGGL((pair_rank_kernel<64, 4, 4>), dim3(grid), dim3(256), 0, st, a);
    else if (S <= 512) hipLaunchKernelGGL((pair_rank_kernel<64, 8, 4>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pair_rank_kernel<64, 16, 2>), dim3(grid), dim3(128), 0, st, a);
    int rc = RLT_LAUNCH_RESULT();
    if (rc) return rc;
    if (loss_out) {
        hipLaunchKernelGGL(pair_rank_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, grid, (double)B, loss_out);
        rc = RLT_LAUNCH_RESULT();
    }
    return rc;
}

}  // extern "C"
