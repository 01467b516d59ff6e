// Paired significance tests between two or more per-query columns (one value per query and system, as run.py --report-out
// writes them): the Fisher sign-flip randomization test and the paired bootstrap, R resamples each, plus the moments the sign
// and t statistics need - all on the device, with a counter-based generator, so no R x Q index tensor ever exists.
//
//   d[q][m] = (double)sys[m][q] - (double)base[q]      exact in float64; a pair with a NaN / Inf member counts in `nonfinite`,
//                                                      gives d = 0 and stays out of n, the sums and wins / ties / losses
//   T_r = sum_q s(r,q) d[q][m]                         s = -1 where bit (q & 31) of word(r, q >> 5) is set, +1 otherwise
//   B_r = sum_{j<Q} d[idx(r,j)][m]                     idx(r,j) = (u(r,j) * Q) >> 32  (64-bit product of two 32-bit numbers)
//
// Generator (tests/compare_restate.py copies this arithmetic; mix32 and row_hash are the two functions of common.h):
//   draw(seed, r, c) = mix32(row_hash(seed, r) ^ mix32(c + 0x7F4A7C15))          all arithmetic mod 2^32
//   word(r, k) = draw(seed,  r, k)               k = q >> 5: 32 signs per draw
//   u(r, j)    = draw(seed', r, j)               seed' = mix32(seed ^ 0xA511E9B3)
// A pure function of (seed, r, c): no dependence on grid, lane or launch order; every system m sees the same signs and the same
// indices (common random numbers).  For a fixed r, c -> draw is a bijection of the 32-bit numbers, so the indices of one
// replicate come from Q distinct values of u; idx is floor(u Q / 2^32), whose probabilities differ from 1/Q by at most 2^-32
// (relative bias at most Q / 2^32 <= 1/64 at the largest Q, 2.4e-4 at 2^20 queries).
//
// Order of every sum (float64, fixed by Q, M and R alone - no float atomics, the same bits from every call):
//   * a replicate's sum over a chunk of queries [c C, min(Q, (c+1) C)) is formed by ONE wavefront: lane l adds the chunk's
//     positions l, l + 64, ... in ascending order, then the 64 lanes by the DPP scan of common.h; the chunks are then added in
//     ascending order by one lane.  The resident form is the one-chunk case (C >= Q).
//   * T_obs is replicate number R of the same kernel with word = 0 (all signs plus): same path, same order, so a replicate that
//     draws all plus - or all minus: IEEE negation commutes with rounding - has |T_r| == |T_obs| bit for bit.
//   * the moments are summed per chunk of MOM_CHUNK queries by one workgroup (per lane its 16 elements in order, the DPP scan,
//     the four wavefronts in order), the chunk records by one workgroup per system in the same way.  The squared deviations are
//     a second pass about mean = sum_d / n.
//   * the three counts are integers (64-bit integer atomics on the record: order cannot matter).
//
// Two forms (rlt_paired_compare_plan):
//   resident  Q M 8 <= 160 KB: d sits in LDS as [q][m]; a 1024-lane workgroup fills it once and walks 16 * rpw replicates, a
//             wavefront per replicate; signs and gathers both read LDS (ds_read_b64 per system, the M values of a query adjacent).
//   chunked   grid = replicates x chunks of C = 32768 queries, a wavefront per (replicate, chunk), 256-lane workgroups and no LDS:
//             the sign pass reads its chunk of d coalesced (the chunk, C M 8 bytes, is shared by all replicates and stays in L2), the
//             bootstrap gathers range over all Q and go through L2 / global memory; [q][m] keeps the M values of a draw in one line.
#include "common.h"

namespace {

constexpr int LDS_BYTES = 160 * 1024;            // gfx950: what one workgroup may own
constexpr int RES_LANES = 1024, RES_WAVES = RES_LANES / 64;
constexpr int CH_LANES = 256, CH_WAVES = CH_LANES / 64;
constexpr int CHUNK = RLT_COMPARE_CHUNK;         // queries per chunk of the chunked form
constexpr int MOM_CHUNK = 4096;                  // queries per moment record: 256 lanes x 16
constexpr int MAX_Q = 1 << 26, MAX_M = RLT_COMPARE_MAX_SYSTEMS, MAX_R = 1 << 20;
typedef struct rlt_paired_compare_plan Plan;
static_assert(CHUNK % 64 == 0 && CHUNK > LDS_BYTES / 8 + 1, "a chunk is whole wavefront strides and larger than any resident Q");

// ---------------------------------------------------------------- the generator
__host__ __device__ __forceinline__ uint32_t cmp_draw_key(uint32_t key, uint32_t c) { return rlt_mix32(key ^ rlt_mix32(c + 0x7F4A7C15U)); }
__host__ __device__ __forceinline__ uint32_t cmp_draw(uint32_t seed, uint32_t r, uint32_t c) { return cmp_draw_key(rlt_row_hash(seed, r), c); }
__host__ __device__ __forceinline__ uint32_t cmp_boot_seed(uint32_t seed) { return rlt_mix32(seed ^ 0xA511E9B3U); }
__host__ __device__ __forceinline__ uint32_t cmp_index(uint32_t u, uint32_t Q) { return (uint32_t)(((uint64_t)u * (uint64_t)Q) >> 32); }

// ---------------------------------------------------------------- moments
struct Mom { double sb, ss, sd; long long n, win, tie, loss, bad; };
static_assert(sizeof(Mom) == 64, "workspace layout");

__device__ __forceinline__ Mom mom_zero() { return Mom{0.0, 0.0, 0.0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ void mom_add(Mom& a, const Mom& b) {
    a.sb += b.sb; a.ss += b.ss; a.sd += b.sd;
    a.n += b.n; a.win += b.win; a.tie += b.tie; a.loss += b.loss; a.bad += b.bad;
}
__device__ __forceinline__ Mom mom_wave(const Mom& f) {
    Mom r;
    r.sb = wave_sum(f.sb); r.ss = wave_sum(f.ss); r.sd = wave_sum(f.sd);
    r.n = wave_sum(f.n); r.win = wave_sum(f.win); r.tie = wave_sum(f.tie); r.loss = wave_sum(f.loss); r.bad = wave_sum(f.bad);
    return r;
}
__device__ __forceinline__ bool cmp_finite(float x) { return fabsf(x) < INFINITY; }      // false for NaN

// pass 1, grid (moment chunks, M): d[q][m] and one record per (m, chunk)
__global__ __launch_bounds__(256) void cmp_prep_kernel(const float* __restrict__ base, const float* __restrict__ sys, int ld, int Q, int M,
                                                       double* __restrict__ d, Mom* __restrict__ part) {
    __shared__ Mom red[4];
    const int m = blockIdx.y, c = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Mom t = mom_zero();
    for (int i = 0; i < MOM_CHUNK / 256; ++i) {
        const int q = c * MOM_CHUNK + i * 256 + (int)threadIdx.x;
        if (q < Q) {
            const float b = base[q], s = sys[(size_t)m * ld + q];
            const bool ok = cmp_finite(b) && cmp_finite(s);
            const double dv = ok ? (double)s - (double)b : 0.0;
            d[(size_t)q * M + m] = dv;
            if (ok) {
                t.sb += (double)b; t.ss += (double)s; t.sd += dv;
                t.n += 1; t.win += dv > 0.0; t.tie += dv == 0.0; t.loss += dv < 0.0;
            } else {
                t.bad += 1;
            }
        }
    }
    t = mom_wave(t);
    if (lane == 0) red[wv] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        Mom r = red[0];
        mom_add(r, red[1]); mom_add(r, red[2]); mom_add(r, red[3]);
        part[(size_t)m * gridDim.x + c] = r;
    }
}

// grid M: the chunk records of a system in order -> its record (every word of it: the counts start from zero here)
__global__ __launch_bounds__(256) void cmp_moments_kernel(const Mom* __restrict__ part, int n_rec, int R, int form, long long* __restrict__ record) {
    __shared__ Mom red[4];
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Mom t = mom_zero();
    for (int c = threadIdx.x; c < n_rec; c += 256) mom_add(t, part[(size_t)m * n_rec + c]);
    t = mom_wave(t);
    if (lane == 0) red[wv] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    Mom r = red[0];
    mom_add(r, red[1]); mom_add(r, red[2]); mom_add(r, red[3]);
    long long* w = record + (size_t)m * RLT_CMP_WORDS;
    double* f = reinterpret_cast<double*>(w);
    w[RLT_CMP_N] = r.n; f[RLT_CMP_SUM_BASE] = r.sb; f[RLT_CMP_SUM_SYS] = r.ss; f[RLT_CMP_SUM_D] = r.sd; f[RLT_CMP_SSD] = 0.0;
    w[RLT_CMP_WINS] = r.win; w[RLT_CMP_TIES] = r.tie; w[RLT_CMP_LOSSES] = r.loss; w[RLT_CMP_NONFINITE] = r.bad;
    f[RLT_CMP_T_OBS] = 0.0; w[RLT_CMP_RAND_GE] = 0; w[RLT_CMP_BOOT_LE0] = 0; w[RLT_CMP_BOOT_GE0] = 0;
    w[RLT_CMP_RESAMPLES] = R; w[RLT_CMP_FORM] = form; w[RLT_CMP_RESERVED] = 0;
}

// pass 2, grid (moment chunks, M): squared deviations about the mean of the record
__global__ __launch_bounds__(256) void cmp_dev_kernel(const float* __restrict__ base, const float* __restrict__ sys, int ld, int Q,
                                                      const long long* __restrict__ record, double* __restrict__ part) {
    __shared__ double red[4];
    const int m = blockIdx.y, c = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long n = record[(size_t)m * RLT_CMP_WORDS + RLT_CMP_N];
    const double mean = n > 0 ? reinterpret_cast<const double*>(record)[(size_t)m * RLT_CMP_WORDS + RLT_CMP_SUM_D] / (double)n : 0.0;
    double t = 0.0;
    for (int i = 0; i < MOM_CHUNK / 256; ++i) {
        const int q = c * MOM_CHUNK + i * 256 + (int)threadIdx.x;
        if (q < Q) {
            const float b = base[q], s = sys[(size_t)m * ld + q];
            if (cmp_finite(b) && cmp_finite(s)) {
                const double e = ((double)s - (double)b) - mean;
                t += e * e;
            }
        }
    }
    t = wave_sum(t);
    if (lane == 0) red[wv] = t;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)m * gridDim.x + c] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void cmp_dev_sum_kernel(const double* __restrict__ part, int n_rec, long long* __restrict__ record) {
    __shared__ double red[4];
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double t = 0.0;
    for (int c = threadIdx.x; c < n_rec; c += 256) t += part[(size_t)m * n_rec + c];
    t = wave_sum(t);
    if (lane == 0) red[wv] = t;
    __syncthreads();
    if (threadIdx.x == 0) reinterpret_cast<double*>(record)[(size_t)m * RLT_CMP_WORDS + RLT_CMP_SSD] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------- the resampling pass
// One wavefront, one replicate r in [0, R] (r == R: the observed statistic), one chunk [q0, q0 + cn) of the queries: the two sums
// of every system, the same value in every lane.  `src` is where the chunk's d[q0 ..][m] is read (LDS or global), `all` where
// d[0 .. Q)[m] is gathered from.  Every index is below Q by construction (u < 2^32), every chunk position below cn.
template <int M>
__device__ __forceinline__ void cmp_replicate(const double* __restrict__ src, const double* __restrict__ all, int q0, int cn, int Q, int r, int R,
                                              uint32_t seed, uint32_t seed_b, int lane, double (&T)[M], double (&B)[M]) {
    const bool obs = r == R;
    const uint32_t key = rlt_row_hash(seed, (uint32_t)r), key_b = rlt_row_hash(seed_b, (uint32_t)r);
    double a[M], b[M];
#pragma unroll
    for (int m = 0; m < M; ++m) { a[m] = 0.0; b[m] = 0.0; }
    for (int j = lane; j < cn; j += 64) {
        const uint32_t q = (uint32_t)(q0 + j);
        const uint32_t w = obs ? 0u : cmp_draw_key(key, q >> 5);
        const bool neg = (w >> (q & 31u)) & 1u;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double v = src[(size_t)j * M + m];
            a[m] += neg ? -v : v;
        }
    }
    if (!obs) {
        for (int j = lane; j < cn; j += 64) {
            const uint32_t idx = cmp_index(cmp_draw_key(key_b, (uint32_t)(q0 + j)), (uint32_t)Q);
#pragma unroll
            for (int m = 0; m < M; ++m) b[m] += all[(size_t)idx * M + m];
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) { T[m] = wave_sum(a[m]); B[m] = wave_sum(b[m]); }
}

// resident: grid = cdiv(R + 1, 16 rpw) workgroups of 16 wavefronts, wavefront w of workgroup g takes replicates (16 g + w) rpw + k
template <int M>
__global__ __launch_bounds__(RES_LANES) void cmp_resident_kernel(const double* __restrict__ d, int Q, int R, int rpw, uint32_t seed, uint32_t seed_b,
                                                                 double* __restrict__ part_rand, double* __restrict__ part_boot) {
    extern __shared__ double cmp_lds[];           // [Q][M]
    for (int i = threadIdx.x; i < Q * M; i += RES_LANES) cmp_lds[i] = d[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < rpw; ++k) {
        const int r = ((int)blockIdx.x * RES_WAVES + wv) * rpw + k;       // wave-uniform
        if (r > R) break;
        double T[M], B[M];
        cmp_replicate<M>(cmp_lds, cmp_lds, 0, Q, Q, r, R, seed, seed_b, lane, T, B);
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                part_rand[(size_t)m * (R + 1) + r] = T[m];
                part_boot[(size_t)m * (R + 1) + r] = B[m];
            }
        }
    }
}

// chunked: grid (cdiv(R + 1, 4), chunks), a wavefront per (replicate, chunk); partials [chunk][m][r]
template <int M>
__global__ __launch_bounds__(CH_LANES) void cmp_chunked_kernel(const double* __restrict__ d, int Q, int R, uint32_t seed, uint32_t seed_b,
                                                               double* __restrict__ part_rand, double* __restrict__ part_boot) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = (int)blockIdx.x * CH_WAVES + wv;                          // wave-uniform
    if (r > R) return;
    const int c = blockIdx.y;
    const int q0 = c * CHUNK;
    const int cn = Q - q0 < CHUNK ? Q - q0 : CHUNK;
    double T[M], B[M];
    cmp_replicate<M>(d + (size_t)q0 * M, d, q0, cn, Q, r, R, seed, seed_b, lane, T, B);
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            part_rand[((size_t)c * M + m) * (R + 1) + r] = T[m];
            part_boot[((size_t)c * M + m) * (R + 1) + r] = B[m];
        }
    }
}

// grid (cdiv(R + 1, 256), M): a lane per replicate adds the chunks in ascending order
__global__ __launch_bounds__(256) void cmp_chunks_sum_kernel(const double* __restrict__ part_rand, const double* __restrict__ part_boot, int chunks,
                                                             int M, int R, double* __restrict__ fin_rand, double* __restrict__ fin_boot,
                                                             double* __restrict__ rand_stat, double* __restrict__ boot_stat) {
    const int r = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (r > R) return;
    double t = 0.0, b = 0.0;
    for (int c = 0; c < chunks; ++c) {
        t += part_rand[((size_t)c * M + m) * (R + 1) + r];
        b += part_boot[((size_t)c * M + m) * (R + 1) + r];
    }
    fin_rand[(size_t)m * (R + 1) + r] = t;
    fin_boot[(size_t)m * (R + 1) + r] = b;
    if (r < R) {
        if (rand_stat) rand_stat[(size_t)m * R + r] = t;
        if (boot_stat) boot_stat[(size_t)m * R + r] = b;
    }
}

// grid (max(1, cdiv(R, 256)), M): the three counts and T_obs into the record
__global__ __launch_bounds__(256) void cmp_count_kernel(const double* __restrict__ fin_rand, const double* __restrict__ fin_boot, int R,
                                                        long long* __restrict__ record) {
    __shared__ long long red[4][3];
    const int r = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double t_obs = fin_rand[(size_t)m * (R + 1) + R];
    long long ge = 0, le0 = 0, ge0 = 0;
    if (r < R) {
        const double t = fin_rand[(size_t)m * (R + 1) + r], b = fin_boot[(size_t)m * (R + 1) + r];
        ge = fabs(t) >= fabs(t_obs);
        le0 = b <= 0.0;
        ge0 = b >= 0.0;
    }
    ge = wave_sum(ge); le0 = wave_sum(le0); ge0 = wave_sum(ge0);
    if (lane == 0) { red[wv][0] = ge; red[wv][1] = le0; red[wv][2] = ge0; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long* w = record + (size_t)m * RLT_CMP_WORDS;
    if (blockIdx.x == 0) reinterpret_cast<double*>(w)[RLT_CMP_T_OBS] = t_obs;
    const int words[3] = {RLT_CMP_RAND_GE, RLT_CMP_BOOT_LE0, RLT_CMP_BOOT_GE0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const long long v = red[0][i] + red[1][i] + red[2][i] + red[3][i];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(w + words[i]), (unsigned long long)v);
    }
}

// ---------------------------------------------------------------- plan, workspace, launch
inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline bool dims_ok(int Q, int M, int R) { return Q >= 1 && Q <= MAX_Q && M >= 1 && M <= MAX_M && R >= 0 && R <= MAX_R; }

void make_plan(int Q, int M, int R, Plan* p) {
    p->resident_max_q = LDS_BYTES / (8 * M);
    p->chunk = CHUNK;
    if (Q <= p->resident_max_q) {
        p->form = RLT_COMPARE_RESIDENT;
        p->chunks = 1;
        p->lds_bytes = Q * M * 8;
        // replicates per wavefront: as many as still leave 1024 workgroups (the fill of the LDS image is paid once per workgroup)
        p->replicates_per_wave = 1;
        for (int rpw = 16; rpw > 1; rpw /= 4)
            if (((long long)R + 1 + RES_WAVES * rpw - 1) / (RES_WAVES * rpw) >= 1024) { p->replicates_per_wave = rpw; break; }
    } else {
        p->form = RLT_COMPARE_CHUNKED;
        p->chunks = (Q + CHUNK - 1) / CHUNK;
        p->lds_bytes = 0;
        p->replicates_per_wave = 1;
    }
}

struct Layout { size_t d, part_rand, part_boot, fin_rand, fin_boot, mom, dev, total; };
Layout make_layout(int Q, int M, int R, const Plan& p) {
    Layout l;
    const size_t r1 = (size_t)R + 1, n_rec = ((size_t)Q + MOM_CHUNK - 1) / MOM_CHUNK;
    size_t o = 0;
    l.d = o;         o += up16((size_t)Q * M * 8);
    l.part_rand = o; o += up16((size_t)p.chunks * M * r1 * 8);
    l.part_boot = o; o += up16((size_t)p.chunks * M * r1 * 8);
    l.fin_rand = o;  o += up16((size_t)M * r1 * 8);
    l.fin_boot = o;  o += up16((size_t)M * r1 * 8);
    l.mom = o;       o += up16((size_t)M * n_rec * sizeof(Mom));
    l.dev = o;       o += up16((size_t)M * n_rec * 8);
    l.total = o;
    return l;
}

template <int M>
int launch_resample(const Plan& p, const double* d, int Q, int R, uint32_t seed, double* part_rand, double* part_boot,
                    hipStream_t st) {
    const uint32_t seed_b = cmp_boot_seed(seed);
    if (p.form == RLT_COMPARE_RESIDENT) {
        const int rc = rlt_allow_lds(cmp_resident_kernel<M>, (size_t)p.lds_bytes);
        if (rc) return rc;
        const int per = RES_WAVES * p.replicates_per_wave;
        hipLaunchKernelGGL(cmp_resident_kernel<M>, dim3((unsigned)((R + 1 + per - 1) / per)), dim3(RES_LANES), (size_t)p.lds_bytes, st, d, Q, R,
                           p.replicates_per_wave, seed, seed_b, part_rand, part_boot);
    } else {
        hipLaunchKernelGGL(cmp_chunked_kernel<M>, dim3((unsigned)((R + 1 + CH_WAVES - 1) / CH_WAVES), (unsigned)p.chunks), dim3(CH_LANES), 0, st, d, Q, R,
                           seed, seed_b, part_rand, part_boot);
    }
    return 0;
}

}  // namespace

extern "C" {

int rlt_paired_compare_plan(int Q, int M, int R, struct rlt_paired_compare_plan* out) {
    RLT_CHECK_ARG(out && Q >= 1 && M >= 1 && R >= 0);
    RLT_CHECK_SHAPE(dims_ok(Q, M, R));
    make_plan(Q, M, R, out);
    return 0;
}

size_t rlt_paired_compare_workspace(int Q, int M, int R) {
    if (!dims_ok(Q, M, R)) return 0;
    Plan p;
    make_plan(Q, M, R, &p);
    return make_layout(Q, M, R, p).total;
}

int rlt_paired_compare(const float* base, const float* sys, int ld, int Q, int M, int R, uint32_t seed, void* ws, size_t ws_bytes,
                       int64_t* record, double* rand_stat, double* boot_stat, void* stream) {
    RLT_CHECK_ARG(base && sys && ws && record && Q >= 1 && M >= 1 && R >= 0 && ld >= Q);
    RLT_CHECK_SHAPE(dims_ok(Q, M, R));
    if (((uintptr_t)base & 3u) || ((uintptr_t)sys & 3u) || ((uintptr_t)record & 7u) || ((uintptr_t)rand_stat & 7u) || ((uintptr_t)boot_stat & 7u))
        return RLT_E_ALIGN;
    Plan p;
    make_plan(Q, M, R, &p);
    const Layout l = make_layout(Q, M, R, p);
    if (!rlt_aligned16(ws) || ws_bytes < l.total) return RLT_E_WORKSPACE;
    char* w = (char*)ws;
    double* d = (double*)(w + l.d);
    double *part_rand = (double*)(w + l.part_rand), *part_boot = (double*)(w + l.part_boot);
    double *fin_rand = (double*)(w + l.fin_rand), *fin_boot = (double*)(w + l.fin_boot);
    Mom* mom = (Mom*)(w + l.mom);
    double* dev = (double*)(w + l.dev);
    long long* rec = (long long*)record;
    hipStream_t st = rlt_stream(stream);
    const int n_rec = (Q + MOM_CHUNK - 1) / MOM_CHUNK;
    hipLaunchKernelGGL(cmp_prep_kernel, dim3((unsigned)n_rec, (unsigned)M), dim3(256), 0, st, base, sys, ld, Q, M, d, mom);
    hipLaunchKernelGGL(cmp_moments_kernel, dim3((unsigned)M), dim3(256), 0, st, (const Mom*)mom, n_rec, R, p.form, rec);
    hipLaunchKernelGGL(cmp_dev_kernel, dim3((unsigned)n_rec, (unsigned)M), dim3(256), 0, st, base, sys, ld, Q, (const long long*)rec, dev);
    hipLaunchKernelGGL(cmp_dev_sum_kernel, dim3((unsigned)M), dim3(256), 0, st, (const double*)dev, n_rec, rec);
    int rc = 0;
    switch (M) {
        case 1: rc = launch_resample<1>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        case 2: rc = launch_resample<2>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        case 3: rc = launch_resample<3>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        case 4: rc = launch_resample<4>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        case 5: rc = launch_resample<5>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        case 6: rc = launch_resample<6>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        case 7: rc = launch_resample<7>(p, d, Q, R, seed, part_rand, part_boot, st); break;
        default: rc = launch_resample<8>(p, d, Q, R, seed, part_rand, part_boot, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(cmp_chunks_sum_kernel, dim3((unsigned)((R + 1 + 255) / 256), (unsigned)M), dim3(256), 0, st, (const double*)part_rand,
                       (const double*)part_boot, p.chunks, M, R, fin_rand, fin_boot, rand_stat, boot_stat);
    hipLaunchKernelGGL(cmp_count_kernel, dim3((unsigned)(R > 0 ? (R + 255) / 256 : 1), (unsigned)M), dim3(256), 0, st, (const double*)fin_rand,
                       (const double*)fin_boot, R, rec);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
