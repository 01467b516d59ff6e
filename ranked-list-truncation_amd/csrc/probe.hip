// Probe heads of the probing study (models/Probe.py:30-53,102-122, models/Classification.py:4-12, models/Rerank.py:4-12, as
// verify_BMT.py and verify_probe.py train them): up to 8 Linear(E,1) heads on frozen position-major features x (S*B, E),
// each ending in
//   RLT_PROBE_BCE     Sigmoid -> nn.BCELoss() (mean over B*S), or
//   RLT_PROBE_RERANK  Softmax over the S positions of a list -> RerankLoss (utils/losses.py:99-141, batch-wide hinge),
// forward, loss and the weight gradients in one read of x.  No dx: the features are frozen.
//
// One workgroup per list, its four wavefronts taking groups of G consecutive positions in turn.  A wavefront loads the G rows
// (E floats each, 16-byte loads where E allows), forms the G logits of every head with one wavefront reduction each, and
// spreads the G scalar tails (sigmoid, log, exp) over G lanes instead of running them on all 64.  While the rows are still in
// registers it accumulates
//   BCE head:    sum_i gz_i x_i, gz_i = torch's BCE backward (1e-12 clamp, / (B*S)) times the sigmoid backward;
//   rerank head: online-softmax sums P = sum_i e^{z_i-m} x_i and Pv = sum_{y_i=1} e^{z_i-m} x_i, rescaled when the running
//                max m rises.  With 0/1 labels the softmax backward of the hinge's d/ds (g_i = gpos or gneg) is
//                dz_i = s_i (g_i - sum_j s_j g_j) = (gpos - gneg) s_i (y_i - V), V = sum_j s_j y_j, so the list's whole
//                contribution to dw is (gpos - gneg) (Pv - V P) / Z: one E-vector, scaled once the batch counts are known.
// The wavefronts' states are merged in a fixed order into one record per list; rlt_rows_reduce_kernel sums the records in a
// fixed order and a one-workgroup kernel forms the losses (rlt_rerank_hinge: the arithmetic of rlt_mt_terms) and scales dw.
// No atomics: bitwise reproducible.
#include "common.h"
#include "mt_terms.h"

namespace {

constexpr int MAXS = 1024, MAXE = 1024, MAXH = 8;

struct ProbeKinds { int k[MAXH]; };

// record of one list (floats): [nh*E dw partials][nh db partials][nh x 2 loss sums][n_pos, n_neg]
__host__ __device__ inline int probe_record_width(int nh, int E) { return nh * E + 3 * nh + 2; }

template <int V>
__device__ __forceinline__ void load_cols(const float* row, int col, int E, float (&d)[V]) {
    if constexpr (V == 4) {
        if (col < E) {
            const float4 v = *reinterpret_cast<const float4*>(row + col);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
            d[0] = d[1] = d[2] = d[3] = 0.f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) d[i] = col + i < E ? row[col + i] : 0.f;
    }
}

// V: floats per lane and load (4 when E % 4 == 0 and x is 16-byte aligned), NC: column chunks of 64 V per lane,
// NHM: heads held in registers (>= nh), G: positions per wavefront step
template <int V, int NC, int NHM, int G>
__global__ __launch_bounds__(256) void probe_pass_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, ProbeKinds kinds, int nh,
                                                         int S, int B, int E, const float* __restrict__ labels,
                                                         float* __restrict__ out, float* __restrict__ rec) {
    constexpr int CW = NC * 64 * V;                    // columns covered by one wavefront
    __shared__ float zs[NHM][MAXS];                    // sigmoid (BCE) or logit (rerank) per position, for `out`
    __shared__ float red[4][CW];
    __shared__ float wst[4][NHM][5];                   // per wavefront: m, Z, sum e*[y=1], sum e*[y=0], BCE loss
    __shared__ float wdb[4][NHM];
    __shared__ float wcnt[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const float inv_n = 1.f / ((float)B * (float)S);
    const float* yrow = labels + (size_t)b * S;

    float wr[NHM][NC][V], acc[NHM][NC][V], accv[NHM][NC][V];
    float m[NHM], zsum[NHM], epos[NHM], eneg[NHM], lsum[NHM], dsum[NHM], bh[NHM];
    int kd[NHM];
#pragma unroll
    for (int h = 0; h < NHM; ++h) {
        kd[h] = h < nh ? kinds.k[h] : RLT_PROBE_BCE;
        bh[h] = h < nh ? bias[h] : 0.f;
        m[h] = -INFINITY; zsum[h] = 0.f; epos[h] = 0.f; eneg[h] = 0.f; lsum[h] = 0.f; dsum[h] = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int col = c * 64 * V + lane * V + i;
                wr[h][c][i] = (h < nh && col < E) ? w[(size_t)h * E + col] : 0.f;
                acc[h][c][i] = 0.f;
                accv[h][c][i] = 0.f;
            }
    }
    float npos = 0.f, nneg = 0.f;

    for (int s0 = wv * G; s0 < S; s0 += 4 * G) {
        float xv[G][NC][V];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const int s = s0 + k;
            const float* row = x + ((size_t)(s < S ? s : 0) * B + b) * E;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (s < S) load_cols<V>(row, c * 64 * V + lane * V, E, xv[k][c]);
                else {
#pragma unroll
                    for (int i = 0; i < V; ++i) xv[k][c][i] = 0.f;
                }
            }
        }
        // lane k < G owns position s0 + k for the scalar tails
        const int kl = lane & (G - 1);
        const bool own = lane < G && s0 + lane < S;
        const float tl = own ? yrow[s0 + lane] : 0.f;
        if (own) { npos += tl == 1.f ? 1.f : 0.f; nneg += tl == 0.f ? 1.f : 0.f; }
        const bool posl = tl == 1.f;
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            if (h >= nh) continue;
            float zk[G];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int i = 0; i < V; ++i) d += xv[k][c][i] * wr[h][c][i];
                zk[k] = s0 + k < S ? wave_sum(d) + bh[h] : -INFINITY;
            }
            float zl = zk[0];
#pragma unroll
            for (int k = 1; k < G; ++k) zl = kl == k ? zk[k] : zl;
            if (kd[h] == RLT_PROBE_BCE) {
                const float sg = 1.f / (1.f + expf(-zl));
                float gz = 0.f;
                if (own) {
                    lsum[h] += rlt_bce_term(sg, tl);
                    gz = rlt_bce_dgrad(sg, tl) * inv_n * (1.f - sg) * sg;   // BCE backward (mean), then sigmoid backward
                    dsum[h] += gz;
                    zs[h][s0 + lane] = sg;
                }
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const float g = rlt_readlane(gz, k);
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int i = 0; i < V; ++i) acc[h][c][i] += g * xv[k][c][i];
                }
            } else {
                float mk = zk[0];
#pragma unroll
                for (int k = 1; k < G; ++k) mk = fmaxf(mk, zk[k]);
                if (mk > m[h]) {                       // wave-uniform: rescale the sums to the new maximum
                    const float sc = m[h] == -INFINITY ? 0.f : expf(m[h] - mk);
                    zsum[h] *= sc; epos[h] *= sc; eneg[h] *= sc;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int i = 0; i < V; ++i) { acc[h][c][i] *= sc; accv[h][c][i] *= sc; }
                    m[h] = mk;
                }
                const float el = own ? expf(zl - m[h]) : 0.f;
                if (own) zs[h][s0 + lane] = zl;
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const float e = rlt_readlane(el, k);
                    const bool pk = rlt_readlane((int)posl, k) != 0;
                    const bool nk = rlt_readlane((int)(own && tl == 0.f), k) != 0;
                    zsum[h] += e;
                    if (pk) epos[h] += e;
                    if (nk) eneg[h] += e;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int i = 0; i < V; ++i) {
                            const float ex = e * xv[k][c][i];
                            acc[h][c][i] += ex;
                            if (pk) accv[h][c][i] += ex;
                        }
                }
            }
        }
    }

    // ---- per-wavefront scalars -> LDS, merged by every thread in a fixed order --------------------------------------
    npos = wave_sum(npos);
    nneg = wave_sum(nneg);
#pragma unroll
    for (int h = 0; h < NHM; ++h) {
        const float l = wave_sum(lsum[h]), d = wave_sum(dsum[h]);
        if (lane == 0 && h < nh) {
            wst[wv][h][0] = m[h]; wst[wv][h][1] = zsum[h]; wst[wv][h][2] = epos[h]; wst[wv][h][3] = eneg[h];
            wst[wv][h][4] = l;
            wdb[wv][h] = d;
        }
    }
    if (lane == 0) { wcnt[wv][0] = npos; wcnt[wv][1] = nneg; }
    __syncthreads();

    const int pw = probe_record_width(nh, E);
    float* r = rec + (size_t)b * pw;
    const int tid = threadIdx.x;
#pragma unroll
    for (int h = 0; h < NHM; ++h) {                    // compile-time h: the register arrays are never indexed at run time
        if (h >= nh) break;                            // block-uniform
        const bool rr = kd[h] == RLT_PROBE_RERANK;
        float M = -INFINITY, Z = 0.f, Vp = 0.f, Vn = 0.f, fw = 1.f;
        if (rr) {
            for (int q = 0; q < 4; ++q) M = fmaxf(M, wst[q][h][0]);
            for (int q = 0; q < 4; ++q) {
                const float f = wst[q][h][0] == -INFINITY ? 0.f : expf(wst[q][h][0] - M);
                Z += f * wst[q][h][1];
                Vp += f * wst[q][h][2];
                Vn += f * wst[q][h][3];
                if (q == wv) fw = f;
            }
        }
        const float rz = rr ? 1.f / Z : 0.f;
        const float vbar = Vp * rz;                    // V = sum_j s_j [y_j = 1]
        // vector merge: a rerank head needs Pv, then P; a BCE head its gradient sum
        float keep[MAXE / 256];
        for (int pass = 0; pass < (rr ? 2 : 1); ++pass) {
            const bool pv = rr && pass == 0;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int i = 0; i < V; ++i) red[wv][c * 64 * V + lane * V + i] = fw * (pv ? accv[h][c][i] : acc[h][c][i]);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < MAXE / 256; ++j) {
                const int col = tid + 256 * j;
                if (col < E) {
                    const float t = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
                    if (!rr) r[h * E + col] = t;
                    else if (pv) keep[j] = t;
                    else r[h * E + col] = (keep[j] - vbar * t) * rz;     // (Pv - V P) / Z
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            r[nh * E + h] = rr ? 0.f : ((wdb[0][h] + wdb[1][h]) + wdb[2][h]) + wdb[3][h];   // a softmax head's db is 0
            r[nh * E + nh + 2 * h] = rr ? Vp * rz : ((wst[0][h][4] + wst[1][h][4]) + wst[2][h][4]) + wst[3][h][4];
            r[nh * E + nh + 2 * h + 1] = rr ? Vn * rz : 0.f;
        }
        if (out) {
            float* dst = out + ((size_t)h * B + b) * S;
            for (int s = tid; s < S; s += 256) dst[s] = rr ? expf(zs[h][s] - M) * rz : zs[h][s];
        }
    }
    if (tid == 0) {
        r[nh * E + 3 * nh] = ((wcnt[0][0] + wcnt[1][0]) + wcnt[2][0]) + wcnt[3][0];
        r[nh * E + 3 * nh + 1] = ((wcnt[0][1] + wcnt[1][1]) + wcnt[2][1]) + wcnt[3][1];
    }
}

// losses and the scaling of the rerank heads' gradients, from the column sums of the records
__global__ __launch_bounds__(256) void probe_final_kernel(const float* __restrict__ sums, ProbeKinds kinds, int nh, int S,
                                                          int B, int E, float margin, float* __restrict__ loss,
                                                          float* __restrict__ dw, float* __restrict__ db) {
    const double n_pos = sums[nh * E + 3 * nh], n_neg = sums[nh * E + 3 * nh + 1];
    for (int h = 0; h < nh; ++h) {
        const bool rr = kinds.k[h] == RLT_PROBE_RERANK;
        const float l0 = sums[nh * E + nh + 2 * h], l1 = sums[nh * E + nh + 2 * h + 1];
        float lh, scale = 1.f;
        if (rr) {
            float gpos, gneg;
            rlt_rerank_hinge((double)l0, n_pos, (double)l1, n_neg, margin, lh, gpos, gneg);
            scale = gpos - gneg;
        } else {
            lh = (float)((double)l0 / ((double)B * (double)S));
        }
        if (threadIdx.x == 0) loss[h] = lh;
        if (dw) {
            for (int col = threadIdx.x; col < E; col += 256) dw[(size_t)h * E + col] = rr ? scale * sums[h * E + col] : sums[h * E + col];
            if (threadIdx.x == 0) db[h] = rr ? scale * sums[nh * E + h] : sums[nh * E + h];
        }
    }
}

template <int V, int NC, int NHM, int G>
void launch_pass(const float* x, const float* w, const float* b, const ProbeKinds& k, int nh, int S, int B, int E,
                 const float* labels, float* out, float* rec, hipStream_t st) {
    hipLaunchKernelGGL((probe_pass_kernel<V, NC, NHM, G>), dim3(B), dim3(256), 0, st, x, w, b, k, nh, S, B, E, labels, out, rec);
}

// Register budget: the study's passes hold 1-2 heads (NHM = 2: no scratch at any E).  With 3-8 heads the E > 256 variants
// exceed the register file and spill to scratch - the results are the same, the pass is then far from HBM speed.
template <int NHM>
void dispatch_pass(bool v4, const float* x, const float* w, const float* b, const ProbeKinds& k, int nh, int S, int B,
                   int E, const float* labels, float* out, float* rec, hipStream_t st) {
    if (v4) {
        if (E <= 256) launch_pass<4, 1, NHM, 8>(x, w, b, k, nh, S, B, E, labels, out, rec, st);
        else launch_pass<4, 4, NHM, 2>(x, w, b, k, nh, S, B, E, labels, out, rec, st);
    } else {
        if (E <= 64) launch_pass<1, 1, NHM, 8>(x, w, b, k, nh, S, B, E, labels, out, rec, st);
        else if (E <= 256) launch_pass<1, 4, NHM, 8>(x, w, b, k, nh, S, B, E, labels, out, rec, st);
        else launch_pass<1, 16, NHM, 2>(x, w, b, k, nh, S, B, E, labels, out, rec, st);
    }
}

}  // namespace

extern "C" {

size_t rlt_probe_heads_workspace(int n_heads, int S, int B, int E) {
    if (n_heads < 1 || n_heads > MAXH || S < 1 || S > MAXS || B < 1 || E < 1 || E > MAXE) return 0;
    return ((size_t)B + 1) * (size_t)probe_record_width(n_heads, E) * sizeof(float);
}

int rlt_probe_heads(const float* x, const float* w, const float* b, const int* kinds, int n_heads,
                    int S, int B, int E, const float* labels, float margin,
                    float* loss, float* dw, float* db, float* out,
                    void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(x && w && b && kinds && labels && loss && ws && S > 0 && B > 0 && E > 0 && n_heads > 0);
    RLT_CHECK_ARG((dw == nullptr) == (db == nullptr));
    RLT_CHECK_SHAPE(n_heads <= MAXH && S <= MAXS && E <= MAXE);
    ProbeKinds pk;
    for (int i = 0; i < MAXH; ++i) {
        pk.k[i] = i < n_heads ? kinds[i] : RLT_PROBE_BCE;
        RLT_CHECK_ARG(pk.k[i] == RLT_PROBE_BCE || pk.k[i] == RLT_PROBE_RERANK);
    }
    if (ws_bytes < rlt_probe_heads_workspace(n_heads, S, B, E)) return RLT_E_WORKSPACE;
    hipStream_t st = rlt_stream(stream);
    const bool v4 = E % 4 == 0 && rlt_aligned16(x);
    const int pw = probe_record_width(n_heads, E);
    float* rec = (float*)ws;
    float* sums = rec + (size_t)B * pw;
    if (n_heads <= 2) dispatch_pass<2>(v4, x, w, b, pk, n_heads, S, B, E, labels, out, rec, st);
    else dispatch_pass<8>(v4, x, w, b, pk, n_heads, S, B, E, labels, out, rec, st);
    hipLaunchKernelGGL(rlt_rows_reduce_kernel, dim3(rlt_cdiv(pw, 16)), dim3(256), 0, st, (const float*)rec, B, pw, pw, pw,
                       sums, (float*)nullptr, 0);
    hipLaunchKernelGGL(probe_final_kernel, dim3(1), dim3(256), 0, st, (const float*)sums, pk, n_heads, S, B, E, margin,
                       loss, dw, db);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
