// Hazard cut head: one Linear(E,1) head whose logit z_s is a stop logit, turned into a cut distribution by the discrete-time
// hazard product  p_s = h_s * prod_{j<s} (1 - h_j),  h_s = sigmoid(z_s), the last position taking the remaining mass
// (include/rlt_hip.h has the formulas).  The layout of heads.hip: one 256-thread workgroup per ranked list, its S token rows
// (E contiguous floats each, position-major) streamed once with 16-byte loads, the E-wide dot by wave_sum in the accumulation
// order of heads_fwd_kernel.  Everything after the dot is float64 and rounded to fp32 once: the transcendental work is spread
// over the four wavefronts, the prefix sum of the softplus terms is taken by wavefront 0 in position order (wave_scan_op over
// rounds of 64 lanes plus a carried scalar) - never as "total minus suffix", so p, stop and z at position s are functions, to
// the bit, of the rows <= s of the list (p at S-1 excepted: it is the remainder).  x is read once per pass, dx written once.
// hazard_append_kernel (rlt_hazard_head_append) is the forward on a chunk of positions, from the same device functions: the prefix
// starts from a carried sum, the last row is the remainder only when the chunk ends the list, and the stop decision is taken here.
#include "common.h"
#include "row_vec.h"

namespace {

constexpr int MAXCH = 4, MAXS = 1024;

// softplus(z) = max(z,0) + t and log sigmoid(z) = min(z,0) - t with t = log1p(exp(-|z|)): no overflow at either end
struct HzTerms { double softplus, logsig, h, omh; };
__device__ __forceinline__ HzTerms hz_terms(double z) {
    const double e = exp(-fabs(z)), t = log1p(e), r = 1.0 / (1.0 + e);
    HzTerms o;
    o.softplus = fmax(z, 0.0) + t;
    o.logsig = fmin(z, 0.0) - t;
    o.h = z >= 0.0 ? r : e * r;            // sigmoid(z)
    o.omh = z >= 0.0 ? e * r : r;          // 1 - sigmoid(z) = sigmoid(-z), without the subtraction
    return o;
}

// wavefront 0: logp[s] -= sum_{j<s} a[j] for s < S, in position order (lane s of a round adds a[s-1]; the carry is the sum of
// the rounds before).  What position s receives is computed from a[0..s-1] alone - and from `carry`, the sum the caller brings
// along (hazard_append_kernel: the softplus terms of the chunks before; 0 for a whole list).
__device__ __forceinline__ void hz_prefix(const double* a, double* logp, int S, int lane, double carry = 0.0) {
    for (int r0 = 0; r0 < S; r0 += 64) {
        const int s = r0 + lane;
        const double v = (s >= 1 && s < S) ? a[s - 1] : 0.0;
        const double incl = wave_scan_op(v, 0.0, [](double p, double q) { return p + q; });
        if (s < S) logp[s] -= carry + incl;
        carry += rlt_readlane(incl, 63);
    }
}

// zs[s] = fp32 dot(x row of position s of list b, w) + bias (+ offset[s]) for s < S: wavefront wv takes the rows wv, wv+4, ..
template <int V>
__device__ __forceinline__ void hz_logits(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                          const float* __restrict__ offset, int S, int B, int E, int b, float* zs, int lane, int wv) {
    const int nch = E / (64 * V);
    float wr[MAXCH][V];
#pragma unroll
    for (int c = 0; c < MAXCH; ++c)
        if (c < nch) ldv<V>(w + c * 64 * V + lane * V, wr[c]);
    const float b0 = bias[0];
    for (int s = wv; s < S; s += 4) {
        const float* row = x + ((size_t)s * B + b) * E;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < MAXCH; ++c)
            if (c < nch) {
                float xv[V];
                ldv<V>(row + c * 64 * V + lane * V, xv);
#pragma unroll
                for (int i = 0; i < V; ++i) acc += xv[i] * wr[c][i];
            }
        const float t = wave_sum(acc);
        if (lane == 0) zs[s] = offset ? (t + b0) + offset[s] : t + b0;
    }
}

template <int V>
__global__ __launch_bounds__(256) void hazard_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ offset,
                                                         int S, int B, int E, float* __restrict__ p_out,
                                                         float* __restrict__ stop_out, float* __restrict__ z_out) {
    __shared__ float zs[MAXS];
    __shared__ double sp[MAXS], logp[MAXS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x;
    hz_logits<V>(x, w, bias, offset, S, B, E, b, zs, lane, wv);
    __syncthreads();
    const size_t o = (size_t)b * S;
    for (int s = threadIdx.x; s < S; s += 256) {
        const float zf = zs[s];
        const HzTerms t = hz_terms((double)zf);
        const bool last = s == S - 1;
        sp[s] = t.softplus;
        logp[s] = last ? 0.0 : t.logsig;
        z_out[o + s] = zf;
        if (stop_out) stop_out[o + s] = last ? 1.f : (float)t.h;
    }
    __syncthreads();
    if (wv == 0) hz_prefix(sp, logp, S, lane);
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) p_out[o + s] = (float)exp(logp[s]);
}

template <int V>
__global__ __launch_bounds__(256) void hazard_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ z, const float* __restrict__ dp,
                                                         const float* __restrict__ dstop, int S, int B, int E,
                                                         float* __restrict__ dx, int accumulate_dx,
                                                         float* __restrict__ partial, int pw) {
    __shared__ float dz[MAXS];
    __shared__ double ga[MAXS], lt[MAXS];                       // softplus, then g = p dp | log p, then T
    extern __shared__ __attribute__((aligned(16))) float red[];   // [4][E]
    __shared__ float dbs;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int nch = E / (64 * V);
    const size_t o = (size_t)b * S;
    // ---- d(logit), float64 from z alone ------------------------------------------------------------
    for (int s = threadIdx.x; s < S; s += 256) {
        const HzTerms t = hz_terms((double)z[o + s]);
        ga[s] = t.softplus;
        lt[s] = s == S - 1 ? 0.0 : t.logsig;
    }
    __syncthreads();
    if (wv == 0) hz_prefix(ga, lt, S, lane);
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) ga[s] = exp(lt[s]) * (double)dp[o + s];
    __syncthreads();
    if (wv == 0) {
        // T_j = sum_{k>j} g_k, from the end of the list towards its head in fixed order: lane i of a round is position
        // S-1 - (r0+i) and adds g of the position after it
        double carry = 0.0;
        for (int r0 = 0; r0 < S; r0 += 64) {
            const int s = S - 1 - (r0 + lane);
            const double v = (s >= 0 && s < S - 1) ? ga[s + 1] : 0.0;
            const double incl = wave_scan_op(v, 0.0, [](double p, double q) { return p + q; });
            if (s >= 0) lt[s] = carry + incl;
            carry += rlt_readlane(incl, 63);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) {
        float d = 0.f;
        if (s < S - 1) {
            const HzTerms t = hz_terms((double)z[o + s]);
            double v = t.omh * ga[s] - t.h * lt[s];
            if (dstop) v += (double)dstop[o + s] * t.h * t.omh;
            d = (float)v;
        }
        dz[s] = d;
    }
    __syncthreads();
    if (wv == 0) {
        float bsum = 0.f;
        for (int s = lane; s < S; s += 64) bsum += dz[s];
        bsum = wave_sum(bsum);
        if (lane == 0) dbs = bsum;
    }
    // ---- dx = dz w, dw partial = sum_s dz x_s ---------------------------------------------------------
    float wr[MAXCH][V], dw[MAXCH][V];
#pragma unroll
    for (int c = 0; c < MAXCH; ++c) {
        if (c < nch) ldv<V>(w + c * 64 * V + lane * V, wr[c]);
#pragma unroll
        for (int i = 0; i < V; ++i) dw[c][i] = 0.f;
    }
    for (int s = wv; s < S; s += 4) {
        const size_t roff = ((size_t)s * B + b) * E;
        const float d = dz[s];
#pragma unroll
        for (int c = 0; c < MAXCH; ++c)
            if (c < nch) {
                const int off = c * 64 * V + lane * V;
                float xv[V], ov[V];
                ldv<V>(x + roff + off, xv);
                if (accumulate_dx) ldv<V>(dx + roff + off, ov);
                else {
#pragma unroll
                    for (int i = 0; i < V; ++i) ov[i] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    ov[i] += d * wr[c][i];
                    dw[c][i] += d * xv[i];
                }
                stv<V>(dx + roff + off, ov);
            }
    }
#pragma unroll
    for (int c = 0; c < MAXCH; ++c)
        if (c < nch) {
#pragma unroll
            for (int i = 0; i < V; ++i) red[(size_t)wv * E + c * 64 * V + lane * V + i] = dw[c][i];
        }
    __syncthreads();
    float* prow = partial + (size_t)b * pw;
    for (int col = threadIdx.x; col < E; col += 256)
        prow[col] = red[col] + red[E + col] + red[2 * E + col] + red[3 * E + col];
    if (threadIdx.x == 0) prow[E] = dbs;
}

// The forward for a CHUNK of C positions t0 .. t0+C-1 (rlt_hazard_head_append): the dot and the float64 terms of hazard_fwd_kernel,
// the prefix sum started from the list's carried L = -sum_{j<t0} softplus(z_j) and continued in position order; the last row is
// the remainder only under `final`.  logp has one slot behind the chunk: what the prefix leaves there is the carry of the next
// chunk.  With `active` the stop decision is taken here - the first row whose stop probability, widened to float64, is >= tau:
// the comparison of rlt_cut_sweep's FIRST_ABOVE rule (csrc/sweep.hip:114, `x[r] >= th` on the value widened at sweep.hip:95) - and a
// retired list leaves before it reads or writes anything.
template <int V>
__global__ __launch_bounds__(256) void hazard_append_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ offset,
                                                            int t0, int C, int B, int E, int final, double* __restrict__ carry,
                                                            double tau, int32_t* __restrict__ active, int32_t* __restrict__ k_out,
                                                            float* __restrict__ stop_out, float* __restrict__ p_out,
                                                            float* __restrict__ z_out) {
    __shared__ float zs[MAXS], st[MAXS];
    __shared__ double sp[MAXS + 1], logp[MAXS + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x;
    if (active && active[b] == 0) return;          // block-uniform
    hz_logits<V>(x, w, bias, offset, C, B, E, b, zs, lane, wv);
    __syncthreads();
    const size_t o = (size_t)b * C;
    for (int s = threadIdx.x; s < C; s += 256) {
        const float zf = zs[s];
        const HzTerms t = hz_terms((double)zf);
        const bool last = final && s == C - 1;
        sp[s] = t.softplus;
        logp[s] = last ? 0.0 : t.logsig;
        const float sf = last ? 1.f : (float)t.h;
        st[s] = sf;
        stop_out[o + s] = sf;
        if (z_out) z_out[o + s] = zf;
    }
    if (threadIdx.x == 0) { sp[C] = 0.0; logp[C] = 0.0; }
    __syncthreads();
    if (wv == 0) {
        hz_prefix(sp, logp, C + 1, lane, -carry[b]);
        if (active) {
            int first = -1;                          // 0-based inside the chunk
            for (int r0 = 0; r0 < C && first < 0; r0 += 64) {
                const int s = r0 + lane;
                const unsigned long long hit = __ballot(s < C && (double)st[s < C ? s : 0] >= tau);
                if (hit != 0ull) first = r0 + (__ffsll((long long)hit) - 1);
            }
            if (first < 0 && final) first = C - 1;   // the list ends here: rlt_cut_sweep's "S if there is none"
            if (first >= 0 && lane == 0) { k_out[b] = t0 + first + 1; active[b] = 0; }
        }
    }
    __syncthreads();
    if (p_out)
        for (int s = threadIdx.x; s < C; s += 256) p_out[o + s] = (float)exp(logp[s]);
    if (threadIdx.x == 0) carry[b] = logp[C];
}

bool hazard_dims_ok(int S, int E) { return S <= MAXS && E % 64 == 0 && E / (64 * pick_v(E)) <= MAXCH; }

}  // namespace

extern "C" {

int rlt_hazard_head_fwd(const float* x, const float* w, const float* b, const float* offset, int S, int B, int E,
                        float* p, float* stop, float* z, void* stream) {
    RLT_CHECK_ARG(x && w && b && p && z && S > 0 && B > 0 && E > 0);
    RLT_CHECK_SHAPE(hazard_dims_ok(S, E));
    if (!(rlt_aligned16(x) && rlt_aligned16(w))) return RLT_E_ALIGN;
    const int V = pick_v(E);
    hipStream_t st = rlt_stream(stream);
    dim3 grid(B), block(256);
    if (V == 4) hipLaunchKernelGGL(hazard_fwd_kernel<4>, grid, block, 0, st, x, w, b, offset, S, B, E, p, stop, z);
    else if (V == 2) hipLaunchKernelGGL(hazard_fwd_kernel<2>, grid, block, 0, st, x, w, b, offset, S, B, E, p, stop, z);
    else hipLaunchKernelGGL(hazard_fwd_kernel<1>, grid, block, 0, st, x, w, b, offset, S, B, E, p, stop, z);
    return RLT_LAUNCH_RESULT();
}

int rlt_hazard_head_append(const float* x, const float* w, const float* b, const float* offset, int t0, int C, int B, int E,
                           int final, double* carry, double tau, int32_t* active, int32_t* k, float* stop, float* p, float* z,
                           void* stream) {
    RLT_CHECK_ARG(x && w && b && carry && stop && (!active || k) && C > 0 && B > 0 && E > 0);
    RLT_CHECK_ARG(t0 >= 0 && t0 <= INT_MAX - C);
    RLT_CHECK_SHAPE(hazard_dims_ok(C, E));
    if (!(rlt_aligned16(x) && rlt_aligned16(w))) return RLT_E_ALIGN;
    const int V = pick_v(E);
    hipStream_t st = rlt_stream(stream);
    dim3 grid(B), block(256);
    if (V == 4) hipLaunchKernelGGL(hazard_append_kernel<4>, grid, block, 0, st, x, w, b, offset, t0, C, B, E, final, carry, tau, active, k, stop, p, z);
    else if (V == 2) hipLaunchKernelGGL(hazard_append_kernel<2>, grid, block, 0, st, x, w, b, offset, t0, C, B, E, final, carry, tau, active, k, stop, p, z);
    else hipLaunchKernelGGL(hazard_append_kernel<1>, grid, block, 0, st, x, w, b, offset, t0, C, B, E, final, carry, tau, active, k, stop, p, z);
    return RLT_LAUNCH_RESULT();
}

size_t rlt_hazard_head_bwd_workspace(int S, int B, int E) {
    if (S <= 0 || B <= 0 || E <= 0 || !hazard_dims_ok(S, E)) return 0;
    return (size_t)B * (E + 4) * sizeof(float);
}

int rlt_hazard_head_bwd(const float* x, const float* w, const float* z, const float* dp, const float* dstop,
                        int S, int B, int E, float* dx, int accumulate_dx, float* dw, float* db,
                        void* ws, size_t ws_bytes, void* stream) {
    RLT_CHECK_ARG(x && w && z && dp && dx && dw && db && ws && S > 0 && B > 0 && E > 0);
    RLT_CHECK_SHAPE(hazard_dims_ok(S, E));
    if (!(rlt_aligned16(x) && rlt_aligned16(w) && rlt_aligned16(dx))) return RLT_E_ALIGN;
    if (ws_bytes < rlt_hazard_head_bwd_workspace(S, B, E)) return RLT_E_WORKSPACE;
    const int V = pick_v(E);
    hipStream_t st = rlt_stream(stream);
    const int pw = E + 4;
    const size_t shm = (size_t)4 * E * sizeof(float);
    dim3 grid(B), block(256);
    float* part = (float*)ws;
    if (V == 4) hipLaunchKernelGGL(hazard_bwd_kernel<4>, grid, block, shm, st, x, w, z, dp, dstop, S, B, E, dx, accumulate_dx, part, pw);
    else if (V == 2) hipLaunchKernelGGL(hazard_bwd_kernel<2>, grid, block, shm, st, x, w, z, dp, dstop, S, B, E, dx, accumulate_dx, part, pw);
    else hipLaunchKernelGGL(hazard_bwd_kernel<1>, grid, block, shm, st, x, w, z, dp, dstop, S, B, E, dx, accumulate_dx, part, pw);
    hipLaunchKernelGGL(rlt_rows_reduce_kernel, dim3(rlt_cdiv(E + 1, 16)), dim3(256), 0, st, (const float*)part, B, pw,
                       E + 1, E, dw, db, 0);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
