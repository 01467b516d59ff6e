// Guarded optimizer step: gradient norm (global and per parameter tensor), norm clipping and the non-finite skip, all on the
// device (torch.nn.utils.clip_grad_norm_ + torch.optim.Adam of run.py:104,129 with no host read in between).
//
//   rlt_grad_norm          one read of the flat fp32 gradient bucket -> float64 sum of squares over the finite elements, the
//                          non-finite count and max |g| per segment (one FlatModel slot) and for the bucket, the clip
//                          coefficient min(1, max_norm / (norm + 1e-6)) and the running epoch figures, into rlt_opt_state;
//   rlt_adam_step_guarded  adam_kernel's arithmetic (csrc/mmoe.hip) on gr = g * coef + wd * p, with the step count and the
//                          bias corrections read from rlt_opt_state; nothing is touched when the step is skipped.
//
// Both are HBM-bound streaming passes: 16-byte loads, a grid capped at GRID_CAP workgroups striding over the bucket, no LDS
// beyond the four-wavefront reduction of the norm pass.
//
// Order of the sums (what makes the norm bitwise reproducible and independent of the grid): the bucket is cut into CHUNKS of
// RLT_GRAD_NORM_CHUNK elements at absolute positions c * CHUNK.  A chunk is summed by ONE workgroup in one fixed order (per
// lane its four 16-byte groups in order, the 64 lanes by the DPP scan of common.h, the four wavefronts in order) whichever
// workgroup of whichever grid takes it.  Where no segment boundary falls inside chunk c its figures are the record head[c];
// where boundaries do, head[c] covers the elements up to the first boundary and every segment s that STARTS inside the chunk
// gets first[s] = its elements inside this chunk (exactly one chunk writes it).  A segment's figures are then first[s] (when
// the segment starts off a chunk edge) and the head records of the chunks that start inside it, in ascending order, summed lane
// by lane (item i in lane i % 64) and by the DPP scan; the bucket's figures are the segment figures summed the same way.
#include "common.h"
#include "seg_table.h"

namespace {

constexpr int CHUNK = RLT_GRAD_NORM_CHUNK;       // elements one workgroup takes per trip: 256 lanes x 4 groups x 4 floats
constexpr int GRID_CAP = RLT_GRAD_NORM_GRID;     // 256 CUs x 8 workgroups
constexpr int GROUPS = CHUNK / 1024;             // 16-byte groups per lane and trip
static_assert(CHUNK % 1024 == 0 && GROUPS == 4, "a chunk is four 16-byte groups per lane of a 256-lane workgroup");

struct Fig {                  // figures of a set of elements: a chunk record, a segment's first piece, a segment, the bucket
    double sumsq;             // over the finite elements
    long long nonfinite;      // NaN and +-Inf
    long long nan;            // of those, NaN (decides whether the norm is NaN or Inf when the gradient is not finite)
    double max_abs;           // over the finite elements (a float value)
};
static_assert(sizeof(Fig) == 32 && sizeof(rlt_grad_seg) == 24 && sizeof(rlt_opt_state) == 104, "ABI layouts");

__device__ __forceinline__ Fig fig_zero() { return Fig{0.0, 0, 0, 0.0}; }
__device__ __forceinline__ void fig_add(Fig& a, const Fig& b) {
    a.sumsq += b.sumsq;
    a.nonfinite += b.nonfinite;
    a.nan += b.nan;
    a.max_abs = fmax(a.max_abs, b.max_abs);
}
__device__ __forceinline__ void fig_take(Fig& a, float x) {
    if (x != x) { a.nonfinite += 1; a.nan += 1; }
    else if (fabsf(x) == INFINITY) a.nonfinite += 1;
    else {
        const double d = (double)x;
        a.sumsq += d * d;
        a.max_abs = fmax(a.max_abs, fabs(d));
    }
}
__device__ __forceinline__ Fig fig_of(const float4& v) {
    Fig f = fig_zero();
    fig_take(f, v.x); fig_take(f, v.y); fig_take(f, v.z); fig_take(f, v.w);
    return f;
}
// the 64 lanes in the fixed order of the DPP scan; the same value in every lane
__device__ __forceinline__ Fig fig_wave(const Fig& f) {
    Fig r;
    r.sumsq = wave_sum(f.sumsq);
    r.nonfinite = wave_sum(f.nonfinite);
    r.nan = wave_sum(f.nan);
    r.max_abs = rlt_readlane(wave_scan_op(f.max_abs, 0.0, [](double a, double b) { return fmax(a, b); }), 63);
    return r;
}

// ---------------------------------------------------------------- the pass: one record per chunk (+ one per segment start)
// Every index that is written is bounded by construction (c < n_chunks, s < n_seg), every element that is read lies below n:
// a table that is not ascending gives meaningless figures and nothing else.
__global__ __launch_bounds__(256) void grad_norm_pass_kernel(const float* __restrict__ g, long long n, long long n_chunks,
                                                             const long long* __restrict__ off, int n_seg,
                                                             Fig* __restrict__ head, Fig* __restrict__ first) {
    __shared__ Fig red[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int s0 = 0, buf = 0;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long long cs = c * CHUNK;
        const long long ce = cs + CHUNK < n ? cs + CHUNK : n;
        float4 x[GROUPS];
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) {
            const long long i = cs + (long long)(j * 256 + threadIdx.x) * 4;
            x[j] = i < n ? *reinterpret_cast<const float4*>(g + i) : make_float4(0.f, 0.f, 0.f, 0.f);     // n % 4 == 0
        }
        long long seg_end = n;                    // end of the segment that holds the chunk's first element
        if (off) {
            if (!(off[s0] <= cs && cs < off[s0 + 1])) s0 = seg_of(off, n_seg, cs);
            seg_end = off[s0 + 1];
        }
        Fig f[GROUPS];
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) f[j] = fig_of(x[j]);
        if (seg_end >= ce) {                      // no boundary inside the chunk: the whole chunk is the head record
            Fig t = f[0];
#pragma unroll
            for (int j = 1; j < GROUPS; ++j) fig_add(t, f[j]);
            t = fig_wave(t);
            if (lane == 0) red[buf][wv] = t;
            __syncthreads();
            if (threadIdx.x == 0) {
                Fig r = red[buf][0];
                fig_add(r, red[buf][1]); fig_add(r, red[buf][2]); fig_add(r, red[buf][3]);
                head[c] = r;
            }
            buf ^= 1;                             // the next trip writes the other half: one barrier per reduction
        } else {
            // piece -1: [cs, seg_end) -> head[c]; then every segment s > s0 that starts below ce: [off[s], min(off[s+1], ce)) -> first[s]
            long long lo = cs, hi = seg_end;
            for (int s = s0;;) {
                Fig t = fig_zero();
#pragma unroll
                for (int j = 0; j < GROUPS; ++j) {
                    const long long i = cs + (long long)(j * 256 + threadIdx.x) * 4;
                    if (i >= lo && i < hi) fig_add(t, f[j]);       // offsets are multiples of 4: a group never straddles
                }
                t = fig_wave(t);
                if (lane == 0) red[buf][wv] = t;
                __syncthreads();
                if (threadIdx.x == 0) {
                    Fig r = red[buf][0];
                    fig_add(r, red[buf][1]); fig_add(r, red[buf][2]); fig_add(r, red[buf][3]);
                    if (s == s0) head[c] = r; else first[s] = r;
                }
                buf ^= 1;
                ++s;
                if (s >= n_seg) break;
                lo = off[s];
                if (lo >= ce || lo < cs) break;   // (lo < cs: only a table that is not ascending)
                hi = off[s + 1] < ce ? off[s + 1] : ce;
            }
        }
    }
}

// ---------------------------------------------------------------- per segment: one wavefront sums its records in order
__global__ __launch_bounds__(256) void grad_norm_seg_kernel(const Fig* __restrict__ head, const Fig* __restrict__ first,
                                                            long long n, long long n_chunks, const long long* __restrict__ off,
                                                            int n_seg, Fig* __restrict__ seg, rlt_grad_seg* __restrict__ seg_out) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_seg) return;                       // wave-uniform
    long long lo = off ? off[s] : 0, hi = off ? off[s + 1] : n;
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < 0 ? 0 : (hi > n ? n : hi);
    Fig t = fig_zero();
    if (hi > lo) {
        const bool has_first = lo % CHUNK != 0;
        long long c0 = (lo + CHUNK - 1) / CHUNK, c1 = (hi + CHUNK - 1) / CHUNK;       // chunks that start inside [lo, hi)
        if (c1 > n_chunks) c1 = n_chunks;
        const long long items = (has_first ? 1 : 0) + (c1 > c0 ? c1 - c0 : 0);
        for (long long i = lane; i < items; i += 64) {
            if (has_first && i == 0) fig_add(t, first[s]);
            else fig_add(t, head[c0 + i - (has_first ? 1 : 0)]);
        }
    }
    t = fig_wave(t);
    if (lane == 0) {
        seg[s] = t;
        if (seg_out) {
            rlt_grad_seg o;
            o.sumsq = t.sumsq; o.nonfinite = t.nonfinite; o.max_abs = t.max_abs;
            seg_out[s] = o;
        }
    }
}

// ---------------------------------------------------------------- the bucket: the segments in order, then norm and coefficient
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const Fig* __restrict__ seg, int n_seg, float max_norm,
                                                               rlt_opt_state* __restrict__ st) {
    __shared__ Fig red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Fig t = fig_zero();
    for (int s = threadIdx.x; s < n_seg; s += 256) fig_add(t, seg[s]);
    t = fig_wave(t);
    if (lane == 0) red[wv] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    Fig r = red[0];
    fig_add(r, red[1]); fig_add(r, red[2]); fig_add(r, red[3]);
    // torch.linalg.vector_norm of a gradient that is not finite: NaN when a NaN is among them, else Inf
    const double norm = r.nan > 0 ? (double)NAN : (r.nonfinite > 0 ? (double)INFINITY : sqrt(r.sumsq));
    float coef = 1.0f;
    if (max_norm > 0.f && max_norm != INFINITY) {          // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1), NaN kept
        const double q = (double)max_norm / (norm + 1e-6);
        coef = (float)(q != q ? q : (q < 1.0 ? q : 1.0));
    }
    st->nonfinite = r.nonfinite;
    st->nan_count = r.nan;
    st->sumsq = r.sumsq;
    st->norm = norm;
    st->max_abs = r.max_abs;
    st->coef = coef;
    if (r.nonfinite == 0) {
        st->norm_sum += norm;
        st->norm_max = fmax(st->norm_max, norm);
        st->norm_steps += 1;
    }
}

// ---------------------------------------------------------------- guarded Adam: decide once, then the update
// One lane: skip or apply, the counters, and the bias corrections of the step about to be applied (a float64 pow per element
// would turn the streaming update into a compute-bound one).
__global__ void adam_decide_kernel(rlt_opt_state* __restrict__ st, float b1, float b2, int skip_nonfinite) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (skip_nonfinite && st->nonfinite != 0) {
        st->apply = 0;
        st->skipped += 1;
        return;
    }
    const long long t = st->step + 1;
    st->step = t;
    if (st->coef < 1.0f) st->clipped += 1;
    st->apply = 1;
    st->bc1 = (float)(1.0 - pow((double)b1, (double)t));
    st->bc2_sqrt = sqrtf((float)(1.0 - pow((double)b2, (double)t)));
}

__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, size_t n4, const rlt_opt_state* __restrict__ st,
                                                           float lr, float b1, float b2, float eps, float wd) {
    if (!st->apply) return;                       // skipped step: p, m, v are not read and not written
    const float coef = st->coef, bc1 = st->bc1, bc2_sqrt = st->bc2_sqrt;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 g4 = reinterpret_cast<const float4*>(g)[i];
        float4 p4 = reinterpret_cast<float4*>(p)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
        const float ge[4] = {g4.x, g4.y, g4.z, g4.w};
        float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w}, ve[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {             // adam_kernel (csrc/mmoe.hip), element for element, on the clipped gradient
            float gr = ge[k] * coef;
            const float pv = pe[k];
            if (wd != 0.f) gr += wd * pv;
            const float mi = b1 * me[k] + (1.f - b1) * gr;
            const float vi = b2 * ve[k] + (1.f - b2) * gr * gr;
            me[k] = mi;
            ve[k] = vi;
            const float denom = sqrtf(vi) / bc2_sqrt + eps;
            pe[k] = pv - (lr / bc1) * (mi / denom);
        }
        reinterpret_cast<float4*>(m)[i] = make_float4(me[0], me[1], me[2], me[3]);
        reinterpret_cast<float4*>(v)[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
        reinterpret_cast<float4*>(p)[i] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    }
}

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline long long chunks_of(size_t n) { return (long long)((n + CHUNK - 1) / CHUNK); }

}  // namespace

extern "C" {

size_t rlt_grad_norm_chunk(void) { return CHUNK; }
int rlt_grad_norm_grid(void) { return GRID_CAP; }

size_t rlt_grad_norm_workspace(size_t n, int n_seg) {
    if (n == 0 || n % 4 != 0 || n_seg < 0) return 0;
    const size_t ns = n_seg > 0 ? (size_t)n_seg : 1;
    return up16((size_t)chunks_of(n) * sizeof(Fig)) + 2 * up16(ns * sizeof(Fig));          // head | first | seg
}

int rlt_grad_norm(const float* g, size_t n, const int64_t* seg_offsets, int n_seg, float max_norm,
                  void* ws, size_t ws_bytes, rlt_grad_seg* seg_out, rlt_opt_state* state, void* stream) {
    RLT_CHECK_ARG(g && ws && state && n > 0 && n_seg >= 0 && max_norm == max_norm);
    RLT_CHECK_ARG(n_seg > 0 ? (seg_offsets && seg_out) : !seg_offsets);
    RLT_CHECK_SHAPE(n % 4 == 0 && n <= ((size_t)1 << 46));
    if (!rlt_aligned16(g) || ((uintptr_t)seg_offsets & 7u) || ((uintptr_t)seg_out & 7u) || ((uintptr_t)state & 7u)) return RLT_E_ALIGN;
    if (!rlt_aligned16(ws) || ws_bytes < rlt_grad_norm_workspace(n, n_seg)) return RLT_E_WORKSPACE;
    if (n_seg > 0 && host_readable(seg_offsets) && !seg_table_ok(seg_offsets, n_seg, n)) return RLT_E_ARG;
    const long long nc = chunks_of(n);
    const int ns = n_seg > 0 ? n_seg : 1;
    Fig* head = (Fig*)ws;
    Fig* first = (Fig*)((char*)ws + up16((size_t)nc * sizeof(Fig)));
    Fig* seg = (Fig*)((char*)first + up16((size_t)ns * sizeof(Fig)));
    hipStream_t st = rlt_stream(stream);
    const long long* off = (const long long*)seg_offsets;
    hipLaunchKernelGGL(grad_norm_pass_kernel, dim3((unsigned)(nc < GRID_CAP ? nc : GRID_CAP)), dim3(256), 0, st, g, (long long)n, nc,
                       off, n_seg, head, first);
    hipLaunchKernelGGL(grad_norm_seg_kernel, dim3(rlt_cdiv(ns, 4)), dim3(256), 0, st, (const Fig*)head, (const Fig*)first, (long long)n,
                       nc, off, ns, seg, seg_out);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, (const Fig*)seg, ns, max_norm, state);
    return RLT_LAUNCH_RESULT();
}

int rlt_adam_step_guarded(float* p, const float* g, float* m, float* v, size_t n, rlt_opt_state* state,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int skip_nonfinite, void* stream) {
    RLT_CHECK_ARG(p && g && m && v && state && n > 0);
    RLT_CHECK_SHAPE(n % 4 == 0);
    if (!(rlt_aligned16(p) && rlt_aligned16(g) && rlt_aligned16(m) && rlt_aligned16(v)) || ((uintptr_t)state & 7u)) return RLT_E_ALIGN;
    hipStream_t st = rlt_stream(stream);
    hipLaunchKernelGGL(adam_decide_kernel, dim3(1), dim3(64), 0, st, state, beta1, beta2, skip_nonfinite);
    const size_t n4 = n / 4;
    const size_t grid = (n4 + 255) / 256;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)(grid < (size_t)GRID_CAP ? grid : (size_t)GRID_CAP)), dim3(256), 0, st, p, g, m, v, n4,
                       (const rlt_opt_state*)state, lr, beta1, beta2, eps, weight_decay);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
