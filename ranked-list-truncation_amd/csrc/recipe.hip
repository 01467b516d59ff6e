// The training recipe in one Adam pass: learning-rate schedule, per-tensor parameter groups, coupled or decoupled weight decay and
// an exponential moving average of the parameters (include/rlt_hip.h states the arithmetic and its order).
//
//   rlt_adam_step_recipe   the decision (one lane: skip or apply, the step count, the bias corrections, lr of the applied-step
//                          count in float64, the EMA decay) and the update, adam_guarded_kernel's arithmetic (csrc/optim.hip) with
//                          the segment's learning rate and weight decay;
//   rlt_lr_at              the decision's schedule expression on the host;
//   rlt_swap_f32           two fp32 buffers exchanged in place (evaluation with the averaged weights).
//
// The update is an HBM-bound streaming pass: 16-byte accesses, a grid capped at GRID_CAP workgroups.  What a group of four
// elements needs beside them - lr_scale and weight_decay of its segment - comes from the n_seg-entry table, not from a side array
// as long as the bucket: the bucket is cut into CHUNKS at absolute positions c * CHUNK as in the norm pass, the segment of a
// chunk's first element is found once per trip (kept from the trip before when it still holds it, else the seg_of search), and
// where boundaries fall inside the chunk every lane walks forward from there over its own four groups, whose positions ascend.
// Offsets are multiples of 4, so a 16-byte group never straddles a boundary.  A chunk with no boundary inside - all but n_seg of
// them - takes the wavefront-uniform path: two table reads per trip, a frozen chunk skipped whole.
#include "common.h"
#include "seg_table.h"

namespace {

constexpr int CHUNK = RLT_RECIPE_CHUNK;          // elements one workgroup takes per trip: 256 lanes x 4 groups x 4 floats
constexpr int GRID_CAP = RLT_RECIPE_GRID;        // 256 CUs x 8 workgroups
constexpr int GROUPS = CHUNK / 1024;             // 16-byte groups per lane and trip
static_assert(CHUNK % 1024 == 0 && GROUPS == 4, "a chunk is four 16-byte groups per lane of a 256-lane workgroup");
static_assert(sizeof(rlt_recipe) == 64 && sizeof(rlt_recipe_group) == 8 && sizeof(rlt_recipe_state) == 32 &&
              sizeof(rlt_opt_state) == 104, "ABI layouts");

// lr(t) as include/rlt_hip.h writes it: float64, left to right, no contraction (the library is built with -ffp-contract=off), so
// that host and device agree bit for bit up to their cos
__host__ __device__ inline double lr_value(double B, double ratio, int kind, long long W, long long T, long long t) {
    const double F = B * ratio;
    if (t <= W) return B * (double)t / (double)W;
    if (kind == RLT_SCHED_CONSTANT) return B;
    if (t > T) return F;
    if (kind == RLT_SCHED_LINEAR) return F + (B - F) * (double)(T - t) / (double)(T - W);
    return F + (B - F) * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)(t - W) / (double)(T - W)));
}

struct Sched { double base, ratio; long long warmup, total; int kind; };
struct Hyper { float b1, b2, eps, wd; };

// ---------------------------------------------------------------- the decision: one lane
__global__ void recipe_decide_kernel(rlt_opt_state* __restrict__ st, rlt_recipe_state* __restrict__ rs, Sched sc, float b1, float b2,
                                     int use_norm, int skip_nonfinite, float ema_decay, int ema_warmup) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float coef = 1.0f;
    if (use_norm) {
        if (skip_nonfinite && st->nonfinite != 0) {          // nothing of the recipe state is written
            st->apply = 0;
            st->skipped += 1;
            return;
        }
        coef = st->coef;
    }
    const long long t = st->step + 1;
    st->step = t;
    if (coef < 1.0f) st->clipped += 1;
    st->apply = 1;
    st->bc1 = (float)(1.0 - pow((double)b1, (double)t));
    st->bc2_sqrt = sqrtf((float)(1.0 - pow((double)b2, (double)t)));
    const double lr = lr_value(sc.base, sc.ratio, sc.kind, sc.warmup, sc.total, t);
    rs->lr64 = lr;
    rs->lr = (float)lr;
    rs->coef = coef;
    if (ema_decay != 0.f) {
        const long long k = rs->ema_updates;
        double d = (double)ema_decay;
        if (ema_warmup) d = fmin(d, (1.0 + (double)k) / (10.0 + (double)k));
        rs->ema_decay = (float)d;
        rs->ema_updates = k + 1;
    }
}

// ---------------------------------------------------------------- the update
struct Step { float coef, lr, bc1, bc2_sqrt, d; };

// one 16-byte group at element i of a segment with learning rate lr_s and weight decay wd
template <bool EMA, bool DECOUPLED>
__device__ __forceinline__ void update_group(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, float* __restrict__ ema, long long i, const Step& s,
                                             const Hyper& h, float lr_s, float wd) {
    const float4 g4 = *reinterpret_cast<const float4*>(g + i);
    const float4 p4 = *reinterpret_cast<const float4*>(p + i), m4 = *reinterpret_cast<const float4*>(m + i);
    const float4 v4 = *reinterpret_cast<const float4*>(v + i);
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EMA) e4 = *reinterpret_cast<const float4*>(ema + i);
    const float ge[4] = {g4.x, g4.y, g4.z, g4.w};
    float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w}, ve[4] = {v4.x, v4.y, v4.z, v4.w};
    float ee[4] = {e4.x, e4.y, e4.z, e4.w};
    const float step = lr_s / s.bc1, decay = lr_s * wd;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                 // adam_guarded_kernel (csrc/optim.hip), element for element
        float gr = ge[k] * s.coef;
        const float pv = pe[k];
        if (!DECOUPLED && wd != 0.f) gr += wd * pv;
        const float mi = h.b1 * me[k] + (1.f - h.b1) * gr;
        const float vi = h.b2 * ve[k] + (1.f - h.b2) * gr * gr;
        me[k] = mi;
        ve[k] = vi;
        const float denom = sqrtf(vi) / s.bc2_sqrt + h.eps;
        const float u = step * (mi / denom);
        const float pn = DECOUPLED ? pv - (decay * pv + u) : pv - u;
        pe[k] = pn;
        if (EMA) ee[k] = s.d * ee[k] + (1.f - s.d) * pn;
    }
    *reinterpret_cast<float4*>(m + i) = make_float4(me[0], me[1], me[2], me[3]);
    *reinterpret_cast<float4*>(v + i) = make_float4(ve[0], ve[1], ve[2], ve[3]);
    *reinterpret_cast<float4*>(p + i) = make_float4(pe[0], pe[1], pe[2], pe[3]);
    if (EMA) *reinterpret_cast<float4*>(ema + i) = make_float4(ee[0], ee[1], ee[2], ee[3]);
}

// Every element that is touched lies below n (i % 4 == 0 and n % 4 == 0), every table index is at most n_seg (offsets) or below
// n_seg (groups): a table that is not ascending gives a meaningless assignment of groups and nothing else.
template <bool EMA, bool DECOUPLED>
__global__ __launch_bounds__(256) void recipe_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, long long n,
                                                            long long n_chunks, const long long* __restrict__ off,
                                                            const rlt_recipe_group* __restrict__ grp, int n_seg,
                                                            const rlt_opt_state* __restrict__ st,
                                                            const rlt_recipe_state* __restrict__ rs, Hyper h) {
    if (!st->apply) return;                       // skipped step: nothing is read and nothing is written
    const Step s{rs->coef, rs->lr, st->bc1, st->bc2_sqrt, rs->ema_decay};
    int s0 = 0;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long long cs = c * CHUNK;
        const long long ce = cs + CHUNK < n ? cs + CHUNK : n;
        long long seg_end = n;                    // end of the segment that holds the chunk's first element
        float scale = 1.f, wd = h.wd;
        if (off) {
            if (!(off[s0] <= cs && cs < off[s0 + 1])) s0 = seg_of(off, n_seg, cs);
            seg_end = off[s0 + 1];
            scale = grp[s0].lr_scale;
            wd = grp[s0].weight_decay;
        }
        if (seg_end >= ce) {                      // no boundary inside the chunk: one group for all of it
            if (scale == 0.f) continue;           // frozen
            const float lr_s = s.lr * scale;
#pragma unroll
            for (int j = 0; j < GROUPS; ++j) {
                const long long i = cs + (long long)(j * 256 + threadIdx.x) * 4;
                if (i < ce) update_group<EMA, DECOUPLED>(p, g, m, v, ema, i, s, h, lr_s, wd);
            }
        } else {
            int sg = s0;
            long long hi = seg_end;
#pragma unroll
            for (int j = 0; j < GROUPS; ++j) {
                const long long i = cs + (long long)(j * 256 + threadIdx.x) * 4;
                if (i >= ce) break;
                while (i >= hi && sg + 1 < n_seg) hi = off[++sg + 1];
                const rlt_recipe_group gr = grp[sg];
                if (gr.lr_scale != 0.f) update_group<EMA, DECOUPLED>(p, g, m, v, ema, i, s, h, s.lr * gr.lr_scale, gr.weight_decay);
            }
        }
    }
}

__global__ __launch_bounds__(256) void swap_kernel(float4* __restrict__ a, float4* __restrict__ b, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

inline bool is_nan(double x) { return x != x; }

// what both rlt_lr_at and the step refuse in the schedule's fields
bool sched_ok(const rlt_recipe* r) {
    if (is_nan(r->base_lr) || is_nan(r->min_lr_ratio)) return false;
    if (r->sched_kind < RLT_SCHED_CONSTANT || r->sched_kind > RLT_SCHED_COSINE || r->warmup_steps < 0) return false;
    if (r->sched_kind != RLT_SCHED_CONSTANT && r->total_steps <= r->warmup_steps) return false;
    return r->min_lr_ratio >= 0.f && r->min_lr_ratio <= 1.f;
}

template <bool EMA, bool DECOUPLED>
void launch_update(hipStream_t st, unsigned grid, float* p, const float* g, float* m, float* v, float* ema, long long n, long long nc,
                   const long long* off, const rlt_recipe_group* grp, int n_seg, const rlt_opt_state* state,
                   const rlt_recipe_state* rstate, Hyper h) {
    hipLaunchKernelGGL((recipe_update_kernel<EMA, DECOUPLED>), dim3(grid), dim3(256), 0, st, p, g, m, v, ema, n, nc, off, grp, n_seg, state,
                       rstate, h);
}

}  // namespace

extern "C" {

size_t rlt_recipe_chunk(void) { return CHUNK; }
int rlt_recipe_grid(void) { return GRID_CAP; }

double rlt_lr_at(const rlt_recipe* r, int64_t t) {
    if (!r || t < 1 || !sched_ok(r)) return (double)NAN;
    return lr_value((double)r->base_lr, (double)r->min_lr_ratio, r->sched_kind, r->warmup_steps, r->total_steps, t);
}

int rlt_adam_step_recipe(float* p, const float* g, float* m, float* v, float* ema, size_t n, const int64_t* seg_offsets,
                         const rlt_recipe_group* groups, int n_seg, rlt_opt_state* state, rlt_recipe_state* rstate,
                         const rlt_recipe* r, void* stream) {
    RLT_CHECK_ARG(p && g && m && v && state && rstate && r && n > 0 && n_seg >= 0);
    RLT_CHECK_ARG(n_seg > 0 ? (seg_offsets && groups) : (!seg_offsets && !groups));
    RLT_CHECK_ARG(!(is_nan(r->beta1) || is_nan(r->beta2) || is_nan(r->eps) || is_nan(r->weight_decay) || is_nan(r->ema_decay)));
    RLT_CHECK_ARG(sched_ok(r));
    RLT_CHECK_ARG(r->ema_decay >= 0.f && r->ema_decay < 1.f && (ema != nullptr) == (r->ema_decay != 0.f));
    RLT_CHECK_SHAPE(n % 4 == 0 && n <= ((size_t)1 << 46));
    if (!(rlt_aligned16(p) && rlt_aligned16(g) && rlt_aligned16(m) && rlt_aligned16(v) && rlt_aligned16(ema))) return RLT_E_ALIGN;
    if (((uintptr_t)state & 7u) || ((uintptr_t)rstate & 7u) || ((uintptr_t)seg_offsets & 7u) || ((uintptr_t)groups & 7u)) return RLT_E_ALIGN;
    if (n_seg > 0 && host_readable(seg_offsets) && !seg_table_ok(seg_offsets, n_seg, n)) return RLT_E_ARG;
    hipStream_t st = rlt_stream(stream);
    const Sched sc{(double)r->base_lr, (double)r->min_lr_ratio, r->warmup_steps, r->total_steps, r->sched_kind};
    hipLaunchKernelGGL(recipe_decide_kernel, dim3(1), dim3(64), 0, st, state, rstate, sc, r->beta1, r->beta2, r->use_norm,
                       r->skip_nonfinite, r->ema_decay, r->ema_warmup);
    const long long nc = (long long)((n + CHUNK - 1) / CHUNK);
    const unsigned grid = (unsigned)(nc < GRID_CAP ? nc : GRID_CAP);
    const Hyper h{r->beta1, r->beta2, r->eps, r->weight_decay};
    const long long* off = (const long long*)seg_offsets;
    auto launch = ema ? (r->decoupled ? launch_update<true, true> : launch_update<true, false>)
                      : (r->decoupled ? launch_update<false, true> : launch_update<false, false>);
    launch(st, grid, p, g, m, v, ema, (long long)n, nc, off, groups, n_seg, state, rstate, h);
    return RLT_LAUNCH_RESULT();
}

int rlt_swap_f32(float* a, float* b, size_t n, void* stream) {
    RLT_CHECK_ARG(a && b && n > 0);
    RLT_CHECK_SHAPE(n % 4 == 0);
    if (!(rlt_aligned16(a) && rlt_aligned16(b))) return RLT_E_ALIGN;
    RLT_CHECK_ARG(a + n <= b || b + n <= a);      // overlapping buffers have no exchange
    const size_t n4 = n / 4, grid = (n4 + 255) / 256;
    hipLaunchKernelGGL(swap_kernel, dim3((unsigned)(grid < (size_t)GRID_CAP ? grid : (size_t)GRID_CAP)), dim3(256), 0, rlt_stream(stream),
                       reinterpret_cast<float4*>(a), reinterpret_cast<float4*>(b), n4);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
