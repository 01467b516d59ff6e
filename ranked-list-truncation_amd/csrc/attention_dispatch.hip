// List-axis attention: the dispatch plan and the public entry points that read it (host code only; the kernels are in the six
// family files, attention_common.h).  attn_plan() is the one place where a kernel, a prepare pass or a buffer layout is chosen.
#include "attention_plan.h"
#include "attention_common.h"
#include <stdlib.h>
#include <string.h>

namespace {

// Every environment switch of the attention family, read once per process (A/B runs: bench.py, tools/*.sh)
struct AttnEnv {
    int mode;           // RLT_ATTN_MODE=fp32|bf16x3: the family in that mode whatever the call's precision; -1 = not set
    bool attn6;         // RLT_ATTN6=0: no six-product kernels in bf16x6 mode (exact fp32 instead)
    bool attn6_img;     // RLT_ATTN6_IMG=1: attention6.hip's kernels stage pre-split tile images (a prepare pass per call, LDS-DMA in
                        // the kernels) instead of splitting their tiles themselves.  Off: it takes the 176-352 split instructions per
                        // tile out of the kernels and gives the same time back in the prepare passes (profiles/r03_notes.md)
    bool attn16;        // RLT_ATTN16=0: exact fp32 at head dim 16 on the 32x32x2 kernels (half padding) instead of attention16.hip
    bool a6n;           // RLT_A6N=0: bf16x6 at head dim 16 on attention6.hip's 32x32x16 kernels instead of attention6n.hip
    bool a6n_1;         // RLT_A6N_1=0: no pipelined head-dim-16 kernels
    bool a6n_img;       // RLT_A6N_IMG=0: the same switch under its older name
    bool a6n_f1;        // RLT_A6N_F1=0: no pipelined head-dim-16 FORWARD
    bool a6h;           // RLT_A6H=0: no pipelined head-dim-64 forward
    bool a6_pp;         // RLT_A6_PP=0: head dim 64 forward in the two-workgroup form instead of the ping-pong kernel
    bool a6_dkv1;       // RLT_A6_DKV1=0 / RLT_A6_DQ1=0: head dim 64 dK+dV / dQ on the two-wavefront kernels
    bool a6_dq1;
    bool attn_sb;       // RLT_ATTN_SB=0: exact fp32 head dim 64 forward double-buffered instead of single-buffered
    bool attn_sb_dq;    // RLT_ATTN_SB_DQ (set to anything): ... the dQ kernel single-buffered too (it spills: off)
    bool dkv_occ1;      // RLT_DKV_OCC=1: exact fp32 dK+dV in the 512-register form at every head dim
};
const AttnEnv& attn_env() {
    static const AttnEnv env = [] {
        auto on = [](const char* e, bool dflt) { return e ? atoi(e) != 0 : dflt; };
        AttnEnv v;
        const char* m = getenv("RLT_ATTN_MODE");
        v.mode = !m ? -1 : (!strcmp(m, "bf16x3") || !strcmp(m, "1")) ? 1 : 0;
        v.attn6 = on(getenv("RLT_ATTN6"), true);
        v.attn6_img = on(getenv("RLT_ATTN6_IMG"), false);
        v.attn16 = on(getenv("RLT_ATTN16"), true);
        v.a6n = on(getenv("RLT_A6N"), true);
        v.a6n_1 = on(getenv("RLT_A6N_1"), true);
        v.a6n_img = on(getenv("RLT_A6N_IMG"), true);
        v.a6n_f1 = on(getenv("RLT_A6N_F1"), true);
        v.a6h = on(getenv("RLT_A6H"), true);
        v.a6_pp = on(getenv("RLT_A6_PP"), true);
        v.a6_dkv1 = on(getenv("RLT_A6_DKV1"), true);
        v.a6_dq1 = on(getenv("RLT_A6_DQ1"), true);
        v.attn_sb = on(getenv("RLT_ATTN_SB"), true);
        v.attn_sb_dq = getenv("RLT_ATTN_SB_DQ") != nullptr;
        const char* o = getenv("RLT_DKV_OCC");
        v.dkv_occ1 = o && atoi(o) == 1;
        return v;
    }();
    return env;
}

bool hd_ok(int HD) { return HD == 16 || HD == 32 || HD == 64 || HD == 128; }
bool drop_ok(float drop_p) { return drop_p >= 0.f && drop_p < 1.f; }
// delta (S,H,B) floats, padded to 1 KiB; one flag word per 256-query workgroup, padded to 256 bytes
size_t delta_bytes(int S, int B, int H) { return ((size_t)S * H * B * sizeof(float) + 1023) / 1024 * 1024; }
size_t flags_bytes(int S, int B, int H) { return ((size_t)S * H * rlt_cdiv(B, 256) * sizeof(uint32_t) + 255) / 256 * 256; }

}  // namespace

AttnPlan attn_plan(int S, int B, int H, int HD, float drop_p, bool have_images) {
    const AttnEnv& e = attn_env();
    const int prec = rlt_precision();
    const bool drop = drop_p > 0.f;
    // ---- the arithmetic.  Head dim 128 (PLECut: d_model 256, 2 heads) has exact-fp32 kernels only, in every mode; RLT_ATTN_MODE
    // overrides the precision and keeps the six-product kernels out
    const bool x3 = HD <= 64 && (e.mode >= 0 ? e.mode == 1 : prec == RLT_PRECISION_BF16X3);
    const bool x6 = HD <= 64 && e.mode < 0 && prec == RLT_PRECISION_BF16X6 && e.attn6;
    const bool staged = x6 && e.attn6_img;
    // ---- the pipelined kernels: 512 lists and more.  Head dim 16: no dropout (train-mode calls leave them), the forward in whole
    // 128-row tiles.  Head dim 64: the forward only, in whole 64-row tiles, with or without dropout.
    const bool pipe16 = x6 && !staged && HD == 16 && B >= 512 && !drop && e.a6n && e.a6n_1 && e.a6n_img;
    const bool pipe16_fwd = pipe16 && B % 128 == 0 && e.a6n_f1;
    const bool pipe64_fwd = x6 && !staged && HD == 64 && B >= 512 && B % 64 == 0 && e.a6h;

    AttnPlan p{};
    // ---- layouts: what the workspace queries return, whatever buffers a call is given
    p.delta_bytes = delta_bytes(S, B, H);
    if (x3) {                     // Q / K / V records from the forward, dO records behind delta: the backward reads both
        p.images_kind = RLT_ATTN_IMAGES_X3_QKV; p.images_bytes = rlt_attn3_images_bytes(S, B, H, HD, 3); p.images_retained = 1;
        p.ws_kind = RLT_ATTN_WS_X3_DO; p.ws_extra_bytes = rlt_attn3_images_bytes(S, B, H, HD, 1);
    } else if (staged) {          // the same scheme with bf16x6 tile images
        p.images_kind = RLT_ATTN_IMAGES_X6_QKV; p.images_bytes = rlt_attn6_images_bytes(S, B, H, HD, 3); p.images_retained = 1;
        p.ws_kind = RLT_ATTN_WS_X6_DO; p.ws_extra_bytes = rlt_attn6_images_bytes(S, B, H, HD, 1);
    } else {
        if (pipe16_fwd || pipe64_fwd) {          // K images | V images | flag words: scratch of the forward call
            p.images_kind = pipe16_fwd ? RLT_ATTN_IMAGES_X6N_KV : RLT_ATTN_IMAGES_X6H_KV;
            p.flags_offset = pipe16_fwd ? rlt_attn6n_fwd_images_bytes(S, B, H) : rlt_attn6h_fwd_images_bytes(S, B, H);
            p.flags_bytes = flags_bytes(S, B, H);
            p.images_bytes = p.flags_offset + p.flags_bytes;
        }
        if (pipe16) { p.ws_kind = RLT_ATTN_WS_X6N_BLOCKS; p.ws_extra_bytes = rlt_attn6n_images_bytes(S, B, H); }
    }
    p.ws_bytes = p.delta_bytes + p.ws_extra_bytes;

    // ---- kernels and prepare passes, one row per case; later rows override earlier ones
    // exact fp32: fp32 mode, head dim 128, RLT_ATTN6=0, a forced mode - and bf16x3 WITHOUT `images` (rows below do not apply)
    const int f32 = HD == 16 && e.attn16 ? RLT_ATTN_F32_HD16 : RLT_ATTN_F32;
    p.fwd = HD == 64 && e.attn_sb ? RLT_ATTN_F32_SB : f32;
    p.dkv = f32 == RLT_ATTN_F32 && (HD == 128 || e.dkv_occ1) ? RLT_ATTN_F32_OCC1 : f32;
    p.dq = HD == 64 && e.attn_sb && e.attn_sb_dq ? RLT_ATTN_F32_SB : f32;
    p.bwd_prepare = RLT_ATTN_PREP_DELTA;
    p.ws_prepare_bytes = p.delta_bytes;
    // _bwd_dkv / _bwd_dq ask for the tile records behind delta unless this is a bf16x3 call without images - bf16x6 with
    // RLT_ATTN6_IMG=1 and no images included, where nothing reads them
    p.ws_part_bytes = have_images || !x3 ? p.ws_bytes : p.delta_bytes;
    if (x3 && have_images) {
        p.fwd = p.dkv = p.dq = RLT_ATTN_X3;
        p.fwd_prepare = RLT_ATTN_PREP_Q | RLT_ATTN_PREP_K | RLT_ATTN_PREP_V;
        p.bwd_prepare = RLT_ATTN_PREP_DELTA | RLT_ATTN_PREP_DO;        // (one pass: delta from the dO tiles it has in registers)
        p.ws_prepare_bytes = p.ws_bytes;
    } else if (x6) {
        // the two-wavefront kernels: attention6n.hip at head dim 16 (it has no image-staged form), else attention6.hip
        const int two_w = staged && have_images ? RLT_ATTN_X6_IMG
                        : HD == 16 && e.a6n ? (B >= 512 ? RLT_ATTN_X6N_2W_SEEDED : RLT_ATTN_X6N_2W) : RLT_ATTN_X6;
        p.fwd = p.dkv = p.dq = two_w;
        if (two_w == RLT_ATTN_X6_IMG) {
            p.fwd_prepare = RLT_ATTN_PREP_Q | RLT_ATTN_PREP_K | RLT_ATTN_PREP_V;
            p.bwd_prepare |= RLT_ATTN_PREP_DO;
            p.ws_prepare_bytes = p.ws_bytes;
        }
        if (HD == 64) {           // head dim 64 has its own kernels; a null or short `images` leaves the forward on this row
            const bool small24 = (long long)B * 3 * H * HD < (1ll << 24);      // the one-wavefront loaders' 24-bit multiplies
            if (e.a6_pp) p.fwd = two_w == RLT_ATTN_X6_IMG ? RLT_ATTN_X6_PP_IMG : RLT_ATTN_X6_PP;
            if (e.a6_dkv1 && small24) p.dkv = RLT_ATTN_X6_DKV1;
            if (e.a6_dq1 && small24) p.dq = RLT_ATTN_X6_DQ1;
        }
        if (pipe64_fwd && have_images) {         // the fix-up is the ping-pong kernel whatever RLT_A6_PP says
            p.fwd = RLT_ATTN_X6H_PIPE; p.fwd_fixup = RLT_ATTN_X6_PP; p.fwd_prepare = RLT_ATTN_PREP_K | RLT_ATTN_PREP_V;
        }
        if (pipe16_fwd && have_images) {
            p.fwd = RLT_ATTN_X6N_PIPE; p.fwd_fixup = RLT_ATTN_X6N_2W_SEEDED; p.fwd_prepare = RLT_ATTN_PREP_K | RLT_ATTN_PREP_V;
        }
        if (pipe16) {             // each backward part prepares what it reads, so the three entry points stay callable on their own
            p.dkv = p.dq = RLT_ATTN_X6N_PIPE;
            p.bwd_prepare |= RLT_ATTN_PREP_DO | RLT_ATTN_PREP_SEEDS;
            p.dkv_prepare = RLT_ATTN_PREP_Q;
            p.dq_prepare = RLT_ATTN_PREP_K | RLT_ATTN_PREP_V;
            p.ws_prepare_bytes = p.ws_bytes;
        }
    }
    return p;
}

namespace {

// one kernel of the plan, by family
int run_kernel(int kernel, int which, const AttnArgs& a, int HD, void* images, void* dimages, hipStream_t st) {
    switch (kernel) {
    case RLT_ATTN_F32: case RLT_ATTN_F32_SB: case RLT_ATTN_F32_OCC1: return rlt_attn_f32_run(kernel, which, a, HD, st);
    case RLT_ATTN_F32_HD16: return rlt_attn16_run(which, a, st);
    case RLT_ATTN_X3: return rlt_attn3_run(which, a, HD, images, dimages, st);
    case RLT_ATTN_X6: case RLT_ATTN_X6_IMG: case RLT_ATTN_X6_PP: case RLT_ATTN_X6_PP_IMG: case RLT_ATTN_X6_DKV1: case RLT_ATTN_X6_DQ1:
        return rlt_attn6_run(kernel, which, a, HD, st);
    case RLT_ATTN_X6N_2W: case RLT_ATTN_X6N_2W_SEEDED: case RLT_ATTN_X6N_PIPE: return rlt_attn6n_run(kernel, which, a, st);
    case RLT_ATTN_X6H_PIPE: return rlt_attn6h_run(which, a, st);
    }
    return RLT_E_ARG;
}

int bwd_prepare(const float* out, const float* dout, const float* lse, int S, int B, int H, int HD,
                const void* images, void* ws, size_t ws_bytes, float drop_p, void* stream) {
    RLT_CHECK_ARG(out && dout && lse && ws && S > 0 && B > 0 && H > 0 && drop_ok(drop_p));
    RLT_CHECK_SHAPE(hd_ok(HD));
    const AttnPlan p = attn_plan(S, B, H, HD, drop_p, images != nullptr);
    if (ws_bytes < p.ws_prepare_bytes) return RLT_E_WORKSPACE;
    if (!rlt_aligned16(ws)) return RLT_E_ALIGN;
    hipStream_t st = rlt_stream(stream);
    uint8_t* extra = (uint8_t*)ws + p.delta_bytes;
    AttnArgs a{};
    a.dout = dout; a.lse = lse; a.delta = (const float*)ws; a.S = S; a.B = B; a.H = H;
    if (p.dkv == RLT_ATTN_X3) {       // the pass that writes the dO records computes delta from the tiles it has in registers
        a.o = const_cast<float*>(out);
        a.drop_p = drop_p;
        return rlt_attn3_run(3, a, HD, nullptr, extra, st);
    }
    int rc = rlt_attn_delta_run(out, dout, S, B, H, HD, (float*)ws, st);
    if (!rc && (p.bwd_prepare & RLT_ATTN_PREP_DO)) {
        if (p.ws_kind == RLT_ATTN_WS_X6_DO) { a.dimg = extra; rc = rlt_attn6_prepare(true, a, HD, st); }
        else { a.img = extra; rc = rlt_attn6n_prepare(3, a, st); }
    }
    if (!rc && (p.bwd_prepare & RLT_ATTN_PREP_SEEDS)) rc = rlt_attn6n_prepare(4, a, st);        // the rows' -lse, -delta
    return rc;
}

int bwd_part(int which, const float* qkv, const float* dout, const float* lse, const void* images, void* ws, size_t ws_bytes,
             int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv, void* stream) {
    RLT_CHECK_ARG(qkv && dout && lse && ws && dqkv && S > 0 && B > 0 && H > 0 && drop_ok(drop_p));
    RLT_CHECK_SHAPE(hd_ok(HD));
    if (!(rlt_aligned16(qkv) && rlt_aligned16(dout) && rlt_aligned16(dqkv) && rlt_aligned16(ws))) return RLT_E_ALIGN;
    // the part reads delta - and, by plan, reads or WRITES tile images behind it - in THIS call's precision scope: a workspace sized
    // under another mode, or by an older delta-only rule, is refused instead of overrun
    const AttnPlan p = attn_plan(S, B, H, HD, drop_p, images != nullptr);
    if (ws_bytes < p.ws_part_bytes) return RLT_E_WORKSPACE;
    const int kernel = which == 1 ? p.dkv : p.dq, prepare = which == 1 ? p.dkv_prepare : p.dq_prepare;
    uint8_t* extra = (uint8_t*)ws + p.delta_bytes;
    AttnArgs a{};
    a.qkv = qkv; a.dout = dout; a.lse = lse; a.delta = (const float*)ws; a.dqkv = dqkv;
    a.S = S; a.B = B; a.H = H;
    a.scale = 1.0f / sqrtf((float)HD);
    a.drop_p = drop_p; a.drop_thr = rlt_drop_threshold(drop_p); a.seed = seed;
    if (kernel == RLT_ATTN_X6_IMG) { a.img = images; a.dimg = extra; }      // (the forward wrote Q / K / V, _bwd_prepare dO)
    if (kernel == RLT_ATTN_X6N_PIPE) a.img = extra;                         // (_bwd_prepare wrote dO + seeds; this part's own below)
    hipStream_t st = rlt_stream(stream);
    int rc = 0;
    for (int what = 0; what < 3 && !rc; ++what)                             // Q, K, V into blocks 0, 1, 2
        if (prepare & (1 << what)) rc = rlt_attn6n_prepare(what, a, st);
    return rc ? rc : run_kernel(kernel, which, a, HD, const_cast<void*>(images), extra, st);
}

}  // namespace

extern "C" {

int rlt_list_attention_plan(int S, int B, int H, int HD, float drop_p, int have_images, int precision, rlt_attention_plan* out) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(out && S > 0 && B > 0 && H > 0 && drop_ok(drop_p));
    RLT_CHECK_SHAPE(hd_ok(HD));
    *out = attn_plan(S, B, H, HD, drop_p, have_images != 0);
    return 0;
}

size_t rlt_list_attention_fwd_workspace(int S, int B, int H, int HD, float drop_p, int precision) {
    RLT_PREC_SCOPE_SZ(precision);
    if (S <= 0 || B <= 0 || H <= 0 || !hd_ok(HD)) return 0;
    return attn_plan(S, B, H, HD, drop_p, true).images_bytes;
}

// 1: the backward entry points read the forward's `images` - the caller keeps the buffer until the backward pass; 0: `images` is
// scratch of the forward call (the pipelined bf16x6 forward kernels) or empty
int rlt_list_attention_images_retained(int S, int B, int H, int HD, int precision) {
    RLT_PREC_SCOPE_SZ(precision);
    if (S <= 0 || B <= 0 || H <= 0 || !hd_ok(HD)) return 0;
    return attn_plan(S, B, H, HD, 0.f, true).images_retained;
}

int rlt_list_attention_fwd(const float* qkv, int S, int B, int H, int HD, float drop_p, uint32_t seed,
                           float* out, float* lse, void* images, size_t images_bytes, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(qkv && out && lse && S > 0 && B > 0 && H > 0 && drop_ok(drop_p));
    RLT_CHECK_SHAPE(hd_ok(HD));
    if (!(rlt_aligned16(qkv) && rlt_aligned16(out))) return RLT_E_ALIGN;
    AttnPlan p = attn_plan(S, B, H, HD, drop_p, images != nullptr);
    if (p.fwd_prepare && p.images_retained) {        // the backward kernels will read these images: they must all be written
        if (images_bytes < p.images_bytes) return RLT_E_WORKSPACE;
        if (!rlt_aligned16(images)) return RLT_E_ALIGN;
    } else if (p.fwd_prepare && !(rlt_aligned16(images) && images_bytes >= p.images_bytes)) {
        p = attn_plan(S, B, H, HD, drop_p, false);   // scratch of a pipelined forward: short or misaligned counts as not given
    }
    AttnArgs a{};
    a.qkv = qkv; a.o = out; a.lse_o = lse; a.S = S; a.B = B; a.H = H;
    a.scale = 1.0f / sqrtf((float)HD);
    a.drop_p = drop_p; a.drop_thr = rlt_drop_threshold(drop_p); a.seed = seed;
    if (p.fwd_prepare) a.img = images;
    if (p.fwd_fixup) a.redo = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(images) + p.flags_offset);
    hipStream_t st = rlt_stream(stream);
    int rc = 0;
    switch (p.fwd) {                                 // the prepare passes of the plan (bf16x3: inside its forward launcher)
    case RLT_ATTN_X6_IMG: case RLT_ATTN_X6_PP_IMG: rc = rlt_attn6_prepare(false, a, HD, st); break;
    case RLT_ATTN_X6N_PIPE: rc = rlt_attn6n_prepare_at(1, 0, a, st); if (!rc) rc = rlt_attn6n_prepare_at(2, 1, a, st); break;
    case RLT_ATTN_X6H_PIPE: rc = rlt_attn6h_prepare2(1, 0, 2, 1, a, st); break;
    }
    if (!rc) rc = run_kernel(p.fwd, 0, a, HD, images, nullptr, st);
    if (!rc && p.fwd_fixup) rc = run_kernel(p.fwd_fixup, 0, a, HD, nullptr, nullptr, st);
    return rc;
}

size_t rlt_list_attention_bwd_workspace(int S, int B, int H, int HD, float drop_p, int precision) {
    RLT_PREC_SCOPE_SZ(precision);
    if (S <= 0 || B <= 0 || H <= 0 || !hd_ok(HD)) return 0;
    return attn_plan(S, B, H, HD, drop_p, true).ws_bytes;
}

int rlt_list_attention_bwd_prepare(const float* out, const float* dout, const float* lse, int S, int B, int H, int HD, float drop_p,
                                   const void* images, void* ws, size_t ws_bytes, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    return bwd_prepare(out, dout, lse, S, B, H, HD, images, ws, ws_bytes, drop_p, stream);
}

int rlt_list_attention_bwd_dkv(const float* qkv, const float* dout, const float* lse, const void* images, void* ws, size_t ws_bytes,
                               int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    return bwd_part(1, qkv, dout, lse, images, ws, ws_bytes, S, B, H, HD, drop_p, seed, dqkv, stream);
}

int rlt_list_attention_bwd_dq(const float* qkv, const float* dout, const float* lse, const void* images, void* ws, size_t ws_bytes,
                              int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    return bwd_part(2, qkv, dout, lse, images, ws, ws_bytes, S, B, H, HD, drop_p, seed, dqkv, stream);
}

int rlt_list_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                           int S, int B, int H, int HD, float drop_p, uint32_t seed, const void* images, float* dqkv,
                           void* ws, size_t ws_bytes, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(drop_ok(drop_p));
    int rc = bwd_prepare(out, dout, lse, S, B, H, HD, images, ws, ws_bytes, drop_p, stream);
    if (!rc) rc = bwd_part(1, qkv, dout, lse, images, ws, ws_bytes, S, B, H, HD, drop_p, seed, dqkv, stream);
    if (!rc) rc = bwd_part(2, qkv, dout, lse, images, ws, ws_bytes, S, B, H, HD, drop_p, seed, dqkv, stream);
    return rc;
}

}  // extern "C"
