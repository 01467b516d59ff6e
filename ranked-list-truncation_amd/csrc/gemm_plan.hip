// The GEMM family's dispatch plan (host code only; the kernels are in gemm_f32.hip, gemm3.hip and the gemm6*.hip files).  gemm_plan() is the one place where a
// kernel family, loader form, persistent form, split, slab length, XCD pinning, gemm6s epilogue or panel form is chosen.
//
// The family's environment switches (A/B runs: bench.py, tools/*.sh), read once per process:
//   switch                   default  governs
//   RLT_GEMM_MODE            unset    fp32|0, bf16x3|1, bf16x6|2: the family in that mode whatever the call's precision
//   RLT_GEMM_NOFAST          0        gemm / gemm3: 1 = the guarded loaders on every shape
//   RLT_GEMM_NO_BIG          0        bf16x3: 1 = no 256 x 256 tiles (gemm3b -> gemm3)
//   RLT_GEMM_PERSIST         256      gemm3b: workgroups of the persistent form; 0 (or no multiple of 8) = off
//   RLT_GEMM_PERSIST_NN      0        gemm3b: 1 = the persistent form for B stored [K][N] too (not with bits_in)
//   RLT_GEMM6_PERSIST        256      gemm6c / gemm6e: workgroups of the persistent form; 0 (or no multiple of 8) = off
//   RLT_GEMM6_SMALL          unset    bf16x6: set = 256 x 128 tiles everywhere (gemm6c / gemm6e / gemm6b -> gemm6)
//   RLT_GEMM6C               1        bf16x6: 0 = gemm6b in place of gemm6c and gemm6e
//   RLT_GEMM6E               1        bf16x6: 0 = gemm6c in place of gemm6e
//   RLT_GEMM6E_ALL           0        bf16x6: 1 = gemm6e for A stored [M][K] at every K below 1024 (not only 768)
//   RLT_GEMM6S               1        bf16x6: 0 = the tiled kernels in place of the weights-stationary one
//   RLT_GEMM_SPLIT_KMIN      1024     split-K from this K
//   RLT_GEMM_SPLIT_TARGET    1024     split-K: workgroups to fill (wanted slabs = target / output tiles of 128 x 128)
//   RLT_GEMM_NO_SLAB_XCD     unset    split-K: set = K slabs in gridDim.z even where their count is a multiple of 8
#define RLT_HOST_ONLY
#include "gemm_plan.h"
#include "common.h"
#include <stdlib.h>
#include <string.h>

namespace {

struct GemmEnv {
    int mode;             // RLT_GEMM_MODE: 0 exact fp32, 1 bf16x3, 2 bf16x6; -1 = not set (the call's precision)
    bool nofast;          // RLT_GEMM_NOFAST=1: guarded loaders everywhere
    bool no_big;          // RLT_GEMM_NO_BIG=1: no gemm3b
    int persist;          // RLT_GEMM_PERSIST: workgroups of persistent gemm3b
    bool persist_nn;      // RLT_GEMM_PERSIST_NN=1: persistent gemm3b with B stored [K][N]
    int persist6;         // RLT_GEMM6_PERSIST: workgroups of persistent gemm6c / gemm6e
    bool small6;          // RLT_GEMM6_SMALL (set to anything): gemm6 on every bf16x6 shape
    bool gemm6c;          // RLT_GEMM6C=0: gemm6b instead of the k-step pipelines
    bool gemm6e;          // RLT_GEMM6E=0: gemm6c instead of gemm6e
    bool gemm6e_all;      // RLT_GEMM6E_ALL=1: gemm6e whatever K and the layout of A
    bool gemm6s;          // RLT_GEMM6S=0: no weights-stationary kernel
    int split_kmin;       // RLT_GEMM_SPLIT_KMIN
    int split_target;     // RLT_GEMM_SPLIT_TARGET
    bool no_slab_xcd;     // RLT_GEMM_NO_SLAB_XCD (set to anything): no XCD-pinned slabs
};
const GemmEnv& gemm_env() {
    static const GemmEnv env = [] {
        auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        GemmEnv v;
        const char* m = getenv("RLT_GEMM_MODE");
        v.mode = !m ? -1 : (!strcmp(m, "bf16x6") || !strcmp(m, "2")) ? 2 : (!strcmp(m, "bf16x3") || !strcmp(m, "1")) ? 1 : 0;
        v.nofast = num("RLT_GEMM_NOFAST", 0) != 0;
        v.no_big = num("RLT_GEMM_NO_BIG", 0) != 0;
        v.persist = num("RLT_GEMM_PERSIST", 256);
        v.persist_nn = num("RLT_GEMM_PERSIST_NN", 0) != 0;
        v.persist6 = num("RLT_GEMM6_PERSIST", 256);
        v.small6 = getenv("RLT_GEMM6_SMALL") != nullptr;
        v.gemm6c = num("RLT_GEMM6C", 1) != 0;
        v.gemm6e = num("RLT_GEMM6E", 1) != 0;
        v.gemm6e_all = num("RLT_GEMM6E_ALL", 0) != 0;
        v.gemm6s = num("RLT_GEMM6S", 1) != 0;
        v.split_kmin = num("RLT_GEMM_SPLIT_KMIN", 1024);
        v.split_target = num("RLT_GEMM_SPLIT_TARGET", 1024);
        v.no_slab_xcd = getenv("RLT_GEMM_NO_SLAB_XCD") != nullptr;
        return v;
    }();
    return env;
}

// split-K fills the chip where the 128 x 128 output tiles alone do not
// (K from 1024: the reference's own batch sizes - 32 / 63 lists x 300 positions = 9,600 / 18,900 rows - leave the K = 2048 products
//  of the encoder with 75-150 output tiles: unsplit, a third of the chip ran 2048-long loops, 160-200 us per product at batch 32)
int wanted_slabs(int M, int N, int K) {
    const GemmEnv& e = gemm_env();
    const long long tiles = (long long)rlt_cdiv(M, 128) * rlt_cdiv(N, 128);
    if (tiles >= 256 || K < e.split_kmin) return 1;
    long long want = e.split_target / tiles > 0 ? e.split_target / tiles : 1;     // workgroups in flight: a whole number of waves of the grid
    const long long per = K >= 4096 ? 512 : 256;              // keep >= 512 of K per slice (>= 256 below K = 4096)
    const long long maxs = K / per > 0 ? K / per : 1;
    if (want > maxs) want = maxs;
    if (want > 256) want = 256;
    if (want >= 8) want = want / 8 * 8;       // whole groups of 8 slabs: one slab per XCD and round (decode_block)
    return (int)want;
}
// the partial products and the partial column sums of `slabs` K slabs
size_t slab_bytes(int slabs, int M, int N) { return slabs > 1 ? ((size_t)slabs * M * N + (size_t)slabs * M) * sizeof(float) : 0; }

}  // namespace

GemmPlan gemm_plan(const GemmCall& c) {
    const GemmEnv& e = gemm_env();
    // 0 = exact fp32 MFMA (parity mode), 1 = split-bf16 (bf16x3), 2 = fp32-faithful six-product split (bf16x6)
    const int mode = e.mode >= 0 ? e.mode : rlt_precision();
    const int M = c.M, N = c.N, K = c.K;
    const bool ta = c.ta != 0, tb = c.tb != 0;
    auto has = [&](int bit) { return (c.present & bit) != 0; };
    auto al = [&](int bit) { return (c.aligned16 & bit) != 0; };
    const bool bias = has(RLT_GEMM_PTR_BIAS), bias2 = has(RLT_GEMM_PTR_BIAS2), mask = has(RLT_GEMM_PTR_RELU_MASK),
               colsum = has(RLT_GEMM_PTR_COLSUM), bits_out = has(RLT_GEMM_PTR_BITS_OUT), bits_in = has(RLT_GEMM_PTR_BITS_IN);
    const bool relu = (c.flags & RLT_GEMM_RELU) != 0, accumulate = (c.flags & RLT_GEMM_ACCUMULATE) != 0, drop = c.drop != 0;
    // 16-byte vector loads of an operand: what every branch-free loader and every tile beyond 128 x 128 needs
    const bool vec = c.lda % 4 == 0 && al(RLT_GEMM_PTR_A) && c.ldb % 4 == 0 && al(RLT_GEMM_PTR_B);

    GemmPlan p{};
    // ---- split-K: the slabs the shape wants (the bit epilogues live in the GEMM kernel proper: no split with them) ...
    const int want = bits_out || bits_in ? 1 : wanted_slabs(M, N, K);
    p.ws_bytes = slab_bytes(want, M, N);
    // ---- ... and the slabs the call gets: none without a workspace; a short one is refused
    int ns = want;
    if (ns > 1 && (c.ws_null || c.ws_bytes < p.ws_bytes)) {
        if (c.ws_null && c.ws_bytes == 0) ns = 1;
        else { p.rc = RLT_E_WORKSPACE; return p; }
    }
    const int kchunk = rlt_cdiv(rlt_cdiv(K, ns), 32) * 32;            // whole 32-wide K tiles per slab, which may take slabs away
    ns = rlt_cdiv(K, kchunk);
    const int slab_xcd = ns > 1 && ns % 8 == 0 && !e.no_slab_xcd;

    // ---- the kernel family, first row that holds
    // gemm6s: K = 256 / 128 with the long dimension in M (the Linear layers of the encoder, the LSTM input projection): the
    // weights-stationary streaming kernel - no K loop, nothing re-split per tile.  Epilogues: bias, ReLU, the mask pair (bits_in
    // with nothing else); 256-column panels, 128-column ones at K = 128 without the masks; 32-bit buffer offsets of a 32-row block
    const bool wide = N % 256 == 0;
    const bool gemm6s = mode == 2 && e.gemm6s && !ta && ns == 1 && !mask && !colsum && !drop && !accumulate &&
        (!bits_in || (!bias && !bias2 && !relu)) && !(bits_out && bits_in) &&
        (K == 256 || K == 128) && (wide || (K == 128 && N % 128 == 0 && !bits_out && !bits_in)) && N <= 256 * 256 && M >= 32 * 256 &&
        vec && c.ldc % 4 == 0 && al(RLT_GEMM_PTR_C) && (!bias || al(RLT_GEMM_PTR_BIAS)) && (!bias2 || al(RLT_GEMM_PTR_BIAS2)) &&
        (!bits_out || al(RLT_GEMM_PTR_BITS_OUT)) && (!bits_in || al(RLT_GEMM_PTR_BITS_IN)) &&
        (size_t)c.lda * 4 * 32 < (1u << 31) && (size_t)c.ldc * 4 * 32 < (1u << 31);
    // the bf16x6 tiles: M % 256 == 0, N % 128 == 0, whole 32-wide K tiles and the branch-free loader preconditions; other shapes of
    // that mode run on the exact f32 MFMA kernel (more exact still).  256 x 256 with N % 256 == 0
    const bool tile6 = mode == 2 && vec && M % 256 == 0 && N % 128 == 0 && K % 32 == 0;
    const bool big6 = tile6 && wide && !e.small6;
    // gemm6c / gemm6e: every K slab, the last one included, holds at least two K tiles of 32 (the k-step pipeline stages one register
    // tile ahead); gemm6b takes the others.  (K % 32 == 0 here, so kchunk <= K and a short last slab is whole tiles too)
    const bool pipe6 = big6 && e.gemm6c && kchunk >= 64 && (K % kchunk == 0 || K % kchunk >= 64);
    // gemm6e (one wavefront per SIMD) where the K loop decides - the weight-gradient products (A stored [K][M], K = the 1.2 M
    // rows: 5.66 against 6.38 ms for 2048 x 256 x 1,228,800) and K >= 1024 (ffn1 dX 5.92 against 6.34 ms, ffn2 forward 5.90 against
    // 6.04) - and the epilogue is one of its plain forms; the K = 256 products (prologue / epilogue bound: 7.02 against 6.70 ms
    // for 1,228,800 x 2048 x 256) and the mask / dropout epilogues stay on gemm6c
    // K = 768 (the attention in-projection's dX, 1,228,800 x 256 x 768, accumulated in place) runs on gemm6e as well since its
    // accumulate epilogue reads C in batches: 2.45 against 3.21 ms accumulating, 2.29 against 2.69-2.99 plain, both layouts of B
    // (before: 3.92 against 3.20).  K = 512 and 992 measured faster there too at that M and N (profiles/accum_epilogue_notes.md);
    // no product of the models has those lengths, and they stay where they were
    const bool plain_epilogue = !mask && !bits_in && !bits_out && !drop;
    // the 256-wide bf16x3 tile: M % 256 == 0, N % 256 == 0, whole 32-wide K tiles, the branch-free loader preconditions
    const bool big3 = mode == 1 && !e.no_big && vec && M % 256 == 0 && N % 256 == 0 && K % 32 == 0;
    const int family = gemm6s ? RLT_GEMM_6S
                     : pipe6 ? (e.gemm6e && plain_epilogue && (ta || K >= 1024 || K == 768 || e.gemm6e_all) ? RLT_GEMM_6E : RLT_GEMM_6C)
                     : big6 ? RLT_GEMM_6B
                     : tile6 ? RLT_GEMM_6
                     : big3 ? RLT_GEMM_3B
                     : mode == 1 ? RLT_GEMM_3 : RLT_GEMM_F32;
    const GemmFamily& f = GEMM_FAMILY[family];
    p.wg = f.wg;
    p.lds_bytes = f.lds;
    p.reduce = ns > 1;

    if (family == RLT_GEMM_6S) {
        if (bits_out && !relu) { p.rc = -1; return p; }
        const int narrow = !wide;                                     // 128-column panels (K = 128)
        const int npanel = N / (narrow ? 128 : 256), nblk = (M + 31) / 32;
        int nstream = 256 / npanel;                                   // one workgroup per CU: the panels x as many row streams as fill the chip
        if (nstream < 1) nstream = 1;
        if (nstream > nblk) nstream = nblk;
        p.tiles_m = nstream; p.tiles_n = npanel;
        p.grid_x = npanel * nstream; p.grid_z = 1;
        p.lds_bytes = K == 256 ? GEMM6S_LDS_K256 : GEMM6S_LDS_K128;
        p.d = rlt_gemm_dispatch{family, 0, tb, 1, 0, 1, K, 0, bits_in ? 3 : bits_out ? 2 : relu ? 1 : 0, narrow};
        return p;
    }
    p.tiles_m = rlt_cdiv(M, f.bm); p.tiles_n = rlt_cdiv(N, f.bn);
    const long long tiles = (long long)p.tiles_m * p.tiles_n;
    // the branch-free loaders of gemm / gemm3 need: aligned operands, K % 4 == 0, K >= 4, MN % 4 == 0 for MN-contiguous operands
    // (A stored [K][M], B stored [K][N]); the other families have no other loader
    const bool small = family == RLT_GEMM_F32 || family == RLT_GEMM_3;
    const bool fast = !small || (!e.nofast && vec && K % 4 == 0 && K >= 4 && (!ta || (M % 4 == 0 && M >= 4)) && (tb || (N % 4 == 0 && N >= 4)));
    // persistent (no split-K, A stored [M][K], more output tiles than workgroups, whole groups of 8 workgroups): the workgroups
    // walk the tiles.  gemm3b, measured: NT -6 % at K = 256, -2 % at K = 2048.  NN (RLT_GEMM_PERSIST_NN=1): -7 % / -2 % alone with a
    // bias epilogue, but the training step, whose dX products accumulate in place, is 0.4 ms slower with it
    const int wgs = family == RLT_GEMM_3B ? e.persist : e.persist6;
    const bool persistent = !ta && ns == 1 && wgs > 0 && wgs % 8 == 0 && tiles > wgs &&
        (family == RLT_GEMM_3B ? (tb || (e.persist_nn && !bits_in)) && K / 32 >= 2 : family == RLT_GEMM_6C || family == RLT_GEMM_6E);
    p.grid_x = persistent ? wgs : (unsigned)(tiles * (slab_xcd ? ns : 1));
    p.grid_z = slab_xcd ? 1 : ns;
    p.d = rlt_gemm_dispatch{family, ta, tb, fast, persistent, ns, kchunk, slab_xcd, 0, 0};
    return p;
}

extern "C" {

size_t rlt_gemm_workspace(int ta, int tb, int M, int N, int K) {
    (void)ta; (void)tb;
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return slab_bytes(wanted_slabs(M, N, K), M, N);
}

int rlt_gemm_plan(const rlt_gemm_call* c, int precision, rlt_gemm_dispatch* out) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(c && out && c->M > 0 && c->N > 0 && c->K > 0);
    RLT_CHECK_ARG(c->lda >= (c->ta ? c->M : c->K) && c->ldb >= (c->tb ? c->K : c->N) && c->ldc >= c->N);
    RLT_CHECK_ARG(!(c->present & RLT_GEMM_PTR_COLSUM) || c->ta);
    const GemmPlan p = gemm_plan(*c);
    *out = p.d;
    return p.rc;
}

}  // extern "C"
