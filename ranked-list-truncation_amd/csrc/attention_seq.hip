// Within-list ("position-axis") attention: every list of the mini-batch attends over its own S positions
// (nn.MultiheadAttention with batch_first=True on a (B, S, E) input).  rlt_seq_attention_fwd / _bwd of include/rlt_hip.h.
//
// Activations stay position-major: qkv is (S*B, 3E) with row s*B + b, so the rows of list b are B*3E floats apart and the
// contiguous run per (row, head) is HD floats.  A workgroup (4 wavefronts) owns 64 COLUMNS of one list: one head at head dim
// 64, four neighbouring heads at head dim 16 (the last group of a head count off 4 is narrower) - every global read of a
// tile row then covers whole 128-byte lines at both head dims.  It streams 64-row tiles of those columns through LDS
// (two tiles of 64 x 68 floats: K and V in the forward and in the dQ phase, Q and dO in the dK+dV phase), flash-style.
//   head dim 64: the four wavefronts each own 32 of 128 rows of the head; head dim 16: wavefront w owns head w, 32 rows.
// Products run on the exact-fp32 32x32x2 MFMA with the OWNED row on the lane (D[i][j], j = lane & 31): the score tile is
// computed transposed, so a lane holds 16 scores of ONE owned row, the row maximum / sum is in-lane plus one exchange with
// lane ^ 32, and the accumulator registers are the B operand of the next product as they stand (the contraction over the
// 32 tile rows runs in the accumulator's row order acc_row(t, half)).  At head dim 16 the transposed outputs (O^T, dQ^T,
// dK^T, dV^T: head dim x 32 rows) fill half of a 32 x 32 tile; the other half is computed and dropped.
// Forward: running maximum m and normaliser l per query, O^T rescaled per tile; lse = m + log l of the UNdropped scores.
// Backward, ONE launch, no sum crosses a workgroup (no atomics, no workspace; two calls give the same bits):
//   phase 1  a wavefront owns 32 queries: delta = rowsum(dout * out) in registers, dQ^T in registers across the key tiles;
//            it leaves the rows' lse * log2(e) and delta in LDS
//   phase 2  a wavefront owns 32 keys: dK^T and dV^T in registers across the query tiles, finished per key block
// (scores and dP are recomputed in both phases: 7 products of 4*S*S*HD/2 flops per (list, head) instead of 5).
// The three precision codes run these same kernels (exact fp32 is at least what bf16x6 / bf16x3 promise).
// Dropout: stream pair_seed(seed, b*H + h), keep = rlt_keep(stream, query, key, thr), kept weights * 1/(1-p).
// CAUSAL (rlt_seq_attention_fwd_ex / _bwd_ex, RLT_SEQ_MASK_CAUSAL): key j is admitted for query i iff j <= i.  A compare per score in
// the diagonal sub-tile, and the tiles above the diagonal are skipped: the forward and phase 1 end the key-tile loop at the pass's
// last query (block-uniform) and a wavefront leaves the sub-tile loop behind its own last query; phase 2 starts the query-tile
// loop at the pass's first key and a wavefront skips the sub-tiles in front of its own.  lse is over the admitted keys; the keep
// stream is unchanged (a masked draw is never used).  A masked weight is an exact 0 times a row of the same sub-tile: finite rows
// below a position never reach it, a NaN or inf there can.  The CAUSAL = false instantiations are the kernels as they were.
// (the per-tile device functions, the geometry and the limits: attention_seq_tile.h, shared with attention_seq_append.hip)
#include "attention_seq_tile.h"

namespace {

struct SeqArgs {
    const float* qkv; const float* out; const float* dout; const float* lse;
    float* o; float* lse_o; float* dqkv;
    int S, B, H;
    float scale, inv_keep;
    uint32_t thr, seed;
};

template <int HD, bool DROP, bool CAUSAL>
__global__ __launch_bounds__(256) void seq_attn_fwd_kernel(SeqArgs a) {
    using G = SeqGeom<HD>;
    constexpr int HPG = G::HPG, OWN = G::OWN, DT = G::DT, KH = G::KH;
    __shared__ __attribute__((aligned(16))) float Ks[SQ_TR * SQ_LD];
    __shared__ __attribute__((aligned(16))) float Vs[SQ_TR * SQ_LD];
    __shared__ uint32_t chash[HPG][SQ_TR];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int S = a.S, B = a.B, H = a.H;
    const int ngrp = (H + HPG - 1) / HPG;
    const int b = blockIdx.x / ngrp, h0 = (blockIdx.x % ngrp) * HPG;
    const int nh = H - h0 < HPG ? H - h0 : HPG;
    const int E = H * HD;
    const size_t ld = 3 * (size_t)E;
    const int c0 = h0 * HD, cw = nh * HD;
    const int hw = HPG == 1 ? 0 : w;              // this wavefront's head inside the group
    const int h = h0 + hw, hc = hw * HD;
    const int woff = HPG == 1 ? 32 * w : 0;       // its rows inside the pass
    const int dcol = hc + (HD == 16 ? (l31 & 15) : l31);
    const float c = a.scale * LOG2E;
    const uint32_t stream = DROP ? pair_seed(a.seed, b * H + h) : 0u;

    for (int q0 = 0; q0 < S; q0 += OWN) {
        const int q = q0 + woff + l31;
        const bool wave_on = hw < nh && q0 + woff < S;
        float qr[KH];
#pragma unroll
        for (int i = 0; i < KH; ++i) qr[i] = 0.f;
        if (wave_on && q < S) sq_load_row<KH>(qr, a.qkv + ((size_t)q * B + b) * ld + c0 + hc + hh * KH);
        f32x16 acc[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
        float m = -INFINITY, lsum = 0.f;
        const uint32_t rh = DROP ? rlt_row_hash(stream, (uint32_t)q) : 0u;

        const int kend = CAUSAL ? sq_key_end(S, q0 + OWN) : S;      // block-uniform: staging is collective
        for (int k0 = 0; k0 < kend; k0 += SQ_TR) {
            __syncthreads();
            sq_stage(Ks, a.qkv + E, ld, B, b, k0, S, c0, cw, tid);
            sq_stage(Vs, a.qkv + 2 * (size_t)E, ld, B, b, k0, S, c0, cw, tid);
            if (DROP && (HPG > 1 || w == 0)) chash[hw][lane] = rlt_col_hash(stream, (uint32_t)(k0 + lane));
            __syncthreads();
            if (!wave_on) continue;
#pragma unroll 1
            for (int sub = 0; sub < SQ_TR / 32; ++sub) {
                const int kb = k0 + 32 * sub;
                if (kb >= S) break;
                if (CAUSAL && kb > q0 + woff + 31) break;   // every key of the sub-tile lies behind the wavefront's last query
                // S^T[key][query]: register r of this lane = key kb + acc_row(r, hh), query q
                f32x16 s = sq_rows_dot<KH>(Ks + (32 * sub + l31) * SQ_LD + hc + hh * KH, qr);
                float mx = m;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = (CAUSAL ? sq_admit(kb + acc_row(r, hh), q, S) : kb + acc_row(r, hh) < S) ? s[r] * c : -INFINITY;
                    s[r] = sv;
                    mx = fmaxf(mx, sv);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 32));          // key kb itself is < S: finite from the first tile on (causal: key 0)
                const float alpha = rlt_exp2(m - mx);
                m = mx;
                lsum *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[dt][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float p = rlt_exp2(s[r] - mx);
                    lsum += p;
                    if (DROP) p = rlt_keep_rc(rh, chash[hw][32 * sub + acc_row(r, hh)], a.thr) ? p * a.inv_keep : 0.f;
                    s[r] = p;
                }
                // O^T[d][query] += V^T[d][key] P^T[key][query]
                sq_cols_acc<DT>(acc, Vs + 32 * sub * SQ_LD + dcol, hh, s);
            }
        }
        if (wave_on) {
            lsum += __shfl_xor(lsum, 32);
            if (q < S) {
                sq_store_T<HD>(a.o + ((size_t)q * B + b) * E + c0 + hc, hh, acc, 1.f / lsum);
                if (hh == 0) a.lse_o[((size_t)b * H + h) * S + q] = (m + log2f(lsum)) * LN2;
            }
        }
    }
}

// dynamic LDS: Xs | Ys (two tiles) | lse2[HPG][Sr] | delta[HPG][Sr] | hashes[HPG][64], Sr = S rounded up to the pass
template <int HD>
size_t seq_bwd_lds_bytes(int S) {
    using G = SeqGeom<HD>;
    const size_t Sr = (size_t)(S + G::OWN - 1) / G::OWN * G::OWN;
    return sizeof(float) * (2 * (size_t)SQ_TR * SQ_LD + 2 * G::HPG * Sr + (size_t)G::HPG * SQ_TR);
}

template <int HD, bool DROP, bool CAUSAL>
__global__ __launch_bounds__(256) void seq_attn_bwd_kernel(SeqArgs a) {
    using G = SeqGeom<HD>;
    constexpr int HPG = G::HPG, OWN = G::OWN, DT = G::DT, KH = G::KH;
    extern __shared__ __attribute__((aligned(16))) float sq_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int S = a.S, B = a.B, H = a.H;
    const int Sr = (S + OWN - 1) / OWN * OWN;
    float* Xs = sq_lds;
    float* Ys = Xs + SQ_TR * SQ_LD;
    float* lse2_s = Ys + SQ_TR * SQ_LD;
    float* delta_s = lse2_s + HPG * Sr;
    uint32_t* hash_s = reinterpret_cast<uint32_t*>(delta_s + HPG * Sr);
    const int ngrp = (H + HPG - 1) / HPG;
    const int b = blockIdx.x / ngrp, h0 = (blockIdx.x % ngrp) * HPG;
    const int nh = H - h0 < HPG ? H - h0 : HPG;
    const int E = H * HD;
    const size_t ld = 3 * (size_t)E;
    const int c0 = h0 * HD, cw = nh * HD;
    const int hw = HPG == 1 ? 0 : w;
    const int h = h0 + hw, hc = hw * HD;
    const int woff = HPG == 1 ? 32 * w : 0;
    const int dcol = hc + (HD == 16 ? (l31 & 15) : l31);
    const float c = a.scale * LOG2E;
    const uint32_t stream = DROP ? pair_seed(a.seed, b * H + h) : 0u;
    float* lse2_w = lse2_s + hw * Sr;
    float* delta_w = delta_s + hw * Sr;
    uint32_t* hash_w = hash_s + hw * SQ_TR;

    // ---- phase 1: dQ (a wavefront owns 32 queries), and the rows' lse * log2(e) and delta into LDS
    for (int q0 = 0; q0 < S; q0 += OWN) {
        const int q = q0 + woff + l31;
        const bool wave_on = hw < nh && q0 + woff < S;
        float qr[KH], dor[KH];
#pragma unroll
        for (int i = 0; i < KH; ++i) { qr[i] = 0.f; dor[i] = 0.f; }
        float lse2 = INFINITY, delta = 0.f;
        if (wave_on && q < S) {
            const size_t row = (size_t)q * B + b;
            sq_load_row<KH>(qr, a.qkv + row * ld + c0 + hc + hh * KH);
            sq_load_row<KH>(dor, a.dout + row * E + c0 + hc + hh * KH);
            float orow[KH];
            sq_load_row<KH>(orow, a.out + row * E + c0 + hc + hh * KH);
#pragma unroll
            for (int i = 0; i < KH; ++i) delta += dor[i] * orow[i];
            lse2 = a.lse[((size_t)b * H + h) * S + q] * LOG2E;
        }
        if (wave_on) {
            delta += __shfl_xor(delta, 32);
            if (hh == 0) { lse2_w[q] = lse2; delta_w[q] = delta; }      // q < Sr; rows >= S: +inf (weight 0), 0
        }
        f32x16 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
        const uint32_t rh = DROP ? rlt_row_hash(stream, (uint32_t)q) : 0u;

        const int kend = CAUSAL ? sq_key_end(S, q0 + OWN) : S;
        for (int k0 = 0; k0 < kend; k0 += SQ_TR) {
            __syncthreads();
            sq_stage(Xs, a.qkv + E, ld, B, b, k0, S, c0, cw, tid);                    // K
            sq_stage(Ys, a.qkv + 2 * (size_t)E, ld, B, b, k0, S, c0, cw, tid);        // V
            if (DROP && (HPG > 1 || w == 0)) hash_w[lane] = rlt_col_hash(stream, (uint32_t)(k0 + lane));
            __syncthreads();
            if (!wave_on) continue;
#pragma unroll 1
            for (int sub = 0; sub < SQ_TR / 32; ++sub) {
                const int kb = k0 + 32 * sub;
                if (kb >= S) break;
                if (CAUSAL && kb > q0 + woff + 31) break;
                const int trow = (32 * sub + l31) * SQ_LD + hc + hh * KH;
                f32x16 s = sq_rows_dot<KH>(Xs + trow, qr);            // S^T[key][query]
                f32x16 dp = sq_rows_dot<KH>(Ys + trow, dor);          // dP^T[key][query]
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = (CAUSAL ? sq_admit(kb + acc_row(r, hh), q, S) : kb + acc_row(r, hh) < S) ? rlt_exp2(s[r] * c - lse2) : 0.f;
                    float g = dp[r];
                    if (DROP) g = rlt_keep_rc(rh, hash_w[32 * sub + acc_row(r, hh)], a.thr) ? g * a.inv_keep : 0.f;
                    s[r] = p * (g - delta) * a.scale;                 // dS^T, with the score scale
                }
                sq_cols_acc<DT>(dq, Xs + 32 * sub * SQ_LD + dcol, hh, s);     // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
            }
        }
        if (wave_on && q < S) sq_store_T<HD>(a.dqkv + ((size_t)q * B + b) * ld + c0 + hc, hh, dq, 1.f);
    }

    // ---- phase 2: dK, dV (a wavefront owns 32 keys); Xs = Q tile, Ys = dO tile
    for (int k0 = 0; k0 < S; k0 += OWN) {
        const int key = k0 + woff + l31;
        const bool wave_on = hw < nh && k0 + woff < S;
        float kr[KH], vr[KH];
#pragma unroll
        for (int i = 0; i < KH; ++i) { kr[i] = 0.f; vr[i] = 0.f; }
        if (wave_on && key < S) {
            const float* row = a.qkv + ((size_t)key * B + b) * ld + c0 + hc + hh * KH;
            sq_load_row<KH>(kr, row + E);
            sq_load_row<KH>(vr, row + 2 * (size_t)E);
        }
        f32x16 dk[DT], dv[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }
        const uint32_t ch = DROP ? rlt_col_hash(stream, (uint32_t)key) : 0u;

        // causal: the queries in front of the pass's first key weigh it 0 - start at the 64-row tile that holds that key
        for (int q0 = CAUSAL ? k0 / SQ_TR * SQ_TR : 0; q0 < S; q0 += SQ_TR) {
            __syncthreads();                                                           // also: phase 1's lse2 / delta are complete
            sq_stage(Xs, a.qkv, ld, B, b, q0, S, c0, cw, tid);                         // Q
            sq_stage(Ys, a.dout, (size_t)E, B, b, q0, S, c0, cw, tid);                 // dO
            if (DROP && (HPG > 1 || w == 0)) hash_w[lane] = rlt_row_hash(stream, (uint32_t)(q0 + lane));
            __syncthreads();
            if (!wave_on) continue;
#pragma unroll 1
            for (int sub = 0; sub < SQ_TR / 32; ++sub) {
                const int qb = q0 + 32 * sub;
                if (qb >= S) break;
                if (CAUSAL && qb + 31 < k0 + woff) continue;          // every query of the sub-tile lies in front of the wavefront's first key
                const int trow = (32 * sub + l31) * SQ_LD + hc + hh * KH;
                f32x16 s = sq_rows_dot<KH>(Xs + trow, kr);            // S[query][key]: register r = query qb + acc_row(r, hh)
                f32x16 dp = sq_rows_dot<KH>(Ys + trow, vr);           // dP[query][key]
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qq = qb + acc_row(r, hh);               // < Sr; rows >= S have lse2 = +inf: weight 0
                    float p = rlt_exp2(s[r] * c - lse2_w[qq]);
                    if (CAUSAL) p = qq >= key ? p : 0.f;              // selected, not left to lse
                    float g = dp[r];
                    if (DROP) {
                        const bool keep = rlt_keep_rc(hash_w[32 * sub + acc_row(r, hh)], ch, a.thr);
                        g = keep ? g * a.inv_keep : 0.f;
                        dp[r] = keep ? p * a.inv_keep : 0.f;          // the dropped weights, for dV
                    } else {
                        dp[r] = p;
                    }
                    s[r] = p * (g - delta_w[qq]) * a.scale;           // dS
                }
                sq_cols_acc<DT>(dv, Ys + 32 * sub * SQ_LD + dcol, hh, dp);    // dV^T[d][key] += dO^T[d][query] P[query][key]
                sq_cols_acc<DT>(dk, Xs + 32 * sub * SQ_LD + dcol, hh, s);     // dK^T[d][key] += Q^T[d][query] dS[query][key]
            }
        }
        if (wave_on && key < S) {
            float* row = a.dqkv + ((size_t)key * B + b) * ld + c0 + hc;
            sq_store_T<HD>(row + E, hh, dk, 1.f);
            sq_store_T<HD>(row + 2 * (size_t)E, hh, dv, 1.f);
        }
    }
}

SeqArgs seq_args(int S, int B, int H, int HD, float drop_p, uint32_t seed) {
    SeqArgs a{};
    a.S = S; a.B = B; a.H = H;
    a.scale = 1.0f / sqrtf((float)HD);
    a.inv_keep = 1.f / (1.f - drop_p);
    a.thr = rlt_drop_threshold(drop_p);
    a.seed = seed;
    return a;
}

template <int HD, bool DROP, bool CAUSAL>
int seq_launch_fwd_as(const SeqArgs& a, hipStream_t st) {
    const int ngrp = (a.H + SeqGeom<HD>::HPG - 1) / SeqGeom<HD>::HPG;
    const dim3 grid((unsigned)((long long)a.B * ngrp)), block(256);
    hipLaunchKernelGGL((seq_attn_fwd_kernel<HD, DROP, CAUSAL>), grid, block, 0, st, a);
    return RLT_LAUNCH_RESULT();
}

template <int HD, bool DROP, bool CAUSAL>
int seq_launch_bwd_as(const SeqArgs& a, hipStream_t st) {
    const int ngrp = (a.H + SeqGeom<HD>::HPG - 1) / SeqGeom<HD>::HPG;
    const dim3 grid((unsigned)((long long)a.B * ngrp)), block(256);
    const size_t lds = seq_bwd_lds_bytes<HD>(a.S);
    if (int rc = rlt_allow_lds(seq_attn_bwd_kernel<HD, DROP, CAUSAL>, lds)) return rc;
    hipLaunchKernelGGL((seq_attn_bwd_kernel<HD, DROP, CAUSAL>), grid, block, lds, st, a);
    return RLT_LAUNCH_RESULT();
}

template <int HD>
int seq_launch_fwd(const SeqArgs& a, bool drop, bool causal, hipStream_t st) {
    if (causal) return drop ? seq_launch_fwd_as<HD, true, true>(a, st) : seq_launch_fwd_as<HD, false, true>(a, st);
    return drop ? seq_launch_fwd_as<HD, true, false>(a, st) : seq_launch_fwd_as<HD, false, false>(a, st);
}

template <int HD>
int seq_launch_bwd(const SeqArgs& a, bool drop, bool causal, hipStream_t st) {
    if (causal) return drop ? seq_launch_bwd_as<HD, true, true>(a, st) : seq_launch_bwd_as<HD, false, true>(a, st);
    return drop ? seq_launch_bwd_as<HD, true, false>(a, st) : seq_launch_bwd_as<HD, false, false>(a, st);
}

}  // namespace

extern "C" {

size_t rlt_seq_attention_bwd_workspace(int S, int B, int H, int HD, float drop_p, int precision) {
    RLT_PREC_SCOPE_SZ(precision);
    (void)S; (void)B; (void)H; (void)HD; (void)drop_p;
    return 0;          // dQ, dK and dV are finished inside one workgroup: nothing to stage, nothing to sum
}

int rlt_seq_attention_fwd_ex(const float* qkv, int S, int B, int H, int HD, float drop_p, uint32_t seed, int mask,
                             float* out, float* lse, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(qkv && out && lse);
    RLT_CHECK_ARG(mask == RLT_SEQ_MASK_NONE || mask == RLT_SEQ_MASK_CAUSAL);
    if (int rc = seq_check_dims(S, B, H, HD, drop_p)) return rc;
    if (!rlt_aligned16(qkv) || !rlt_aligned16(out) || !rlt_aligned16(lse)) return RLT_E_ALIGN;
    SeqArgs a = seq_args(S, B, H, HD, drop_p, seed);
    a.qkv = qkv; a.o = out; a.lse_o = lse;
    const bool causal = mask == RLT_SEQ_MASK_CAUSAL;
    return HD == 64 ? seq_launch_fwd<64>(a, drop_p > 0.f, causal, rlt_stream(stream))
                    : seq_launch_fwd<16>(a, drop_p > 0.f, causal, rlt_stream(stream));
}

int rlt_seq_attention_fwd(const float* qkv, int S, int B, int H, int HD, float drop_p, uint32_t seed,
                          float* out, float* lse, int precision, void* stream) {
    return rlt_seq_attention_fwd_ex(qkv, S, B, H, HD, drop_p, seed, RLT_SEQ_MASK_NONE, out, lse, precision, stream);
}

int rlt_seq_attention_bwd_ex(const float* qkv, const float* out, const float* dout, const float* lse,
                             int S, int B, int H, int HD, float drop_p, uint32_t seed, int mask, float* dqkv,
                             void* ws, size_t ws_bytes, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(qkv && out && dout && lse && dqkv);
    RLT_CHECK_ARG(mask == RLT_SEQ_MASK_NONE || mask == RLT_SEQ_MASK_CAUSAL);
    if (int rc = seq_check_dims(S, B, H, HD, drop_p)) return rc;
    if (!rlt_aligned16(qkv) || !rlt_aligned16(out) || !rlt_aligned16(dout) || !rlt_aligned16(lse) || !rlt_aligned16(dqkv) ||
        !rlt_aligned16(ws))
        return RLT_E_ALIGN;
    if (ws_bytes < rlt_seq_attention_bwd_workspace(S, B, H, HD, drop_p, precision)) return RLT_E_WORKSPACE;   // 0 bytes: ws may be NULL
    SeqArgs a = seq_args(S, B, H, HD, drop_p, seed);
    a.qkv = qkv; a.out = out; a.dout = dout; a.lse = lse; a.dqkv = dqkv;
    const bool causal = mask == RLT_SEQ_MASK_CAUSAL;
    return HD == 64 ? seq_launch_bwd<64>(a, drop_p > 0.f, causal, rlt_stream(stream))
                    : seq_launch_bwd<16>(a, drop_p > 0.f, causal, rlt_stream(stream));
}

int rlt_seq_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                          int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv,
                          void* ws, size_t ws_bytes, int precision, void* stream) {
    return rlt_seq_attention_bwd_ex(qkv, out, dout, lse, S, B, H, HD, drop_p, seed, RLT_SEQ_MASK_NONE, dqkv, ws, ws_bytes, precision,
                                    stream);
}

}  // extern "C"
