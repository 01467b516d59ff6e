// K/V-cached append forward of the causal within-list attention: rlt_seq_attention_append of include/rlt_hip.h.  A chunk of C new
// ranks t0 .. t0+C-1 of every list arrives as qkv_chunk (C*B, 3E); the K and V rows of the ranks before it live in kv_cache
// (Smax*B, 2E), row s*B + b = [K | V] of rank s.  The call appends the chunk's K | V rows to the cache and computes the causal
// attention of the C new queries over ranks 0 .. t0+i - inference only: no dropout, no backward.
//
// Geometry: that of seq_attn_fwd_kernel<HD, false, true> (attention_seq.hip), from the same device functions
// (attention_seq_tile.h).  A workgroup owns 64 columns of one list, the owned query is on the lane, products on the 32x32x2 fp32
// MFMA, running maximum and normaliser rescaled per 32-key sub-tile.  The chunk's queries are taken in passes aligned to ABSOLUTE
// multiples of the pass (128 ranks at head dim 64, 32 at head dim 16), so a wavefront's 32 queries are the ranks 32 j .. 32 j + 31
// they are in the one-shot kernel; a wavefront without a rank of the chunk only stages.  Row q visits the sub-tiles
// 0 .. floor(q / 32) in that order, keys > q take weight 0 by the same compare, and the rows >= t0+C of a tile are staged as
// zeros where the one-shot kernel stages the ranks behind q (weight 0 either way: the one thing this can change is the sign of an
// exactly-zero sum).  So out and lse of rank q are, as fp32 values, what rlt_seq_attention_fwd_ex computes under
// RLT_SEQ_MASK_CAUSAL for the whole list - whatever the chunking.
//
// Cache visibility: a tile is staged from TWO sources - ranks < t0 from the cache, ranks t0 .. t0+C-1 from the chunk itself,
// ranks >= t0+C as zeros - so the kernel never reads a cache row it writes in the same launch, and no fence or second launch
// stands between the append and the attention.  A workgroup writes the cache columns it owns (its 64 of K and of V), once.
// A retired list (active[b] == 0) is skipped by its workgroups before anything is read or written.
//
// What is not fast: at C = 1 one of a wavefront's 32 query lanes works, and at head dim 64 three of the four wavefronts only
// stage; the call is then bound by reading the cache.  The key range is not split across wavefronts: that would change the
// order of the sums and give up the bit-for-bit contract above.
#include "attention_seq_tile.h"

namespace {

struct SeqAppendArgs {
    const float* chunk; float* cache; const int32_t* active;
    float* o; float* lse_o;
    int t0, C, B, H;
    float scale;
};

// rows row0 .. row0+63 of list b, columns c0 .. c0+cw-1 of K (koff = 0) or V (koff = E) -> tile[64][SQ_LD], as sq_stage lays it
// out: ranks < t0 from the cache (2E floats per row), ranks t0 .. send-1 from the chunk (3E floats per row, K | V behind Q), ranks
// >= send and columns >= cw as zeros
__device__ __forceinline__ void sqa_stage(float* __restrict__ tile, const float* __restrict__ cache, const float* __restrict__ chunk,
                                          int E, int koff, int B, int b, int row0, int t0, int send, int c0, int cw, int tid) {
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, c4 = (idx & 15) * 4, row = row0 + r;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < send && c4 < cw) {
            const float* src = row < t0 ? cache + ((size_t)row * B + b) * (2 * (size_t)E) + koff
                                        : chunk + ((size_t)(row - t0) * B + b) * (3 * (size_t)E) + E + koff;
            v[i] = *reinterpret_cast<const float4*>(src + c0 + c4);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 4, c4 = (idx & 15) * 4;
        *reinterpret_cast<float4*>(tile + r * SQ_LD + c4) = v[i];
    }
}

template <int HD>
__global__ __launch_bounds__(256) void seq_attn_append_kernel(SeqAppendArgs a) {
    using G = SeqGeom<HD>;
    constexpr int HPG = G::HPG, OWN = G::OWN, DT = G::DT, KH = G::KH;
    __shared__ __attribute__((aligned(16))) float Ks[SQ_TR * SQ_LD];
    __shared__ __attribute__((aligned(16))) float Vs[SQ_TR * SQ_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l31 = lane & 31;
    const int t0 = a.t0, C = a.C, B = a.B, H = a.H;
    const int send = t0 + C;                      // the list as far as it is known: what S is to the one-shot kernel
    const int ngrp = (H + HPG - 1) / HPG;
    const int b = blockIdx.x / ngrp, h0 = (blockIdx.x % ngrp) * HPG;
    if (a.active && a.active[b] == 0) return;     // block-uniform: a retired list costs its workgroups one load
    const int nh = H - h0 < HPG ? H - h0 : HPG;
    const int E = H * HD;
    const size_t ld = 3 * (size_t)E;
    const int c0 = h0 * HD, cw = nh * HD;
    const int hw = HPG == 1 ? 0 : w;
    const int h = h0 + hw, hc = hw * HD;
    const int woff = HPG == 1 ? 32 * w : 0;
    const int dcol = hc + (HD == 16 ? (l31 & 15) : l31);
    const float c = a.scale * LOG2E;

    // ---- append: the chunk's K | V rows, this workgroup's columns, into cache rows t0 .. t0+C-1 (never read back below)
    {
        const int per = cw / 4, n = 2 * per * C;  // float4s: C rows of [K columns | V columns]
        for (int idx = tid; idx < n; idx += 256) {
            const int i = idx / (2 * per), j = idx % (2 * per), kv = j / per, c4 = (j % per) * 4;
            const float4 v = *reinterpret_cast<const float4*>(a.chunk + ((size_t)i * B + b) * ld + (size_t)(1 + kv) * E + c0 + c4);
            *reinterpret_cast<float4*>(a.cache + ((size_t)(t0 + i) * B + b) * (2 * (size_t)E) + (size_t)kv * E + c0 + c4) = v;
        }
    }

    // ---- attention of the chunk's queries, in the one-shot kernel's passes
    for (int q0 = t0 / OWN * OWN; q0 < send; q0 += OWN) {
        const int q = q0 + woff + l31;
        const bool q_on = q >= t0 && q < send;    // this lane's query is a rank of the chunk
        const bool wave_on = hw < nh && q0 + woff < send && q0 + woff + 31 >= t0;
        float qr[KH];
#pragma unroll
        for (int i = 0; i < KH; ++i) qr[i] = 0.f;
        if (wave_on && q_on) sq_load_row<KH>(qr, a.chunk + ((size_t)(q - t0) * B + b) * ld + c0 + hc + hh * KH);
        f32x16 acc[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
        float m = -INFINITY, lsum = 0.f;

        const int kend = sq_key_end(send, q0 + OWN);                // block-uniform: staging is collective
        for (int k0 = 0; k0 < kend; k0 += SQ_TR) {
            __syncthreads();
            sqa_stage(Ks, a.cache, a.chunk, E, 0, B, b, k0, t0, send, c0, cw, tid);
            sqa_stage(Vs, a.cache, a.chunk, E, E, B, b, k0, t0, send, c0, cw, tid);
            __syncthreads();
            if (!wave_on) continue;
#pragma unroll 1
            for (int sub = 0; sub < SQ_TR / 32; ++sub) {
                const int kb = k0 + 32 * sub;
                if (kb >= send) break;
                if (kb > q0 + woff + 31) break;             // every key of the sub-tile lies behind the wavefront's last query
                f32x16 s = sq_rows_dot<KH>(Ks + (32 * sub + l31) * SQ_LD + hc + hh * KH, qr);
                float mx = m;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = sq_admit(kb + acc_row(r, hh), q, send) ? s[r] * c : -INFINITY;
                    s[r] = sv;
                    mx = fmaxf(mx, sv);
                }
                // the online-softmax step of seq_attn_fwd_kernel, operation for operation (no dropout here)
                mx = fmaxf(mx, __shfl_xor(mx, 32));          // key kb itself is <= the wavefront's queries: finite from key 0 on
                const float alpha = rlt_exp2(m - mx);
                m = mx;
                lsum *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[dt][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = rlt_exp2(s[r] - mx);
                    lsum += p;
                    s[r] = p;
                }
                sq_cols_acc<DT>(acc, Vs + 32 * sub * SQ_LD + dcol, hh, s);
            }
        }
        if (wave_on) {
            lsum += __shfl_xor(lsum, 32);
            if (q_on) {
                sq_store_T<HD>(a.o + ((size_t)(q - t0) * B + b) * E + c0 + hc, hh, acc, 1.f / lsum);
                if (a.lse_o && hh == 0) a.lse_o[((size_t)b * H + h) * C + (q - t0)] = (m + log2f(lsum)) * LN2;
            }
        }
    }
}

template <int HD>
int seq_append_launch(const SeqAppendArgs& a, hipStream_t st) {
    const int ngrp = (a.H + SeqGeom<HD>::HPG - 1) / SeqGeom<HD>::HPG;
    const dim3 grid((unsigned)((long long)a.B * ngrp)), block(256);
    hipLaunchKernelGGL((seq_attn_append_kernel<HD>), grid, block, 0, st, a);
    return RLT_LAUNCH_RESULT();
}

}  // namespace

extern "C" {

int rlt_seq_attention_append(const float* qkv_chunk, float* kv_cache, int t0, int C, int Smax, int B, int H, int HD,
                             const int32_t* active, float* out, float* lse, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(qkv_chunk && kv_cache && out);
    RLT_CHECK_ARG(C > 0 && Smax > 0 && t0 >= 0 && (long long)t0 + C <= Smax);
    if (int rc = seq_check_dims(Smax, B, H, HD, 0.f)) return rc;
    if (!rlt_aligned16(qkv_chunk) || !rlt_aligned16(kv_cache) || !rlt_aligned16(out) || !rlt_aligned16(lse)) return RLT_E_ALIGN;
    SeqAppendArgs a{};
    a.chunk = qkv_chunk; a.cache = kv_cache; a.active = active; a.o = out; a.lse_o = lse;
    a.t0 = t0; a.C = C; a.B = B; a.H = H;
    a.scale = 1.0f / sqrtf((float)HD);
    return HD == 64 ? seq_append_launch<64>(a, rlt_stream(stream)) : seq_append_launch<16>(a, rlt_stream(stream));
}

}  // extern "C"
