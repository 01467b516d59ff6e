// BiLSTM recurrence, hidden size 128 (row M2 of SURVEY.md section 8a; nn.LSTM call sites
// models/AttnCut.py:8,17, models/MtAttnCut.py:8,22, models/MMOECut.py:63,88).
//
// The time loop is strictly sequential (S steps per direction), so it runs as ONE persistent
// launch per layer: a workgroup of 16 wavefronts owns 32 ranked lists of one direction for all
// S steps.  W_hh (512x128 fp32 = 256 KB) does not fit LDS (160 KB); it lives in REGISTERS,
// 64 VGPRs per lane across the 1024 threads, as the A operand of v_mfma_f32_32x32x2_f32:
//   wavefront w owns hidden units 8w..8w+7 and their 4 gates (32 rows of W_hh);
//   accumulator row m <-> (gate m>>3, unit 8w + (m&7)), accumulator column <-> list.
// In the MFMA accumulator layout a lane then holds i,f,g,o of the SAME (list, unit) in registers
// r, r+4, r+8, r+12, so the cell update is lane-local.  h_{t-1} (32 lists x 128) is exchanged
// through a double-buffered LDS tile; one barrier per step.  The input projections
// x_t W_ih^T + b_ih + b_hh for all steps were produced beforehand by one large rlt_gemm and are
// streamed in (loads issued before the MFMA chain, consumed after it).
//
// Backward is the reverse-time recurrence: dA_t (gradient of the pre-activation gates) is
// computed lane-locally and fed straight from registers as the MFMA B operand of
// dh_{t-1} = W_hh^T dA_t; the contraction runs over gate rows, which are spread over the 16
// wavefronts, so the 16 partial products are reduced through LDS in a fixed order
// (deterministic).  dA is written in place over the gate stash; dW_ih, dW_hh, db and dx are then
// plain GEMMs / column sums on it (position-major layout makes h_{t-1} a row offset of B).
#include "common.h"
#include "lstm_common.h"
#include "split6.h"
#include <stdlib.h>

namespace {

constexpr int HID = 128;
constexpr int LISTS = 32;
constexpr int LDH = 132;      // LDS row stride of the h tile (floats)
constexpr int LDP = 68;       // LDS row stride of the partial dh tiles (floats)

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Fused input projection for narrow inputs (I <= 3, the reference's score / tf-idf / doc2vec features): instead of a
// separate GEMM writing x W_ih^T + b_ih + b_hh to HBM (4 KB per token) and the recurrence reading it back, the
// recurrence computes the 16 pre-activations of a lane from the I input values of its list and a per-direction table
// (row -> W_ih[row][0..2], b_ih[row] + b_hh[row]) kept in LDS (8 KB; all lanes of a wavefront read the same two
// addresses, a broadcast).
using XIn = RltXIn;
__device__ __forceinline__ void xin_table(const XIn& xi, int dir, int tid, int nthreads, float4* tab) {
    for (int row = tid; row < 4 * 128; row += nthreads) {
        const float* wr = xi.w_ih[dir] + (size_t)row * xi.I;
        float4 t;
        t.x = wr[0];
        t.y = xi.I > 1 ? wr[1] : 0.f;
        t.z = xi.I > 2 ? wr[2] : 0.f;
        t.w = xi.b_ih[dir][row] + xi.b_hh[dir][row];
        tab[row] = t;
    }
}
__device__ __forceinline__ void xin_gates(const XIn& xi, const float4* tab, size_t tok, int ucol, float4 (&gin)[4]) {
    const float* xr = xi.x + tok * xi.I;
    const float x0 = xr[0], x1 = xi.I > 1 ? xr[1] : 0.f, x2 = xi.I > 2 ? xr[2] : 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 t = tab[g * 128 + ucol + u];
            v[u] = ((t.x * x0 + t.y * x1) + t.z * x2) + t.w;
        }
        gin[g] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

template <bool XIN>
__global__ __launch_bounds__(1024) void bilstm_fwd_kernel(float* __restrict__ gates, const float* __restrict__ w_hh_f,
                                                          const float* __restrict__ w_hh_r, int S, int B, float* __restrict__ h_out,
                                                          float* __restrict__ c_out, XIn xi) {
    __shared__ __attribute__((aligned(16))) float hs[2][LISTS * LDH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.y;
    const int b = blockIdx.x * LISTS + l31;
    const bool valid = b < B;

    // A operand: W_hh rows of this wavefront (gate l31>>3, unit 8w + (l31&7)), k = hh*64 + ks
    float wreg[64];
    // XIN (layer 0): the input projection x W_ih^T + b_ih + b_hh rides on the same accumulators as TWO more MFMAs - k pairs
    // (x0, x1) and (x2, 1) against (W_ih[row][0], W_ih[row][1]) and (W_ih[row][2], b_ih[row] + b_hh[row]): exact fp32
    // products like every other one of the chain.  The LDS table + 16 float4 reads + 48 FMAs per lane and step this replaces
    // pushed 32 of the 64 W_hh registers into scratch, re-read at every step: 10 GB of scratch reads per launch (the 8.8 GB
    // against 2.5 GB of VERDICT r03 item 6).
    float wx0 = 0.f, wx1 = 0.f;
    {
        const int row = (l31 >> 3) * HID + 8 * w + (l31 & 7);
        const float* wp = (dir ? w_hh_r : w_hh_f) + (size_t)row * HID + hh * 64;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(wp + 4 * q);
            wreg[4 * q + 0] = v.x; wreg[4 * q + 1] = v.y; wreg[4 * q + 2] = v.z; wreg[4 * q + 3] = v.w;
        }
        if (XIN) {
            const float* wr = xi.w_ih[dir] + (size_t)row * xi.I;
            wx0 = hh == 0 ? wr[0] : (xi.I > 1 ? wr[1] : 0.f);
            wx1 = hh == 0 ? (xi.I > 2 ? wr[2] : 0.f) : xi.b_ih[dir][row] + xi.b_hh[dir][row];
        }
    }
    for (int i = tid; i < LISTS * LDH; i += 1024) hs[0][i] = 0.f;      // h_0 = 0
    float c[4] = {0.f, 0.f, 0.f, 0.f};                                  // c_0 = 0
    const int ucol = 8 * w + 4 * hh;                                    // first of this lane's 4 units
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < S; ++t) {
        const int s = dir ? S - 1 - t : t;
        const size_t tok = (size_t)s * B + (valid ? b : 0);
        float* grow = gates + tok * (8 * HID) + dir * 4 * HID + ucol;
        float4 gin[4];
        float xb0 = 0.f, xb1 = 0.f;                // B operands of the two input-projection MFMAs: (x0 | x1), (x2 | 1)
        if (XIN) {                                 // (invalid lists read list 0's row, never stored)
            const float* xr = xi.x + tok * xi.I;
            xb0 = hh == 0 ? xr[0] : (xi.I > 1 ? xr[1] : 0.f);
            xb1 = hh == 0 ? (xi.I > 2 ? xr[2] : 0.f) : 1.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) gin[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g)    // unconditional (invalid lists read list 0's row, never stored); consumed after the MFMAs
                gin[g] = *reinterpret_cast<const float4*>(grow + g * HID);
        }

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* hp = hs[cur] + l31 * LDH + hh * 64;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float4 hv = *reinterpret_cast<const float4*>(hp + 4 * q);
            acc = mfma32(wreg[4 * q + 0], hv.x, acc);
            acc = mfma32(wreg[4 * q + 1], hv.y, acc);
            acc = mfma32(wreg[4 * q + 2], hv.z, acc);
            acc = mfma32(wreg[4 * q + 3], hv.w, acc);
        }
        if (XIN) {
            acc = mfma32(wx0, xb0, acc);
            acc = mfma32(wx1, xb1, acc);
        }
        const float* gi_ = reinterpret_cast<const float*>(&gin[0]);
        float act[16], hnew[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float ig = sigmoidf_(acc[u] + gi_[u]);
            const float fg = sigmoidf_(acc[4 + u] + gi_[4 + u]);
            const float gg = tanhf(acc[8 + u] + gi_[8 + u]);
            const float og = sigmoidf_(acc[12 + u] + gi_[12 + u]);
            c[u] = fg * c[u] + ig * gg;
            hnew[u] = og * tanhf(c[u]);
            act[u] = ig; act[4 + u] = fg; act[8 + u] = gg; act[12 + u] = og;
        }
        if (valid) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(grow + g * HID) = make_float4(act[4 * g], act[4 * g + 1], act[4 * g + 2], act[4 * g + 3]);
            *reinterpret_cast<float4*>(c_out + (tok * 2 + dir) * HID + ucol) = make_float4(c[0], c[1], c[2], c[3]);
            *reinterpret_cast<float4*>(h_out + tok * (2 * HID) + dir * HID + ucol) = make_float4(hnew[0], hnew[1], hnew[2], hnew[3]);
        }
        *reinterpret_cast<float4*>(&hs[cur ^ 1][l31 * LDH + ucol]) = make_float4(hnew[0], hnew[1], hnew[2], hnew[3]);
        __syncthreads();
        cur ^= 1;
    }
}

__global__ __launch_bounds__(1024) void bilstm_bwd_kernel(float* __restrict__ gates, const float* __restrict__ cst,
                                                          const float* __restrict__ w_hh_f, const float* __restrict__ w_hh_r,
                                                          const float* __restrict__ d_hout, int S, int B) {
    extern __shared__ __attribute__((aligned(16))) float P[];           // [16][LISTS][LDP]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.y;
    const int b = blockIdx.x * LISTS + l31;
    const bool valid = b < B;
    const int ucol = 8 * w + 4 * hh;

    // A operand of dh = W_hh^T dA: wT[a][r] = W_hh[(r>>2)*128 + 8w + 4hh + (r&3)][a*32 + l31]
    float wT[4][16];
    {
        const float* wp = dir ? w_hh_r : w_hh_f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* rp = wp + (size_t)((r >> 2) * HID + ucol + (r & 3)) * HID + l31;
#pragma unroll
            for (int a = 0; a < 4; ++a) wT[a][r] = rp[a * 32];
        }
    }
    float dc[4] = {0.f, 0.f, 0.f, 0.f}, dhrec[4] = {0.f, 0.f, 0.f, 0.f};

    for (int t = S - 1; t >= 0; --t) {
        const int s = dir ? S - 1 - t : t;
        const size_t tok = (size_t)s * B + (valid ? b : 0);
        float* grow = gates + tok * (8 * HID) + dir * 4 * HID + ucol;
        float dA[16];
        if (valid) {
            float4 gv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gv[g] = *reinterpret_cast<const float4*>(grow + g * HID);
            const float4 ct4 = *reinterpret_cast<const float4*>(cst + (tok * 2 + dir) * HID + ucol);
            float4 cp4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t > 0) {
                const size_t tokp = (size_t)(dir ? s + 1 : s - 1) * B + b;
                cp4 = *reinterpret_cast<const float4*>(cst + (tokp * 2 + dir) * HID + ucol);
            }
            const float4 dh4 = *reinterpret_cast<const float4*>(d_hout + tok * (2 * HID) + dir * HID + ucol);
            const float* gf_ = reinterpret_cast<const float*>(&gv[0]);
            const float* ct = reinterpret_cast<const float*>(&ct4);
            const float* cp = reinterpret_cast<const float*>(&cp4);
            const float* dho = reinterpret_cast<const float*>(&dh4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float ig = gf_[u], fg = gf_[4 + u], gg = gf_[8 + u], og = gf_[12 + u];
                const float dh = dho[u] + dhrec[u];
                const float tc = tanhf(ct[u]);
                const float dcu = dc[u] + dh * og * (1.f - tc * tc);
                dA[u] = dcu * gg * ig * (1.f - ig);
                dA[4 + u] = dcu * cp[u] * fg * (1.f - fg);
                dA[8 + u] = dcu * ig * (1.f - gg * gg);
                dA[12 + u] = dh * tc * og * (1.f - og);
                dc[u] = dcu * fg;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(grow + g * HID) = make_float4(dA[4 * g], dA[4 * g + 1], dA[4 * g + 2], dA[4 * g + 3]);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) dA[r] = 0.f;
        }
        if (t == 0) break;                         // dh_{-1} is not needed
        // dh_{t-1}[list][k] = sum_rows dA[list][row] W_hh[row][k]; k tiles {0,1} then {2,3}
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc0 = mfma32(wT[2 * rd][r], dA[r], acc0);
                acc1 = mfma32(wT[2 * rd + 1][r], dA[r], acc1);
            }
            float* pw = P + (size_t)(w * LISTS + l31) * LDP + 4 * hh;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<float4*>(pw + 8 * g) = make_float4(acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]);
                *reinterpret_cast<float4*>(pw + 32 + 8 * g) = make_float4(acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]);
            }
            __syncthreads();
            if ((w >> 3) == rd) {
                const float* pr = P + (size_t)l31 * LDP + 8 * (w & 7) + 4 * hh;
                float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int ww = 0; ww < 16; ++ww) {
                    const float4 v = *reinterpret_cast<const float4*>(pr + (size_t)ww * LISTS * LDP);
                    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
                }
                dhrec[0] = sum.x; dhrec[1] = sum.y; dhrec[2] = sum.z; dhrec[3] = sum.w;
            }
            __syncthreads();
        }
    }
}

// ======================================================================================================
// Split-bf16 ("bf16x3") variants: the recurrent products h W_hh^T and W_hh^T dA on v_mfma_f32_32x32x16_bf16 with
// every operand split into bf16 hi + lo (3 products, fp32 accumulate); W_hh fragments still live in registers
// (64 VGPRs), h_{t-1} is exchanged through LDS already split.  Gate nonlinearities use v_exp/v_rcp forms.
constexpr int LDH3 = 136;      // bf16 elements per row of the h tile images (272 B)

// sigmoid / tanh on the hardware exp2 + rcp (abs error ~1e-7, far inside the 1e-4 parity bound)
__device__ __forceinline__ float fsigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + rlt_exp2(-1.4426950408889634f * x)); }
__device__ __forceinline__ float ftanh(float x) { return 2.f * fsigmoid(2.f * x) - 1.f; }

template <bool XIN>
__global__ __launch_bounds__(1024) void bilstm3_fwd_kernel(float* __restrict__ gates, const float* __restrict__ w_hh_f,
                                                           const float* __restrict__ w_hh_r, int S, int B,
                                                           float* __restrict__ h_out, float* __restrict__ c_out, XIn xi) {
    __shared__ __attribute__((aligned(16))) uint16_t hs[2][2][LISTS * LDH3];        // [buffer][hi|lo]
    __shared__ float4 xtab[XIN ? 4 * HID : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.y;
    const int b = blockIdx.x * LISTS + l31;
    const bool valid = b < B;

    // A operand: W_hh rows of this wavefront (gate l31>>3, unit 8w + (l31&7)); fragment ks covers k = 16ks + 8hh + j
    bf16x8 wh[8], wl[8];
    {
        const float* wp = (dir ? w_hh_r : w_hh_f) + (size_t)((l31 >> 3) * HID + 8 * w + (l31 & 7)) * HID + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const float4 v0 = *reinterpret_cast<const float4*>(wp + 16 * ks);
            const float4 v1 = *reinterpret_cast<const float4*>(wp + 16 * ks + 4);
            const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            split8(x, wh[ks], wl[ks]);
        }
    }
    for (int i = tid; i < 2 * LISTS * LDH3; i += 1024) (&hs[0][0][0])[i] = 0;       // h_0 = 0 (hi and lo images)
    if (XIN) xin_table(xi, blockIdx.y, tid, 1024, xtab);
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    const int ucol = 8 * w + 4 * hh;
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < S; ++t) {
        const int s = dir ? S - 1 - t : t;
        const size_t tok = (size_t)s * B + (valid ? b : 0);
        float* grow = gates + tok * (8 * HID) + dir * 4 * HID + ucol;
        float4 gin[4];
        if (XIN) xin_gates(xi, xtab, tok, ucol, gin);
        else {
#pragma unroll
            for (int g = 0; g < 4; ++g)    // unconditional (invalid lists read list 0's row, never stored); consumed after the MFMAs
                gin[g] = *reinterpret_cast<const float4*>(grow + g * HID);
        }
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const uint16_t* hph = hs[cur][0] + l31 * LDH3 + 8 * hh;
        const uint16_t* hpl = hs[cur][1] + l31 * LDH3 + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(hph + 16 * ks);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(hpl + 16 * ks);
            acc = mfma3(wh[ks], wl[ks], bh, bl, acc);
        }
        const float* gi_ = reinterpret_cast<const float*>(&gin[0]);
        float act[16], hnew[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float ig = fsigmoid(acc[u] + gi_[u]);
            const float fg = fsigmoid(acc[4 + u] + gi_[4 + u]);
            const float gg = ftanh(acc[8 + u] + gi_[8 + u]);
            const float og = fsigmoid(acc[12 + u] + gi_[12 + u]);
            c[u] = fg * c[u] + ig * gg;
            hnew[u] = og * ftanh(c[u]);
            act[u] = ig; act[4 + u] = fg; act[8 + u] = gg; act[12 + u] = og;
        }
        if (valid) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(grow + g * HID) = make_float4(act[4 * g], act[4 * g + 1], act[4 * g + 2], act[4 * g + 3]);
            *reinterpret_cast<float4*>(c_out + (tok * 2 + dir) * HID + ucol) = make_float4(c[0], c[1], c[2], c[3]);
            *reinterpret_cast<float4*>(h_out + tok * (2 * HID) + dir * HID + ucol) = make_float4(hnew[0], hnew[1], hnew[2], hnew[3]);
        }
        uint2 h2, l2;
        split4(hnew[0], hnew[1], hnew[2], hnew[3], h2, l2);
        *reinterpret_cast<uint2*>(&hs[cur ^ 1][0][l31 * LDH3 + ucol]) = h2;
        *reinterpret_cast<uint2*>(&hs[cur ^ 1][1][l31 * LDH3 + ucol]) = l2;
        __syncthreads();
        cur ^= 1;
    }
}

// Split-bf16 backward recurrence, 512 threads: 8 wavefronts x 16 hidden units, two wavefronts per SIMD and therefore a
// 256-VGPR budget.  (A 1024-thread form like the forward kernel's has 128 VGPRs per lane, half of them taken by the
// W_hh^T fragments; it spilled 9 fragments that were reloaded from scratch every time step: ~11 GB of extra memory
// traffic per launch, profiles/r01_i_pmc_traffic.json.)  Nothing spills, the partial dh tiles of all four 32-column
// blocks fit LDS at once (one exchange per step) and the sum runs over 8 partials.
constexpr int LDP8 = 132;      // floats per row of a partial dh tile (128 + 4)
__global__ __launch_bounds__(512) void bilstm3_bwd8_kernel(float* __restrict__ gates, const float* __restrict__ cst,
                                                           const float* __restrict__ w_hh_f, const float* __restrict__ w_hh_r,
                                                           const float* __restrict__ d_hout, int S, int B) {
    extern __shared__ __attribute__((aligned(16))) float P[];           // [8][LISTS][LDP8]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.y;
    const int b = blockIdx.x * LISTS + l31;
    const bool valid = b < B;
    const int ucol = 16 * w + 8 * hh;          // this lane's 8 hidden units

    // dh = W_hh^T dA with the lane's own dA values as the B operand.  k-step (p, uh): element j <-> gate 2p + (j>>2),
    // unit ucol + 4uh + (j&3); the A fragment (32-column block a) holds the same rows of W_hh at column 32a + l31.
    bf16x8 wth[4][4], wtl[4][4];
    {
        const float* wp = dir ? w_hh_r : w_hh_f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int pgate = ks >> 1, uh = ks & 1;
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    x[j] = wp[(size_t)((2 * pgate + (j >> 2)) * HID + ucol + 4 * uh + (j & 3)) * HID + a * 32 + l31];
                split8(x, wth[a][ks], wtl[a][ks]);
            }
    }
    float dc[8], dhrec[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { dc[u] = 0.f; dhrec[u] = 0.f; }

    // Operands of a time step (the lane's 2 x 4 units): the stashed gates i,f,g,o, dL/dh_out and c_{t-1}.  None of them
    // depends on the recurrence, so the set of step t-1 is fetched while step t runs its MFMAs and the partial-sum
    // exchange (with the loads at the top of the step, every one of the S steps exposed a full HBM latency);
    // c_t of step t-1 is c_{t-1} of step t and is kept.
    struct StepIn { float4 gv[2][4], cp[2], dh[2]; };
    auto tok_of = [&](int t) { return (size_t)(dir ? S - 1 - t : t) * B + (valid ? b : 0); };
    auto fetch = [&](int t, StepIn& in) {
        const size_t tok = tok_of(t), tokp = tok_of(t > 0 ? t - 1 : t);
        const float* grow = gates + tok * (8 * HID) + dir * 4 * HID + ucol;
#pragma unroll
        for (int uh = 0; uh < 2; ++uh) {
#pragma unroll
            for (int g = 0; g < 4; ++g) in.gv[uh][g] = *reinterpret_cast<const float4*>(grow + g * HID + 4 * uh);
            in.cp[uh] = *reinterpret_cast<const float4*>(cst + (tokp * 2 + dir) * HID + ucol + 4 * uh);   // step 0: unused (c_{-1} = 0)
            in.dh[uh] = *reinterpret_cast<const float4*>(d_hout + tok * (2 * HID) + dir * HID + ucol + 4 * uh);
        }
    };
    StepIn cur;
    float4 ctc[2];
    fetch(S - 1, cur);
#pragma unroll
    for (int uh = 0; uh < 2; ++uh) ctc[uh] = *reinterpret_cast<const float4*>(cst + (tok_of(S - 1) * 2 + dir) * HID + ucol + 4 * uh);

    for (int t = S - 1; t >= 0; --t) {
        float* grow = gates + tok_of(t) * (8 * HID) + dir * 4 * HID + ucol;
        bf16x8 dah[4], dal[4];
#pragma unroll
        for (int uh = 0; uh < 2; ++uh) {
            const float* gf_ = reinterpret_cast<const float*>(&cur.gv[uh][0]);
            const float* ct = reinterpret_cast<const float*>(&ctc[uh]);
            const float4 cp4 = t > 0 ? cur.cp[uh] : make_float4(0.f, 0.f, 0.f, 0.f);      // (no select at fetch time: it would wait for the load)
            const float* cp = reinterpret_cast<const float*>(&cp4);
            const float* dho = reinterpret_cast<const float*>(&cur.dh[uh]);
            float dA[16];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float ig = gf_[u], fg = gf_[4 + u], gg = gf_[8 + u], og = gf_[12 + u];
                const float dh = dho[u] + dhrec[4 * uh + u];
                const float tc = ftanh(ct[u]);
                const float dcu = dc[4 * uh + u] + dh * og * (1.f - tc * tc);
                dA[u] = valid ? dcu * gg * ig * (1.f - ig) : 0.f;
                dA[4 + u] = valid ? dcu * cp[u] * fg * (1.f - fg) : 0.f;
                dA[8 + u] = valid ? dcu * ig * (1.f - gg * gg) : 0.f;
                dA[12 + u] = valid ? dh * tc * og * (1.f - og) : 0.f;
                dc[4 * uh + u] = dcu * fg;
            }
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(grow + g * HID + 4 * uh) = make_float4(dA[4 * g], dA[4 * g + 1], dA[4 * g + 2], dA[4 * g + 3]);
            }
#pragma unroll
            for (int pgate = 0; pgate < 2; ++pgate) {
                const float x[8] = {dA[8 * pgate + 0], dA[8 * pgate + 1], dA[8 * pgate + 2], dA[8 * pgate + 3],
                                    dA[8 * pgate + 4], dA[8 * pgate + 5], dA[8 * pgate + 6], dA[8 * pgate + 7]};
                split8(x, dah[2 * pgate + uh], dal[2 * pgate + uh]);
            }
            ctc[uh] = cur.cp[uh];                  // c_{t-1}: the cell state of the step that runs next
        }
        if (t == 0) break;
        fetch(t - 1, cur);                         // in flight during the MFMAs and the exchange below
        float* pw = P + (size_t)(w * LISTS + l31) * LDP8 + 4 * hh;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) acc = mfma3(wth[a][ks], wtl[a][ks], dah[ks], dal[ks], acc);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(pw + 32 * a + 8 * g) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        }
        __syncthreads();
        {
            const float* pr = P + (size_t)l31 * LDP8 + ucol;
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
#pragma unroll
            for (int ww = 0; ww < 8; ++ww) {
                const float4 v0 = *reinterpret_cast<const float4*>(pr + (size_t)ww * LISTS * LDP8);
                const float4 v1 = *reinterpret_cast<const float4*>(pr + (size_t)ww * LISTS * LDP8 + 4);
                s0.x += v0.x; s0.y += v0.y; s0.z += v0.z; s0.w += v0.w;
                s1.x += v1.x; s1.y += v1.y; s1.z += v1.z; s1.w += v1.w;
            }
            dhrec[0] = s0.x; dhrec[1] = s0.y; dhrec[2] = s0.z; dhrec[3] = s0.w;
            dhrec[4] = s1.x; dhrec[5] = s1.y; dhrec[6] = s1.z; dhrec[7] = s1.w;
        }
        __syncthreads();
    }
}

// ======================================================================================================
// fp32-FAITHFUL forward recurrence ("bf16x6"): h W_hh^T on the exact three-way bf16 split of both
// operands (x = h + m + l, 8 + 8 + 8 significand bits), six MFMA products per fp32 product, fp32 accumulate - the scheme of
// gemm6*_kernel / attention6.hip; per (block, k-step) 6 x 32 matrix cycles against the 8 x 64 of the f32 MFMA.
// Where W_hh lives: its three planes are 384 KB per direction; the register file of a CU holds 512 KB.  512 threads = 8
// wavefronts x 16 hidden units (two 32-row MFMA blocks: rows = 4 gates x 8 units), a 256-register budget: the h and m planes
// stay in registers as A operands (128 VGPRs), the l plane - used by ONE of the six products, l h' - sits in LDS in
// fragment order (128 KB: every wavefront reads back exactly the 1 KB pieces it wrote, conflict-free), read once per
// (block, k-step).  h_{t-1} is exchanged through ONE 24 KB tile of three planes (LDS is full: 152 KB), so a step has two
// barriers (all fragments read | new h written); rows of 256 bytes, 16-byte chunks XOR-swizzled with the list index.
// Layer 0 (XIN): the input projection x W_ih^T + b_ih + b_hh rides on the same accumulators as one more k-step whose A
// fragments (W_ih columns, the bias sum, zeros; all three planes in registers) meet B = (x0, x1, x2, 1, 0...) - exact like
// every other product of the mode; the pre-activations never exist in memory.  Gate nonlinearities: hardware exp2 / rcp forms
// (abs error ~1e-7, measured against the libm forms of the f32 kernel in every fp32-tolerance test of the suite).
constexpr int WL6_BYTES = 8 * 2 * 8 * 64 * 16;          // l plane of W_hh in fragment order
constexpr int HX6_PLANE = LISTS * 256;                   // one plane of the h tile: 32 lists x 128 bf16
constexpr size_t LSTM6_LDS = (size_t)WL6_BYTES + 3 * HX6_PLANE;

// FULL: every workgroup holds 32 lists (B % 32 == 0): the stores are unconditional - behind an `if (valid)` hipcc loses the exact
// load / store counts at the join and waits with vmcnt(0), i.e. for the write acknowledgements of the step's stores.
template <bool XIN, bool FULL>
__global__ __launch_bounds__(512) void bilstm6_fwd_kernel(float* __restrict__ gates, const float* __restrict__ pre,
                                                          const float* __restrict__ w_hh_f,
                                                          const float* __restrict__ w_hh_r, int S, int B,
                                                          float* __restrict__ h_out, float* __restrict__ c_out, XIn xi) {
    // `pre` = `gates` (the pre-activations are overwritten in place by the activated gates, each row read one step before it is
    // written): a second name for the same buffer, so that hipcc's memory-counter bookkeeping does not tie the loads of the
    // next row to the stores of this one
    extern __shared__ __attribute__((aligned(16))) uint8_t sm6[];
    uint4* wl_s = reinterpret_cast<uint4*>(sm6);
    uint8_t* hx = sm6 + WL6_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.y;
    const int b = blockIdx.x * LISTS + l31;
    const bool valid = FULL || b < B;

    // A operand, block blk: row l31 <-> (gate l31 >> 3, unit 16 w + 8 blk + (l31 & 7)); fragment ks covers k = 16 ks + 8 hh + j
    bf16x8 wh[2][8], wm[2][8];
    bf16x8 wxh[2], wxm[2], wxl[2];                        // XIN: the input-projection k-step (W_ih columns, b_ih + b_hh, zeros)
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int row = (l31 >> 3) * HID + 16 * w + 8 * blk + (l31 & 7);
        const float* wp = (dir ? w_hh_r : w_hh_f) + (size_t)row * HID + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const float4 v0 = *reinterpret_cast<const float4*>(wp + 16 * ks);
            const float4 v1 = *reinterpret_cast<const float4*>(wp + 16 * ks + 4);
            const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            bf16x8 wl;
            split8x3<true>(x, wh[blk][ks], wm[blk][ks], wl);
            wl_s[((w * 2 + blk) * 8 + ks) * 64 + lane] = __builtin_bit_cast(uint4, wl);
        }
        if (XIN) {
            const float* wr = xi.w_ih[dir] + (size_t)row * xi.I;
            const bool lo_half = hh == 0;
            const float x[8] = {lo_half ? wr[0] : 0.f, (lo_half && xi.I > 1) ? wr[1] : 0.f, (lo_half && xi.I > 2) ? wr[2] : 0.f,
                                lo_half ? xi.b_ih[dir][row] + xi.b_hh[dir][row] : 0.f, 0.f, 0.f, 0.f, 0.f};
            split8x3<true>(x, wxh[blk], wxm[blk], wxl[blk]);
        }
    }
    for (int i = tid; i < 3 * HX6_PLANE / 16; i += 512) reinterpret_cast<uint4*>(hx)[i] = make_uint4(0u, 0u, 0u, 0u);   // h_0 = 0
    float c[2][4];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int u = 0; u < 4; ++u) c[blk][u] = 0.f;
    const int sw = l31 & 15;
    const uint8_t* hrow = hx + l31 * 256;
    __syncthreads();

    // Operands of a step that do not depend on the recurrence - the stashed pre-activations (layer 1) or the list's input row
    // (layer 0) - are fetched one step ahead, and the fetch of step t + 1 is issued BETWEEN the activations of step t (which
    // consume the registers) and its stores: vmcnt counts loads and stores in order, so loads issued behind the 12 stores of a
    // step would wait for the write acknowledgements of those stores before they could be consumed - one exposed HBM
    // write latency per step; in front of them, `s_waitcnt vmcnt(12)` lets the stores drain behind the next MFMA phase.
    float4 gin[2][4];
    float xv[3] = {0.f, 0.f, 0.f};
    auto tok_of = [&](int t) { return (size_t)(dir ? S - 1 - t : t) * B + (valid ? b : 0); };
    auto fetch = [&](int t) {              // (invalid lists read list 0's row, never stored)
        const size_t tk = tok_of(t);
        if (XIN) {
            const float* xr = xi.x + tk * xi.I;
            xv[0] = xr[0];
            if (xi.I > 1) xv[1] = xr[1];
            if (xi.I > 2) xv[2] = xr[2];
        } else {
            const float* gr = pre + tk * (8 * HID) + dir * 4 * HID + 16 * w + 4 * hh;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int g = 0; g < 4; ++g) gin[blk][g] = *reinterpret_cast<const float4*>(gr + g * HID + 8 * blk);
        }
    };
    fetch(0);
    asm volatile("" ::: "memory");             // (the loads stay in front of the stores below: hipcc sinks them into the loop preheader otherwise)
    if (FULL) {
        // the loop is entered with the same picture of outstanding operations as its back edge carries - 8 loads followed by
        // the 12 stores of a step - so that hipcc's merged count at the loop head is vmcnt(12), not the vmcnt(0) the bare
        // preheader (8 loads, nothing behind them) would force on every iteration.  The 12 stores go to step 0's own output
        // rows, which step 0 overwrites (same wavefront, same addresses, program order).
        const size_t tok = tok_of(0);
        float* grow = gates + tok * (8 * HID) + dir * 4 * HID + 16 * w + 4 * hh;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            if (!XIN) {        // (layer 1 reads the gate rows as its pre-activations: only c / h rows are free to touch - those of
                               //  the first three steps, each overwritten by its own step before anything reads it)
                const int ucol = 16 * w + 8 * blk + 4 * hh;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const size_t tq = tok_of(q < S ? q : S - 1);
                    *reinterpret_cast<float4*>(c_out + (tq * 2 + dir) * HID + ucol) = z;
                    *reinterpret_cast<float4*>(h_out + tq * (2 * HID) + dir * HID + ucol) = z;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(grow + g * HID + 8 * blk) = z;
                const int ucol = 16 * w + 8 * blk + 4 * hh;
                *reinterpret_cast<float4*>(c_out + (tok * 2 + dir) * HID + ucol) = z;
                *reinterpret_cast<float4*>(h_out + tok * (2 * HID) + dir * HID + ucol) = z;
            }
        }
    }
    for (int t = 0; t < S; ++t) {
        const size_t tok = tok_of(t);
        float* grow = gates + tok * (8 * HID) + dir * 4 * HID + 16 * w + 4 * hh;
        f32x16 acc[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[blk][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int co = ((2 * ks + hh) ^ sw) * 16;
            const bf16x8 xh = *reinterpret_cast<const bf16x8*>(hrow + co);
            const bf16x8 xm = *reinterpret_cast<const bf16x8*>(hrow + HX6_PLANE + co);
            const bf16x8 xl = *reinterpret_cast<const bf16x8*>(hrow + 2 * HX6_PLANE + co);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const bf16x8 wl = __builtin_bit_cast(bf16x8, wl_s[((w * 2 + blk) * 8 + ks) * 64 + lane]);
                acc[blk] = mfma6(wh[blk][ks], wm[blk][ks], wl, xh, xm, xl, acc[blk]);
            }
        }
        if (XIN) {            // + x_t W_ih^T + b_ih + b_hh: B = (x0, x1, x2, 1, 0, 0, 0, 0) in the lanes of k-half 0
            const bool lo_half = hh == 0;
            const float x[8] = {lo_half ? xv[0] : 0.f, lo_half ? xv[1] : 0.f, lo_half ? xv[2] : 0.f, lo_half ? 1.f : 0.f, 0.f, 0.f, 0.f, 0.f};
            bf16x8 xh, xm, xl;
            split8x3<true>(x, xh, xm, xl);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) acc[blk] = mfma6(wxh[blk], wxm[blk], wxl[blk], xh, xm, xl, acc[blk]);
        }
        __syncthreads();                                   // every wavefront has read its fragments of h_{t-1}
        float act[2][16], hnew[2][4];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const float* gi_ = reinterpret_cast<const float*>(&gin[blk][0]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float ig = fsigmoid(acc[blk][u] + (XIN ? 0.f : gi_[u]));
                const float fg = fsigmoid(acc[blk][4 + u] + (XIN ? 0.f : gi_[4 + u]));
                const float gg = ftanh(acc[blk][8 + u] + (XIN ? 0.f : gi_[8 + u]));
                const float og = fsigmoid(acc[blk][12 + u] + (XIN ? 0.f : gi_[12 + u]));
                c[blk][u] = fg * c[blk][u] + ig * gg;
                hnew[blk][u] = og * ftanh(c[blk][u]);
                act[blk][u] = ig; act[blk][4 + u] = fg; act[blk][8 + u] = gg; act[blk][12 + u] = og;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch(t + 1 < S ? t + 1 : t);                      // unconditional (the last step re-reads its own row): exact vmcnt counts
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(grow + g * HID + 8 * blk) =
                        make_float4(act[blk][4 * g], act[blk][4 * g + 1], act[blk][4 * g + 2], act[blk][4 * g + 3]);
                const int ucol = 16 * w + 8 * blk + 4 * hh;
                *reinterpret_cast<float4*>(c_out + (tok * 2 + dir) * HID + ucol) = make_float4(c[blk][0], c[blk][1], c[blk][2], c[blk][3]);
                *reinterpret_cast<float4*>(h_out + tok * (2 * HID) + dir * HID + ucol) =
                    make_float4(hnew[blk][0], hnew[blk][1], hnew[blk][2], hnew[blk][3]);
            }
            uint2 h2, m2, l2;
            split4x3<true>(hnew[blk][0], hnew[blk][1], hnew[blk][2], hnew[blk][3], h2, m2, l2);
            uint8_t* dst = hx + l31 * 256 + (((2 * w + blk) ^ sw) * 16) + 8 * hh;
            *reinterpret_cast<uint2*>(dst) = h2;
            *reinterpret_cast<uint2*>(dst + HX6_PLANE) = m2;
            *reinterpret_cast<uint2*>(dst + 2 * HX6_PLANE) = l2;
        }
        __syncthreads();                                   // h_t is in place
    }
}

}  // namespace

// Every environment switch of the recurrence, read once per process (A/B runs: bench.py, tools/x6_probe.py)
struct LstmEnv {
    bool lstm6;         // RLT_LSTM6=0: bf16x6 FORWARD on the f32 MFMA kernels
    bool lstm6w;        // RLT_LSTM6W=0: round 4's two-phase forward and the f32 MFMA backward instead of lstm6w.hip
    bool lstm6w_bwd;    // RLT_LSTM6W_BWD=0: the f32 MFMA backward recurrence of rounds 1-4 only
    bool single;        // RLT_LSTM6W_SINGLE=0: lstm6w.hip always in its two-half form
};
static const LstmEnv& lstm_env() {
    static const LstmEnv env = [] {
        auto on = [](const char* e) { return !e || atoi(e) != 0; };
        LstmEnv v;
        v.lstm6 = on(getenv("RLT_LSTM6"));
        v.lstm6w = on(getenv("RLT_LSTM6W"));
        v.lstm6w_bwd = on(getenv("RLT_LSTM6W_BWD"));
        v.single = on(getenv("RLT_LSTM6W_SINGLE"));
        return v;
    }();
    return env;
}

LstmPlan lstm_plan(int B) {
    const LstmEnv& env = lstm_env();
    const int prec = rlt_precision();
    // (lstm6w.hip bounds its buffer instructions with 32-bit byte counts of B * 4096: 2^20 lists and more take the kernels of this file)
    const bool w6_fits = B < (1 << 20);
    // one 16-list half per workgroup while that still gives every workgroup its own CU (256 CUs, two directions)
    const int w6 = env.single && B <= 16 * 128 ? RLT_LSTM_X6W_SINGLE : RLT_LSTM_X6W_HALVES;
    const int w6_lists = w6 == RLT_LSTM_X6W_SINGLE ? 16 : 32;
    LstmPlan p;
    p.fwd_lists = p.bwd_lists = LISTS;
    if (prec == RLT_PRECISION_BF16X6 && env.lstm6 && env.lstm6w && w6_fits) { p.fwd = w6; p.fwd_lists = w6_lists; }
    else if (prec == RLT_PRECISION_BF16X6 && env.lstm6) p.fwd = RLT_LSTM_X6;
    else if (prec == RLT_PRECISION_BF16X3) p.fwd = RLT_LSTM_X3;
    else p.fwd = RLT_LSTM_F32;
    // (the backward does not read RLT_LSTM6: with it off, bf16x6 still takes lstm6w.hip's backward)
    if (prec == RLT_PRECISION_BF16X6 && env.lstm6w && env.lstm6w_bwd && w6_fits) { p.bwd = w6; p.bwd_lists = w6_lists; }
    else if (prec == RLT_PRECISION_BF16X3) p.bwd = RLT_LSTM_X3;
    else p.bwd = RLT_LSTM_F32;
    return p;
}

extern "C" {

static int launch_bilstm_fwd(float* gates, const float* w_hh_fwd, const float* w_hh_rev, int S, int B,
                             float* h_out, float* c_out, const XIn& xi, void* stream) {
    const LstmPlan plan = lstm_plan(B);
    const dim3 grid(rlt_cdiv(B, plan.fwd_lists), 2), block(1024);
    hipStream_t st = rlt_stream(stream);
    if (plan.fwd == RLT_LSTM_X6W_SINGLE || plan.fwd == RLT_LSTM_X6W_HALVES) {
        const int rc = rlt_lstm6w_fwd(plan.fwd, plan.fwd_lists, gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi, stream);
        if (rc) return rc;
    } else if (plan.fwd == RLT_LSTM_X6) {
        auto go = [&](auto kern) {
            const int rc = rlt_allow_lds(kern, LSTM6_LDS);
            if (rc) return rc;
            hipLaunchKernelGGL(kern, grid, dim3(512), LSTM6_LDS, st, gates, (const float*)gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi);
            return 0;
        };
        const bool full = B % LISTS == 0;
        const int rc = xi.x ? (full ? go(bilstm6_fwd_kernel<true, true>) : go(bilstm6_fwd_kernel<true, false>))
                            : (full ? go(bilstm6_fwd_kernel<false, true>) : go(bilstm6_fwd_kernel<false, false>));
        if (rc) return rc;
    } else if (plan.fwd == RLT_LSTM_X3) {
        if (xi.x) hipLaunchKernelGGL(bilstm3_fwd_kernel<true>, grid, block, 0, st, gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi);
        else hipLaunchKernelGGL(bilstm3_fwd_kernel<false>, grid, block, 0, st, gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi);
    } else {
        if (xi.x) hipLaunchKernelGGL(bilstm_fwd_kernel<true>, grid, block, 0, st, gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi);
        else hipLaunchKernelGGL(bilstm_fwd_kernel<false>, grid, block, 0, st, gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi);
    }
    return RLT_LAUNCH_RESULT();
}

int rlt_bilstm_rec_plan(int B, int xin, int precision, struct rlt_bilstm_rec_plan* out) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(out && B > 0 && (xin == 0 || xin == 1));
    *out = lstm_plan(B);
    return 0;
}

int rlt_bilstm_rec_fwd(float* gates, const float* w_hh_fwd, const float* w_hh_rev, int S, int B,
                       float* h_out, float* c_out, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(gates && w_hh_fwd && w_hh_rev && h_out && c_out && S > 0 && B > 0);
    if (!(rlt_aligned16(gates) && rlt_aligned16(w_hh_fwd) && rlt_aligned16(w_hh_rev) && rlt_aligned16(h_out) && rlt_aligned16(c_out)))
        return RLT_E_ALIGN;
    XIn xi{};
    return launch_bilstm_fwd(gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi, stream);
}

int rlt_bilstm_rec_fwd_x(const float* x, int I, const float* w_ih_fwd, const float* b_ih_fwd, const float* b_hh_fwd,
                         const float* w_ih_rev, const float* b_ih_rev, const float* b_hh_rev,
                         const float* w_hh_fwd, const float* w_hh_rev, int S, int B,
                         float* gates, float* h_out, float* c_out, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(x && w_ih_fwd && b_ih_fwd && b_hh_fwd && w_ih_rev && b_ih_rev && b_hh_rev);
    RLT_CHECK_ARG(gates && w_hh_fwd && w_hh_rev && h_out && c_out && S > 0 && B > 0);
    RLT_CHECK_SHAPE(I >= 1 && I <= 3);
    if (!(rlt_aligned16(gates) && rlt_aligned16(w_hh_fwd) && rlt_aligned16(w_hh_rev) && rlt_aligned16(h_out) && rlt_aligned16(c_out)))
        return RLT_E_ALIGN;
    XIn xi{};
    xi.x = x; xi.I = I;
    xi.w_ih[0] = w_ih_fwd; xi.w_ih[1] = w_ih_rev;
    xi.b_ih[0] = b_ih_fwd; xi.b_ih[1] = b_ih_rev;
    xi.b_hh[0] = b_hh_fwd; xi.b_hh[1] = b_hh_rev;
    return launch_bilstm_fwd(gates, w_hh_fwd, w_hh_rev, S, B, h_out, c_out, xi, stream);
}

int rlt_bilstm_rec_bwd(float* gates, const float* c, const float* w_hh_fwd, const float* w_hh_rev,
                       const float* d_hout, int S, int B, int precision, void* stream) {
    RLT_PREC_SCOPE(precision);
    RLT_CHECK_ARG(gates && c && w_hh_fwd && w_hh_rev && d_hout && S > 0 && B > 0);
    if (!(rlt_aligned16(gates) && rlt_aligned16(c) && rlt_aligned16(w_hh_fwd) && rlt_aligned16(w_hh_rev) && rlt_aligned16(d_hout)))
        return RLT_E_ALIGN;
    const size_t shm = (size_t)16 * LISTS * LDP * sizeof(float);
    const size_t shm8 = (size_t)8 * LISTS * LDP8 * sizeof(float);
    int rc = rlt_allow_lds(bilstm_bwd_kernel, shm);
    if (!rc) rc = rlt_allow_lds(bilstm3_bwd8_kernel, shm8);
    if (rc) return rc;
    const LstmPlan plan = lstm_plan(B);
    const dim3 grid(rlt_cdiv(B, plan.bwd_lists), 2);
    if (plan.bwd == RLT_LSTM_X6W_SINGLE || plan.bwd == RLT_LSTM_X6W_HALVES) {
        rc = rlt_lstm6w_bwd(plan.bwd, plan.bwd_lists, gates, c, w_hh_fwd, w_hh_rev, d_hout, S, B, stream);
        if (rc) return rc;
    } else if (plan.bwd == RLT_LSTM_X3)
        hipLaunchKernelGGL(bilstm3_bwd8_kernel, grid, dim3(512), shm8, rlt_stream(stream), gates, c, w_hh_fwd, w_hh_rev, d_hout, S, B);
    else
        hipLaunchKernelGGL(bilstm_bwd_kernel, grid, dim3(1024), shm, rlt_stream(stream), gates, c, w_hh_fwd, w_hh_rev, d_hout, S, B);
    return RLT_LAUNCH_RESULT();
}

}  // extern "C"
