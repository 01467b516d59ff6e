// The bf16 split arithmetic of the bf16x3 / bf16x6 modes, in ONE place: vector types, the cast-form pack and its unpacks, the exact
// two- and three-way splits, the MFMA sequences that consume them (32x32x16), the transposed LDS read, the four-lane column
// reductions - and the three-way split handed out in parts (split6_part, for kernels that fill the gaps behind their MFMAs themselves).
// Everything is __device__ __forceinline__ at namespace scope: it vanishes into the kernels of the file that includes it.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));

// two floats -> a packed bf16 pair (a in the low half).  The cast form: hipcc emits v_cvt_pk_bf16_f32 and inserts the wait states
// an MFMA needs behind a vector write of its operand
__device__ __forceinline__ uint32_t pk2(float a, float b) {
    typedef __bf16 v2 __attribute__((ext_vector_type(2)));
    const v2 t = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, t);
}
__device__ __forceinline__ float lo16(uint32_t p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float hi16(uint32_t p) { return __builtin_bit_cast(float, p & 0xffff0000u); }
__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ bf16x8 frag4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return as_frag(make_uint4(a, b, c, d)); }
__device__ __forceinline__ bf16x8 cat2(uint2 a, uint2 b) { return as_frag(make_uint4(a.x, a.y, b.x, b.y)); }

// KEEP_PACKED, the one real difference between the splits below: the packed pair is made opaque to the optimiser before it is
// unpacked - otherwise hipcc re-derives the low element's bf16 with a second v_cvt_pk (x, 0) instead of shifting the packed pair
// (one extra VALU instruction per two elements).  The kernels on v_mfma_f32_16x16x32_bf16 (attention6n.hip, attention6h.hip)
// split without it.  Which form a call site has is what it had when the copies were merged, not a measured choice: changing
// one is a change of code and wants a measurement.
template <bool KEEP_PACKED>
__device__ __forceinline__ void keep_packed(uint2& p) { if (KEEP_PACKED) asm("" : "+v"(p.x), "+v"(p.y)); }

// bf16x3: x = hi + lo, hi = bf16(x), lo = bf16(x - hi); four values -> two packed pairs each, eight -> one fragment each
__device__ __forceinline__ void split4(float a, float b, float c, float d, uint2& hi, uint2& lo) {
    hi.x = pk2(a, b);
    hi.y = pk2(c, d);
    keep_packed<true>(hi);
    lo.x = pk2(a - lo16(hi.x), b - hi16(hi.x));
    lo.y = pk2(c - lo16(hi.y), d - hi16(hi.y));
}
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
    uint2 h0, l0, h1, l1;
    split4(x[0], x[1], x[2], x[3], h0, l0);
    split4(x[4], x[5], x[6], x[7], h1, l1);
    hi = cat2(h0, h1);
    lo = cat2(l0, l1);
}
// a*b as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, smallest first
__device__ __forceinline__ f32x16 mfma3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
    return c;
}

// bf16x6: the EXACT three-way split x = h + m + l (h = bf16(x), m = bf16(x - h), l = x - h - m: 8 + 8 + 8 significand bits, the
// last residual is exactly representable; tests/test_split6.py restates it in numpy)
template <bool KEEP_PACKED>
__device__ __forceinline__ void split4x3(float a, float b, float c, float d, uint2& hi, uint2& mid, uint2& lo) {
    hi.x = pk2(a, b);
    hi.y = pk2(c, d);
    keep_packed<KEEP_PACKED>(hi);
    const float ra = a - lo16(hi.x), rb = b - hi16(hi.x), rc = c - lo16(hi.y), rd = d - hi16(hi.y);
    mid.x = pk2(ra, rb);
    mid.y = pk2(rc, rd);
    keep_packed<KEEP_PACKED>(mid);
    lo.x = pk2(ra - lo16(mid.x), rb - hi16(mid.x));
    lo.y = pk2(rc - lo16(mid.y), rd - hi16(mid.y));
}
template <bool KEEP_PACKED>
__device__ __forceinline__ void split8x3(const float (&x)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    uint2 h0, m0, l0, h1, m1, l1;
    split4x3<KEEP_PACKED>(x[0], x[1], x[2], x[3], h0, m0, l0);
    split4x3<KEEP_PACKED>(x[4], x[5], x[6], x[7], h1, m1, l1);
    h = cat2(h0, h1);
    m = cat2(m0, m1);
    l = cat2(l0, l1);
}
// attention6h.hip's form: no KEEP_PACKED, and one pair carried through all three planes at a time (hipcc schedules from the order
// of the statements, and the assembly of every kernel is held to what it was when the copies were merged)
__device__ __forceinline__ void split8x3_by_pair(const float (&x)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    uint32_t hh[4], mm[4], ll[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = x[2 * i], b = x[2 * i + 1];
        hh[i] = pk2(a, b);
        const float ra = a - lo16(hh[i]), rb = b - hi16(hh[i]);
        mm[i] = pk2(ra, rb);
        ll[i] = pk2(ra - lo16(mm[i]), rb - hi16(mm[i]));
    }
    h = frag4(hh[0], hh[1], hh[2], hh[3]);
    m = frag4(mm[0], mm[1], mm[2], mm[3]);
    l = frag4(ll[0], ll[1], ll[2], ll[3]);
}

// The six plane products of a bf16x6 product a*b, smallest first: product i takes plane x6_plane_a(i) of the A operand and plane
// x6_plane_b(i) of the B operand (0 = h, 1 = m, 2 = l).  The same order as PROD in tools/attn_pipe_sched.py, which the generated
// tile bodies are scheduled for.
__host__ __device__ __forceinline__ constexpr int x6_plane_a(int i) { return i == 0 ? 1 : i == 1 ? 2 : i == 2 ? 0 : i == 3 ? 1 : 0; }
__host__ __device__ __forceinline__ constexpr int x6_plane_b(int i) { return i == 0 ? 1 : i == 1 ? 0 : i == 2 ? 2 : i == 3 ? 0 : i == 4 ? 1 : 0; }
static_assert(x6_plane_a(0) == 1 && x6_plane_b(0) == 1 && x6_plane_a(1) == 2 && x6_plane_b(1) == 0 && x6_plane_a(2) == 0 && x6_plane_b(2) == 2 &&
              x6_plane_a(3) == 1 && x6_plane_b(3) == 0 && x6_plane_a(4) == 0 && x6_plane_b(4) == 1 && x6_plane_a(5) == 0 && x6_plane_b(5) == 0,
              "(m, m) (l, h) (h, l) (m, h) (h, m) (h, h)");
// ... on v_mfma_f32_32x32x16_bf16, written out in that order
__device__ __forceinline__ f32x16 mfma6(bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 bh, bf16x8 bm, bf16x8 bl, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
    return c;
}

// the three fragments of one operand, and the same two functions on them
struct Frag3 { bf16x8 h, m, l; };
template <bool KEEP_PACKED>
__device__ __forceinline__ Frag3 split8x3(const float (&x)[8]) {
    Frag3 f;
    split8x3<KEEP_PACKED>(x, f.h, f.m, f.l);
    return f;
}
__device__ __forceinline__ f32x16 mfma6(const Frag3& a, const Frag3& b, f32x16 c) { return mfma6(a.h, a.m, a.l, b.h, b.m, b.l, c); }

// ds_read_b64_tr_b16: per 16-lane group a 4-row x 16-column block of 16-bit elements, delivered column-major (lane i of the
// group gets column i of the 4 rows); every lane's address 8-byte aligned, EXEC all ones.  Two of them make one fragment.
__device__ __forceinline__ v4s tr_read(const uint16_t* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(p));
}
__device__ __forceinline__ bf16x8 cat_frag(v4s a, v4s b) {
    const v8s v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// max / sum over the four lanes (l & 15) + 16 {0, 1, 2, 3} that share a column of a 16x16x32 accumulator tile
__device__ __forceinline__ float col_max4(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float col_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// The split written one instruction per asm statement in LEVEL order (both conversions, the four unpacks, the four subtractions,
// ...), as six parts (4, 4, 4, 4, 4, 2 instructions) with its state, for kernels that hand the parts out one per MFMA gap: in
// that order no instruction sits next to the one it depends on, and the 22 instructions vanish in the shadows of six MFMAs of the
// same wavefront (tools/micro/mfma_split.hip: 200 cycles per step with and without; 304 as a block behind the MFMAs).  The wait
// state a v_cvt_pk_bf16_f32 needs before its result is used two instructions later is inserted by hipcc for these asm statements
// exactly as for its own code (`cvt; cvt; s_nop 0; use` in the ISA): no `s_nop` in the asm text.
struct Split6 { uint2 hi, mid, lo; uint32_t t0, t1, t2, t3; float r0, r1, r2, r3; };
__device__ __forceinline__ void split6_part(Split6& u, float a, float b, float c, float d, int part) {
    if (part == 0) {
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u.hi.x) : "v"(a), "v"(b));
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u.hi.y) : "v"(c), "v"(d));
        asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(u.t0) : "v"(u.hi.x));
        asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(u.t1) : "v"(u.hi.x));
    } else if (part == 1) {
        asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(u.t2) : "v"(u.hi.y));
        asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(u.t3) : "v"(u.hi.y));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r0) : "v"(a), "v"(u.t0));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r1) : "v"(b), "v"(u.t1));
    } else if (part == 2) {
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r2) : "v"(c), "v"(u.t2));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r3) : "v"(d), "v"(u.t3));
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u.mid.x) : "v"(u.r0), "v"(u.r1));
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u.mid.y) : "v"(u.r2), "v"(u.r3));
    } else if (part == 3) {
        asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(u.t0) : "v"(u.mid.x));
        asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(u.t1) : "v"(u.mid.x));
        asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(u.t2) : "v"(u.mid.y));
        asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(u.t3) : "v"(u.mid.y));
    } else if (part == 4) {
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r0) : "v"(u.r0), "v"(u.t0));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r1) : "v"(u.r1), "v"(u.t1));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r2) : "v"(u.r2), "v"(u.t2));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(u.r3) : "v"(u.r3), "v"(u.t3));
    } else {
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u.lo.x) : "v"(u.r0), "v"(u.r1));
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u.lo.y) : "v"(u.r2), "v"(u.r3));
    }
}
