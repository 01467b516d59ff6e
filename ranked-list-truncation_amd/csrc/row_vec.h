// Row access of the per-list head kernels (heads.hip, hazard.hip): a row of E floats is read by one wavefront in chunks of
// 64 lanes x V floats, V = pick_v(E) floats (4, 8 or 16 bytes) per lane and load.
#pragma once
#include "common.h"

namespace {

template <int V> struct VecT;
template <> struct VecT<1> { typedef float T; };
template <> struct VecT<2> { typedef float2 T; };
template <> struct VecT<4> { typedef float4 T; };
template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&d)[V]) {
    typename VecT<V>::T v = *reinterpret_cast<const typename VecT<V>::T*>(p);
    const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
    for (int i = 0; i < V; ++i) d[i] = f[i];
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&d)[V]) {
    typename VecT<V>::T v;
    float* f = reinterpret_cast<float*>(&v);
#pragma unroll
    for (int i = 0; i < V; ++i) f[i] = d[i];
    *reinterpret_cast<typename VecT<V>::T*>(p) = v;
}

int pick_v(int E) { return (E % 256 == 0) ? 4 : ((E % 128 == 0) ? 2 : 1); }

}  // namespace
