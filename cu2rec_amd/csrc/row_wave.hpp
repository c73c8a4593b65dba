// One wavefront per row: what the conjugate-gradient half-steps (als_cg.hip), the logistic trainer's sparse pass (lmf.hip) and the
// pairwise-ranking trainer's gradient kernels (bpr.hip) share.
//
// Two lane <-> element maps of a row of up to 64 E floats.  OWNER: lane l holds elements l, l + 64, ... (E registers).  ENTRY: the
// wavefront is four groups of 16 lanes, group g takes the row's entries e = g, g + 4, ... in ascending order, lane l16 of a group
// holds columns 4 l16 + 64 k .. + 3 of the gathered partner row (E float4).  A group's dot product is reduced by a butterfly over
// its 16 lanes, its sums are accumulated per group, and the four groups' partial sums go through LDS and are added in group order:
// the order of every sum is a function of the row's length and f alone.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

namespace cu2rec {

// the launch shape of the one-wavefront-per-row kernels of lmf.hip and bpr.hip: four rows per workgroup, the grid strides beyond
// kRowMaxBlocks workgroups
constexpr int kRowThreads = 256, kRowWaves = kRowThreads / 64, kRowMaxBlocks = 8192;
inline int row_grid(int rows) { return std::min((rows + kRowWaves - 1) / kRowWaves, kRowMaxBlocks); }

// the wavefront's LDS traffic is its own: order it for the compiler and the memory model, no instruction is needed beyond that
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// sum over the wavefront, the same bits in every lane (a butterfly: both partners add the same two values)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// partner row `idx` of X (row stride ldx), columns c0 .. c0 + 3, zero from column F on: the padding floats are never read as data.
// ONE: column F is the constant 1 of [x | 1], synthesised here (never loaded, also where column F starts a float4 of its own)
template <bool ONE>
__device__ __forceinline__ float4 load_partner4(const float *X, int ldx, int F, int idx, int c0) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < F) {
        v = *reinterpret_cast<const float4 *>(X + static_cast<size_t>(idx) * ldx + c0);
        if (c0 + 1 >= F) v.y = 0.f;
        if (c0 + 2 >= F) v.z = 0.f;
        if (c0 + 3 >= F) v.w = 0.f;
    }
    if constexpr (ONE) {
        if (c0 == F) v.x = 1.f;
        if (c0 + 1 == F) v.y = 1.f;
        if (c0 + 2 == F) v.z = 1.f;
        if (c0 + 3 == F) v.w = 1.f;
    }
    return v;
}

// ENTRY map: q . v over the group's 16 lanes, columns ascending within a lane; every lane of the group returns the sum
template <int E>
__device__ __forceinline__ float group_dot4(const float4 (&q)[E], const float4 (&v)[E]) {
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        d = fmaf(q[k].x, v[k].x, d);
        d = fmaf(q[k].y, v[k].y, d);
        d = fmaf(q[k].z, v[k].z, d);
        d = fmaf(q[k].w, v[k].w, d);
    }
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) d = d + __shfl_xor(d, m, 16);
    return d;
}

// ENTRY map: acc += s q, one float4 of the lane's E
__device__ __forceinline__ void axpy4(float s, const float4 &q, float4 &acc) {
    acc.x = fmaf(s, q.x, acc.x);
    acc.y = fmaf(s, q.y, acc.y);
    acc.z = fmaf(s, q.z, acc.z);
    acc.w = fmaf(s, q.w, acc.w);
}

// the four groups' sums (ENTRY map) through part, the wavefront's [4][64 E] floats, added in group order into the OWNER map.
// mine: this lane's first float4 in its group's [64 E], part + g 64 E + 4 l16 -- formed by the caller, next to its other uses of g
// and l16: formed here, the address arithmetic of every kernel that inlines this comes out differently.  The caller has ordered
// part's earlier reads before this (wave_sync)
template <int E>
__device__ __forceinline__ void combine_groups(const float4 (&acc)[E], float *part, float *mine, int lane, float (&out)[E]) {
    constexpr int FS = 64 * E;
#pragma unroll
    for (int k = 0; k < E; ++k) *reinterpret_cast<float4 *>(mine + 64 * k) = acc[k];
    wave_sync();
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = lane + 64 * k;
        out[k] = ((part[i] + part[FS + i]) + part[2 * FS + i]) + part[3 * FS + i];
    }
}

// f(std::integral_constant<int, E>{}) for the E = 1 .. 4 elements per lane of a row of `order` floats (order <= 256, checked by the
// caller: 252 factors and the bias)
template <class F>
auto dispatch_1_to_4(int order, F &&f) -> decltype(f(std::integral_constant<int, 1>{})) {
    switch ((order + 63) / 64) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

}  // namespace cu2rec
