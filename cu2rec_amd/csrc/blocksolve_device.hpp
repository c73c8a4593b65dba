// What the phases of the block-solve mode share on the device (blocksolve.hip includes this and one header per phase:
// blocksolve_gram.hpp, blocksolve_solve.hpp, blocksolve_lookahead.hpp, blocksolve_update.hpp): the block and tile geometry, the
// decay tables' offsets, the native vector types and lane exchanges, and the rule that picks a chain's phase-2 form.  Everything
// is constexpr or __device__ __forceinline__.
#pragma once

#include <hip/hip_runtime.h>

#include "blocksolve.hpp"
#include "sgd_device.hpp"

namespace cu2rec {
namespace bs_dev {

using namespace dev;

constexpr int kB = kBsLinks;
constexpr int kTabAdel = 0, kTabCdel = kBsTableStride, kTabApow = 2 * kBsTableStride, kTabCpow = 3 * kBsTableStride;
constexpr int kH = 32;   // tile edge: a block is two halves of 32 links
constexpr int kMS = 36;  // LDS row stride (floats) of a 32x32 tile: 16-byte aligned rows, odd in float4 units

// native vectors: a float4 (a struct) is copied with memcpy, and an array of them written that way stayed in scratch;
// pairs of them feed v_pk_fma_f32 (two FMAs an issue slot) straight from the registers a 16-byte LDS read filled
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 lds4(const float4 *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ f32x2 lo2(f32x4 v) { return __builtin_shufflevector(v, v, 0, 1); }
__device__ __forceinline__ f32x2 hi2(f32x4 v) { return __builtin_shufflevector(v, v, 2, 3); }
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 dup2(float v) { return f32x2{v, v}; }
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned ld_agent(const unsigned *p) {  // global_load sc1: never served from this CU's L1
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// every device-side wait in here is bounded: BsIteration::wait_ticks (wait_ticks(): CU2REC_BS_WAIT_S seconds, default 2) of the 100 MHz wall clock

// v[l] + v[l ^ 16] in every lane
__device__ __forceinline__ float row_pair_sum(float v) {
    const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

// v[l & 31] + v[(l & 31) + 32] in every lane
__device__ __forceinline__ float half_sum(float v) {
    const u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---- which chains take the look-ahead form (phase 2, chain_lookahead) -------------------------------------------------------
// The longest chains ARE the iteration's critical path.  For popularity ranks below la_ranks phase 1 also builds, for every block
// but the chain's first, the block of lr L that couples it to the block before it (gram_cross_block), and phase 2 then needs the
// item row for nothing on its dependent path.  The chain's blocks must lie below la_cap (the cross blocks' buffer).
__device__ __forceinline__ bool chain_is_lookahead(const BsIteration &it, int chain, const BsChainDesc &cd) {
    const int nblk = (cd.len + kB - 1) / kB;
    return chain < it.la_ranks && nblk >= 2 && cd.blk0 + nblk <= it.la_cap;
}

}  // namespace bs_dev
}  // namespace cu2rec
