// The selection code the fused top-k (topk.hip) and the item-neighbourhood product (knn.hip) share: the 64-bit keys whose unsigned
// order is recommend's order, and the wavefront bitonic sort that keeps the best of them.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace cu2rec {

// rocPRIM's float radix code (radix_key_codec, with the descending sort's -0.0 == +0.0) in the high word; the low word is
// (0x7FFFFFFF - item) << 1, so a larger key is a better (score, smaller item) pair, and bit 0 keeps the sign of a zero score
// so that the listed score is the computed float bit for bit.  Key 0 is never a candidate: it marks an empty slot.
__device__ __forceinline__ unsigned long long topk_key(float s, int item) {
    unsigned b = __float_as_uint(s);
    const unsigned negzero = b == 0x80000000u;
    if (negzero) b = 0u;
    const unsigned enc = b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
    return (static_cast<unsigned long long>(enc) << 32) | (static_cast<unsigned>(0x7FFFFFFF - item) << 1) | negzero;
}

__device__ __forceinline__ void topk_decode(unsigned long long key, int &item, float &score) {
    if (key == 0ull) {
        item = -1;
        score = __builtin_nanf("");
        return;
    }
    const unsigned enc = static_cast<unsigned>(key >> 32);
    const unsigned b = (key & 1ull) ? 0x80000000u : enc ^ ((enc & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu);
    item = 0x7FFFFFFF - static_cast<int>((static_cast<unsigned>(key) >> 1) & 0x7FFFFFFFu);
    score = __uint_as_float(b);
}

// Bitonic sort, descending, of the wavefront's 64 E keys; element e of lane l is key e * 64 + l.  Strides below 64 pair lanes
// (shuffles), larger ones pair registers of one lane.  Every index is a compile-time constant after unrolling.
template <int E>
__device__ __forceinline__ void wave_sort_desc(unsigned long long (&v)[E], int lane) {
#pragma unroll
    for (int size = 2; size <= 64 * E; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= 64) {
                const int es = stride >> 6;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if (e & es) continue;
                    const bool desc = ((e * 64 + lane) & size) == 0;  // this block ends up descending: the lower slot takes the max
                    const unsigned long long a = v[e], b = v[e | es];
                    const bool swap = desc ? a < b : a > b;
                    v[e] = swap ? b : a;
                    v[e | es] = swap ? a : b;
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const unsigned long long o = __shfl_xor(v[e], stride);
                    const bool lower = (lane & stride) == 0, desc = ((e * 64 + lane) & size) == 0;
                    v[e] = lower == desc ? max(v[e], o) : min(v[e], o);
                }
            }
        }
    }
}

// loads the count keys of a candidate buffer (the rest as empty), sorts them best first
template <int E>
__device__ __forceinline__ void load_sorted(unsigned long long (&v)[E], const unsigned long long *buf, int count, int lane) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = e * 64 + lane < count ? buf[e * 64 + lane] : 0ull;
    wave_sort_desc<E>(v, lane);
}

}  // namespace cu2rec
