// The sort primitives of the rating-matrix views (csr_views.hip) and of BPR's per-sweep regrouping (bpr.hip), one copy of each:
// rocPRIM's two-call form, the radix sorts' key width, the element-wise kernels around a sort and their launch grid.
#pragma once

#include <algorithm>
#include <cstddef>

#include "hip_check.hpp"

namespace cu2rec {

// call(temp, bytes): the rocPRIM call with all but its first two arguments bound -- a call with a null temporary only reports the
// bytes it needs, the same call with that many does the work.  temp grows to what the call asks for and 16 bytes of slack, and never
// shrinks: a cached buffer or a fresh local one, as the caller has it
template <class Call>
void with_rocprim_temp(DeviceBuffer<unsigned char> &temp, Call &&call) {
    size_t bytes = 0;
    CU2REC_HIP(call(nullptr, bytes));
    if (temp.count < bytes + 16) temp.allocate(bytes + 16);
    CU2REC_HIP(call(temp.ptr, bytes));
}

inline unsigned key_bits(int top) {  // bits that hold every key in [0, top]
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) <= static_cast<unsigned long long>(top)) ++bits;
    return bits;
}

// workgroups of a grid-stride kernel over n elements, per_block to a workgroup of kElementThreads: one at least, 8192 at most
constexpr int kElementThreads = 256;
inline int element_grid(size_t n, int per_block = kElementThreads) {
    return static_cast<int>(std::max<size_t>(1, std::min<size_t>((n + per_block - 1) / per_block, 8192)));
}

// csr_views.hip.  x[i] = i;  out[i] = src[pos[i]];  n == 0 launches nothing
void fill_iota(int *x, int n, hipStream_t stream);
template <class T>  // int and float
void gather(const T *src, const int *pos, int n, T *out, hipStream_t stream);
// (keys_in, vals_in) by ascending key into (keys_out, vals_out) -- a stable LSD radix sort over the keys' low `bits` bits: equal
// keys keep the order they came in -- and then starts[k] = the first position of keys_out that holds k or more, k = 0 .. n_groups
// (n == 0: zeros)
void sort_pairs_into_groups(DeviceBuffer<unsigned char> &temp, const unsigned *keys_in, unsigned *keys_out, const int *vals_in,
                            int *vals_out, int n, unsigned bits, int n_groups, int *starts, hipStream_t stream);

}  // namespace cu2rec
