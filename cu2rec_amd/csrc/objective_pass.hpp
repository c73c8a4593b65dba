// The double-precision objective passes (als.hip: ials_objective_kernel; lmf.hip: lmf_objective_kernel; bpr.hip:
// bpr_objective_kernel): a 16-lane group per entry or row, per-thread sums in double, one tree reduction per workgroup.  Every sum's
// order is a function of the grid alone.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "hip_check.hpp"

namespace cu2rec {

constexpr int kObjThreads = 256, kObjGroup = 16, kObjMaxBlocks = 4096;

// workgroups of an objective pass over `work` entries or rows: eight per group, kObjMaxBlocks at most (the groups stride beyond that)
inline int objective_blocks(size_t work) {
    const int per_block = (kObjThreads / kObjGroup) * 8;
    return static_cast<int>(std::min<size_t>(std::max<size_t>((work + per_block - 1) / per_block, 1), kObjMaxBlocks));
}

// x . y over the first f floats of two rows, in double, by one 16-lane group; every lane returns the sum
__device__ inline double group_dot(const float *x, const float *y, int f, int lane16) {
    double d = 0.0;
    for (int c0 = 4 * lane16; c0 < f; c0 += 4 * kObjGroup) {
        const float4 a = *reinterpret_cast<const float4 *>(x + c0), b = *reinterpret_cast<const float4 *>(y + c0);
        d += static_cast<double>(a.x) * static_cast<double>(b.x);
        if (c0 + 1 < f) d += static_cast<double>(a.y) * static_cast<double>(b.y);
        if (c0 + 2 < f) d += static_cast<double>(a.z) * static_cast<double>(b.z);
        if (c0 + 3 < f) d += static_cast<double>(a.w) * static_cast<double>(b.w);
    }
    for (int m = kObjGroup / 2; m > 0; m >>= 1) d += __shfl_xor(d, m, kObjGroup);
    return d;
}

// the row of CSR entry k: the last u with indptr[u] <= k
__device__ inline int row_of_entry(const int *indptr, int rows, int k) {
    int lo = 0, hi = rows;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (indptr[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the first position in sorted[lo, hi) (ascending) that holds key or more; hi where none does
template <class T>
__device__ inline int first_at_least(const T *sorted, int lo, int hi, T key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the workgroup's N sums, a fixed tree over its kObjThreads threads: red[j][0] holds sum j, for thread 0 to read
template <int N>
__device__ inline void block_reduce(const double (&s)[N], double (&red)[N][kObjThreads]) {
    const int tid = threadIdx.x;
    for (int j = 0; j < N; ++j) red[j][tid] = s[j];
    for (int stride = kObjThreads / 2; stride > 0; stride >>= 1) {
        __syncthreads();
        if (tid < stride)
            for (int j = 0; j < N; ++j) red[j][tid] += red[j][tid + stride];
    }
}

// partials[block][N], as thread 0 of every workgroup left them, added on the host in block order (synchronises)
template <int N>
void sum_block_partials(DeviceBuffer<double> &partials, int blocks, double (&out)[N], hipStream_t stream) {
    std::vector<double> part(N * static_cast<size_t>(blocks));
    CU2REC_HIP(hipMemcpyAsync(part.data(), partials.ptr, part.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    for (int j = 0; j < N; ++j) out[j] = 0.0;
    for (int b = 0; b < blocks; ++b)
        for (int j = 0; j < N; ++j) out[j] += part[N * b + j];
}

}  // namespace cu2rec
