// The views derived from a rating matrix (csr_views.hpp) and the sort primitives they share with BPR's regrouping (rocprim_temp.hpp).
#include <hip/hip_runtime.h>

#include <cstring>  // (rocPRIM's headers call memset without including it)
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "csr_views.hpp"
#include "device.hpp"
#include "objective_pass.hpp"
#include "rocprim_temp.hpp"

namespace cu2rec {

namespace {

__global__ __launch_bounds__(kElementThreads) void iota_kernel(int *__restrict__ x, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) x[i] = i;
}

template <class T>
__global__ __launch_bounds__(kElementThreads) void gather_kernel(const T *__restrict__ src, const int *__restrict__ pos, int n,
                                                                 T *__restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = src[pos[i]];
}

__global__ __launch_bounds__(kElementThreads) void group_starts_kernel(const unsigned *__restrict__ keys, int n, int n_groups,
                                                                       int *__restrict__ starts) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k <= n_groups; k += gridDim.x * blockDim.x)
        starts[k] = first_at_least(keys, 0, n, static_cast<unsigned>(k));
}

__global__ __launch_bounds__(kElementThreads) void row_of_kernel(const int *__restrict__ indptr, int rows, int nnz, int *__restrict__ row_of) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += gridDim.x * blockDim.x) row_of[e] = row_of_entry(indptr, rows, e);
}

// one wavefront per row of the sorted columns: a column equal to the one before it is a repeated entry
__global__ __launch_bounds__(kElementThreads) void duplicate_kernel(const int *__restrict__ indptr, const int *__restrict__ idx, int rows,
                                                                    int *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
        const int lo = indptr[row], hi = indptr[row + 1];
        for (int e = lo + 1 + lane; e < hi; e += 64)
            if (idx[e] == idx[e - 1]) atomicOr(flag, 1);
    }
}

}  // namespace

void fill_iota(int *x, int n, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(iota_kernel, dim3(element_grid(n)), dim3(kElementThreads), 0, stream, x, n);
    CU2REC_HIP(hipGetLastError());
}

template <class T>
void gather(const T *src, const int *pos, int n, T *out, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(gather_kernel<T>, dim3(element_grid(n)), dim3(kElementThreads), 0, stream, src, pos, n, out);
    CU2REC_HIP(hipGetLastError());
}
template void gather<int>(const int *, const int *, int, int *, hipStream_t);
template void gather<float>(const float *, const int *, int, float *, hipStream_t);

void sort_pairs_into_groups(DeviceBuffer<unsigned char> &temp, const unsigned *keys_in, unsigned *keys_out, const int *vals_in,
                            int *vals_out, int n, unsigned bits, int n_groups, int *starts, hipStream_t stream) {
    if (n > 0)
        with_rocprim_temp(temp, [&](void *t, size_t &bytes) {
            return rocprim::radix_sort_pairs(t, bytes, keys_in, keys_out, vals_in, vals_out, static_cast<size_t>(n), 0u, bits, stream);
        });
    hipLaunchKernelGGL(group_starts_kernel, dim3(element_grid(static_cast<size_t>(n_groups) + 1)), dim3(kElementThreads), 0, stream, keys_out,
                       n, n_groups, starts);
    CU2REC_HIP(hipGetLastError());
}

const int *row_of_view(const DeviceCsr &m, hipStream_t stream) {
    CsrViews &v = m.views;
    if (v.row_of_built) return v.row_of.ptr;
    v.row_of.allocate(static_cast<size_t>(std::max(m.nnz, 1)));
    if (m.nnz > 0) {
        hipLaunchKernelGGL(row_of_kernel, dim3(element_grid(m.nnz)), dim3(kElementThreads), 0, stream, m.indptr.ptr, m.rows, m.nnz, v.row_of.ptr);
        CU2REC_HIP(hipGetLastError());
    }
    v.row_of_built = true;
    return v.row_of.ptr;
}

const ItemMajorView &item_major_view(const DeviceCsr &m, hipStream_t stream) {
    ItemMajorView &v = m.views.items;
    if (v.built) return v;
    const int *row_of = row_of_view(m, stream);
    const size_t n = static_cast<size_t>(std::max(m.nnz, 1));
    v.indptr.allocate(static_cast<size_t>(m.cols) + 1);
    v.indices.allocate(n);
    v.data.allocate(n);
    v.pos.allocate(n);
    DeviceBuffer<int> iota(n);
    DeviceBuffer<unsigned> cols_sorted(n);
    DeviceBuffer<unsigned char> temp;
    fill_iota(iota.ptr, m.nnz, stream);
    sort_pairs_into_groups(temp, reinterpret_cast<const unsigned *>(m.indices.ptr), cols_sorted.ptr, iota.ptr, v.pos.ptr, m.nnz,
                           key_bits(std::max(m.cols - 1, 1)), m.cols, v.indptr.ptr, stream);
    gather(row_of, v.pos.ptr, m.nnz, v.indices.ptr, stream);
    gather(m.data.ptr, v.pos.ptr, m.nnz, v.data.ptr, stream);
    CU2REC_HIP(hipStreamSynchronize(stream));  // before the temporaries are freed
    v.built = true;
    return v;
}

const RowSortedView &row_sorted_view(const DeviceCsr &m, bool with_values, hipStream_t stream) {
    RowSortedView &v = m.views.sorted;
    if (v.built && (v.has_values || !with_values)) return v;
    const size_t n = static_cast<size_t>(std::max(m.nnz, 1));
    const size_t n_values = with_values ? n : 0;
    DeviceBuffer<int> idx(n), pos(n_values), iota(n_values), flag(1);  // idx: v.idx again where an earlier caller built it without the values
    DeviceBuffer<float> val(n_values);
    DeviceBuffer<unsigned char> temp;
    int dup = v.has_duplicate;
    if (m.nnz > 0) {
        const unsigned bits = key_bits(std::max(m.cols - 1, 1)), nnz = static_cast<unsigned>(m.nnz), rows = static_cast<unsigned>(m.rows);
        const unsigned *keys = reinterpret_cast<const unsigned *>(m.indices.ptr);
        unsigned *keys_out = reinterpret_cast<unsigned *>(idx.ptr);
        const int *begin = m.indptr.ptr, *end = m.indptr.ptr + 1;
        if (with_values) {
            fill_iota(iota.ptr, m.nnz, stream);
            with_rocprim_temp(temp, [&](void *t, size_t &bytes) {
                return rocprim::segmented_radix_sort_pairs(t, bytes, keys, keys_out, iota.ptr, pos.ptr, nnz, rows, begin, end, 0u, bits, stream);
            });
            gather(m.data.ptr, pos.ptr, m.nnz, val.ptr, stream);
        } else {
            with_rocprim_temp(temp, [&](void *t, size_t &bytes) {
                return rocprim::segmented_radix_sort_keys(t, bytes, keys, keys_out, nnz, rows, begin, end, 0u, bits, stream);
            });
        }
        if (!v.built) {
            CU2REC_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), stream));
            hipLaunchKernelGGL(duplicate_kernel, dim3(element_grid(static_cast<size_t>(m.rows), 4)), dim3(kElementThreads), 0, stream, begin,
                               idx.ptr, m.rows, flag.ptr);
            CU2REC_HIP(hipGetLastError());
            CU2REC_HIP(hipMemcpyAsync(&dup, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        CU2REC_HIP(hipStreamSynchronize(stream));  // before the temporaries are freed
    }
    if (!v.built) v.idx.swap(idx);
    if (with_values) {
        v.pos.swap(pos);
        v.val.swap(val);
        v.has_values = true;
    }
    v.has_duplicate = dup != 0;
    v.built = true;
    return v;
}

}  // namespace cu2rec
