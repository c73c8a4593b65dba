// SLIM (include/cu2rec_amd.h: cu2rec_slim_create): for every item j the weights w = W[:, j] that minimise
//   1/2 w^T A w - sum_{k != j} A_kj w_k + l1 |w|_1,   w_j = 0 (and w >= 0 when `positive`),   A = X^T X + l2 I (ease_gram),
// by cyclic coordinate descent over the coordinates k = 0 .. ld - 1 in ascending order, each coordinate for all columns j at once.
// Three ld x ld float matrices: A, the residual C = A - A W (C = A at the start, since W = 0) and W.  One step of coordinate k:
//   rho = C[k, j] + A_kk W[k, j];  new = soft threshold of rho by l1, over A_kk (0 for k = j);  delta = new - W[k, j];
//   W[k, j] = new;  C[:, j] -= delta A[:, k].
// The coordinates are taken kEaseBlock = 64 at a time -- the same sequence of values as one by one, in two launches per block K:
//
//   slim_sweep_kernel   one wavefront per tile J of 64 columns, a lane per column: A[K, K] in LDS (every read a broadcast), the lane's
//                       64 entries of C[K, j] and of W[K, j] in registers; the 64 steps in order, each delta applied to the LATER
//                       coordinates of the lane's own copy of C[K, j] only.  Writes W[K, J], the tile Delta[K, J], a flag per tile
//                       (any delta != 0) and the tile's largest |delta| into the sweep's maximum.
//   slim_update_kernel  one workgroup per tile (I, J) of C, K's own row tile included: C[I, J] -= A[I, K] Delta[K, J], one tile
//                       product on v_mfma_f32_32x32x2_f32 from zero, subtracted with one rounding per element (ease_tile.hpp).  A
//                       workgroup whose tile of Delta is all zeros returns at once: what it would subtract is an exact zero.
//
// Every sum is an fmaf or MFMA chain in an order fixed by the indices alone.  The one atomic is an integer maximum of the bit patterns
// of non-negative floats, which is exact in any order.  Rows and columns of unstored items and of the padding have zero rho throughout
// and stay zero with no special case.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "csr_views.hpp"
#include "device.hpp"
#include "ease_tile.hpp"
#include "hip_check.hpp"
#include "rocprim_temp.hpp"
#include "slim.hpp"

namespace cu2rec {

namespace {

struct SlimBlock {
    const float *A, *C;
    float *W, *delta;     // delta: [kNb][ld], the block's row panel
    int *flags;           // [ld / kNb]: tile J of delta has a nonzero
    unsigned *max_delta;  // the bit pattern of the sweep's largest |delta| so far (a NaN's is above every number's)
    int ld, kb;
    float l1;
};

// workgroup J (one wavefront): the coordinates kb * kNb .. + kNb - 1 of the columns J * kNb .. + kNb - 1
template <bool POSITIVE>
__global__ __launch_bounds__(64) void slim_sweep_kernel(SlimBlock a) {
    __shared__ float akk[kNb][kLs];
    const int lane = threadIdx.x;
    const int k0 = a.kb * kNb, j = blockIdx.x * kNb + lane;
    const size_t at = static_cast<size_t>(k0) * a.ld + j;  // (k0, j); row k0 + t is t * ld further
    load_tile(akk, a.A + static_cast<size_t>(k0) * a.ld + k0, a.ld, 64);
    float c[kNb], w[kNb];
#pragma unroll
    for (int t = 0; t < kNb; ++t) {
        c[t] = a.C[at + static_cast<size_t>(t) * a.ld];
        w[t] = a.W[at + static_cast<size_t>(t) * a.ld];
    }
    __syncthreads();
    unsigned top = 0u;
#pragma unroll
    for (int t = 0; t < kNb; ++t) {
        const float diag = akk[t][t];
        const float rho = fmaf(diag, w[t], c[t]);
        float nw = POSITIVE ? fmaxf(rho - a.l1, 0.f) / diag : copysignf(fmaxf(fabsf(rho) - a.l1, 0.f) / diag, rho);
        if (k0 + t == j) nw = 0.f;
        const float d = nw - w[t];
        a.W[at + static_cast<size_t>(t) * a.ld] = nw;
        a.delta[static_cast<size_t>(t) * a.ld + j] = d;
        top = max(top, __float_as_uint(fabsf(d)));
#pragma unroll
        for (int s = t + 1; s < kNb; ++s) c[s] = fmaf(-d, akk[s][t], c[s]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) top = max(top, static_cast<unsigned>(__shfl_xor(static_cast<int>(top), off)));
    if (lane == 0) {
        a.flags[blockIdx.x] = top != 0u;
        if (top != 0u) atomicMax(a.max_delta, top);
    }
}

// workgroup (J, I): C[I, J] -= A[I, kb] Delta[kb, J]
__global__ __launch_bounds__(256) void slim_update_kernel(const float *__restrict__ A, float *__restrict__ C, const float *__restrict__ delta,
                                                          const int *__restrict__ flags, int ld, int kb) {
    __shared__ float x[kNb][kLs], y[kNb][kLs];
    const int bj = blockIdx.x, bi = blockIdx.y;
    if (!flags[bj]) return;  // the workgroup's branch
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wi = wave >> 1, wj = wave & 1;
    load_tile(x, A + static_cast<size_t>(bi) * kNb * ld + static_cast<size_t>(kb) * kNb, ld, 256);
    load_tile(y, delta + static_cast<size_t>(bj) * kNb, ld, 256);
    __syncthreads();
    f32x16 part = zero_tile();
    tile_mma<false, false, false>(part, x, y, wi, wj, lane);
    float *c = tile_at(C, ld, bi, bj);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        float *at = c + static_cast<size_t>(wi * 32 + acc_row(reg, lane >> 5)) * ld + wj * 32 + (lane & 31);
        *at = *at - part[reg];
    }
}

// count[0] += the nonzeros of w[0 .. total)
__global__ __launch_bounds__(256) void slim_count_kernel(const float *__restrict__ w, size_t total, unsigned long long *__restrict__ count) {
    unsigned long long mine = 0;
    for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += static_cast<size_t>(gridDim.x) * blockDim.x)
        mine += w[t] != 0.f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);  // an integer sum: exact in any order
}

}  // namespace

void slim_check(const SlimParams &p) {
    const Need need{"cu2rec_slim_create"};
    need(std::isfinite(p.l1) && p.l1 >= 0.f, CU2REC_EINVAL, ": l1 must be finite and >= 0");
    ease_check_l2("cu2rec_slim_create", p.l2);
    need(p.max_sweeps >= 1, CU2REC_EINVAL, ": max_sweeps must be >= 1");
    need(p.tol >= 0.f, CU2REC_EINVAL, ": tol must be >= 0 and not NaN");
}

DeviceEase::DeviceEase(const DeviceCsr &train, const SlimParams &p, cu2rec_slim_report *report)
    : items(train.cols), ld(ease_padded(train.cols)), l2(p.l2) {
    slim_check(p);
    if (items > kEaseMaxItems) fail(CU2REC_EUNSUPPORTED, "cu2rec_slim_create: more than CU2REC_EASE_MAX_ITEMS columns");
    if (report) *report = cu2rec_slim_report{0, 0.f, 0};
    if (items == 0) return;
    require_device();
    check_faults();
    hipStream_t stream = nullptr;
    if (row_sorted_view(train, true, stream).has_duplicate) fail(CU2REC_EINVAL, "cu2rec_slim_create: a row stores the same column twice");
    const int T = ld / kNb;
    const size_t order2 = static_cast<size_t>(ld) * ld;
    DeviceBuffer<float> A, C, delta(static_cast<size_t>(kNb) * ld);
    ease_allocate_matrix(A, order2, "cu2rec_slim_create");
    ease_allocate_matrix(C, order2, "cu2rec_slim_create");
    ease_allocate_matrix(B, order2, "cu2rec_slim_create");
    DeviceBuffer<int> flags(T);
    DeviceBuffer<unsigned> max_delta(1);
    DeviceBuffer<unsigned long long> count(1);
    ease_gram(train, l2, ld, A.ptr, stream);
    CU2REC_HIP(hipMemcpyAsync(C.ptr, A.ptr, order2 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    CU2REC_HIP(hipMemsetAsync(B.ptr, 0, order2 * sizeof(float), stream));
    int sweeps = 0;
    float last = 0.f;
    while (sweeps < p.max_sweeps) {
        CU2REC_HIP(hipMemsetAsync(max_delta.ptr, 0, sizeof(unsigned), stream));
        for (int kb = 0; kb < T; ++kb) {
            const SlimBlock a{A.ptr, C.ptr, B.ptr, delta.ptr, flags.ptr, max_delta.ptr, ld, kb, p.l1};
            if (p.positive) hipLaunchKernelGGL(slim_sweep_kernel<true>, dim3(T), dim3(64), 0, stream, a);
            else hipLaunchKernelGGL(slim_sweep_kernel<false>, dim3(T), dim3(64), 0, stream, a);
            hipLaunchKernelGGL(slim_update_kernel, dim3(T, T), dim3(256), 0, stream, A.ptr, C.ptr, delta.ptr, flags.ptr, ld, kb);
        }
        CU2REC_HIP(hipGetLastError());
        CU2REC_HIP(hipMemcpyAsync(&last, max_delta.ptr, sizeof(float), hipMemcpyDeviceToHost, stream));  // the float whose bits were kept
        CU2REC_HIP(hipStreamSynchronize(stream));
        ++sweeps;
        if (!std::isfinite(last))
            fail(CU2REC_EUNSUPPORTED, "cu2rec_slim_create: a weight of sweep " + std::to_string(sweeps) + " is not a finite number (a NaN or an infinite value in the data)");
        if (p.tol > 0.f && last <= p.tol) break;  // tol = 0: every sweep is run
    }
    unsigned long long nonzeros = 0;
    CU2REC_HIP(hipMemsetAsync(count.ptr, 0, sizeof(nonzeros), stream));
    hipLaunchKernelGGL(slim_count_kernel, dim3(element_grid(order2)), dim3(256), 0, stream, B.ptr, order2, count.ptr);
    CU2REC_HIP(hipGetLastError());
    CU2REC_HIP(hipMemcpyAsync(&nonzeros, count.ptr, sizeof(nonzeros), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));  // also before A, C and the panel are freed
    if (report) *report = cu2rec_slim_report{sweeps, last, static_cast<long long>(nonzeros)};
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_slim_create(const cu2rec_csr *train, float l1, float l2, int positive, int max_sweeps, float tol, cu2rec_slim_report *report,
                       cu2rec_ease **out) {
    return guarded([&] {
        require(out, "cu2rec_slim_create: null argument");
        *out = nullptr;
        const SlimParams p{l1, l2, positive != 0, max_sweeps, tol};
        slim_check(p);
        require(train, "cu2rec_slim_create: null argument");
        *out = new cu2rec_ease(unwrap(train), p, report);
    });
}

}  // extern "C"
