// Alternating least squares half-step (als.hpp, include/cu2rec_amd.h: cu2rec_model_als).
//
// For a row with n ratings the partner rows are staged kAlsStep at a time into LDS as the augmented matrix
// Z = [x_i | 1 | t_i] (f + 2 columns, zero-filled to C = 32 NT; the 1 column is synthesised here, the model's padding floats
// are never read as data), and the lower triangle of Z^T Z is accumulated on the matrix cores: v_mfma_f32_32x32x2_f32 (exact
// f32, a k-ordered fmaf chain) with the ratings as the K dimension, one 32 x 32 tile pair (ti >= tj) per accumulator, the
// NT (NT + 1) / 2 tile pairs spread over the workgroup's eight wavefronts.  Its last row holds Z^T t, the right-hand side.
//
// The accumulators are written into LDS as a packed lower triangle of order f + 2, the regulariser n * reg goes onto the
// diagonal, and a right-looking Cholesky factorisation runs over the first f + 1 pivots: the rank-1 updates carry the
// appended row along, so it ends as L^-1 b (the forward substitution comes for free).  A back substitution gives the row's
// [factors; bias].  A pivot that is not a finite positive float, or a solution that is not finite, leaves the row unchanged and
// counts it (integer atomic).  Everything a row's result depends on -- staging, accumulation order, the chunk cut of a long row
// and the order its partial Grams are summed in, the factorisation -- is a function of the row's own length: no float atomics,
// nothing that depends on the batch or the other rows.
#include <hip/hip_runtime.h>

#include <cstring>  // (rocPRIM's headers call memset without including it)
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "als.hpp"
#include "kernels.hpp"
#include "score_tile.hpp"

namespace cu2rec {

namespace {

constexpr int kAlsThreads = 512;
constexpr int kAlsWaves = kAlsThreads / 64;

struct AlsArgs {
    const int *indptr, *indices;
    const float *data;
    AlsProblem p;
    const int *long_rows, *long_first_chunk, *chunk_lo, *chunk_hi;
    int chunk0, row0;  // first chunk / first long row of the batch
    float *ws;         // the batch's partial Grams: [chunk][pair][16][64]
    int *unsolved;
};

template <int NT>
struct AlsShape {
    static constexpr int C = 32 * NT;  // staged columns
    static constexpr int pairs = NT * (NT + 1) / 2;
    static constexpr int per_wave = (pairs + kAlsWaves - 1) / kAlsWaves;
};

__host__ __device__ inline int tri(int i) { return i * (i + 1) / 2; }

__device__ inline void pair_tiles(int p, int &ti, int &tj) {  // pair p of the row-major lower triangle of tiles
    ti = 0;
    while (tri(ti + 1) <= p) ++ti;
    tj = p - tri(ti);
}

__host__ __device__ inline size_t solve_lds_floats(int f) {  // packed augmented triangle + three vectors of order f + 2 + a flag
    return static_cast<size_t>(tri(f + 2)) + 3 * static_cast<size_t>(f + 4) + 4;
}

// acc += the augmented Gram of ratings [lo, hi) of the current row, kAlsStep ratings per LDS stage
template <int NT>
__device__ void als_accumulate(const AlsArgs &a, int lo, int hi, f32x16 (&acc)[AlsShape<NT>::per_wave], float *zs) {
    constexpr int C = AlsShape<NT>::C, S4 = C / 4, pairs = AlsShape<NT>::pairs;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int F = a.p.n_factors;
    float4 *zs4 = reinterpret_cast<float4 *>(zs);
    for (int k0 = lo; k0 < hi; k0 += kAlsStep) {
        __syncthreads();  // the previous stage's operands have been read
        for (int e = tid; e < kAlsStep * S4; e += kAlsThreads) {
            const int row = e / S4, s = e - row * S4, k = k0 + row, c0 = 4 * s;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < hi) {
                const int idx = a.indices[k];
                if (c0 < F) v = *reinterpret_cast<const float4 *>(a.p.X + static_cast<size_t>(idx) * a.p.ldx + c0);
                if (c0 + 3 >= F) {  // columns F (the constant 1), F + 1 (t) and zero fill
                    float t = 0.f;
                    if (c0 <= F + 1 && F + 1 <= c0 + 3) t = (a.data[k] - a.p.global_bias) - a.p.xb[idx];
                    auto fix = [&](float &x, int c) {
                        if (c >= F) x = c == F ? 1.f : (c == F + 1 ? t : 0.f);
                    };
                    fix(v.x, c0);
                    fix(v.y, c0 + 1);
                    fix(v.z, c0 + 2);
                    fix(v.w, c0 + 3);
                }
            }
            zs4[row * S4 + s] = v;
        }
        __syncthreads();
        // A[i][k] = Z[k][32 ti + i], B[k][j] = Z[k][32 tj + j]: lane (r, h) feeds row 2 kk + h of the stage
#pragma unroll
        for (int s = 0; s < AlsShape<NT>::per_wave; ++s) {
            const int p = wave + kAlsWaves * s;
            if (p < pairs) {
                int ti, tj;
                pair_tiles(p, ti, tj);
                const float *za = zs + h * C + 32 * ti + r, *zb = zs + h * C + 32 * tj + r;
#pragma unroll
                for (int kk = 0; kk < kAlsStep / 2; ++kk)
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[2 * kk * C], zb[2 * kk * C], acc[s], 0, 0, 0);
            }
        }
    }
}

// the accumulated augmented Gram of `row` (n ratings) -> Cholesky in LDS -> the row's factors and bias, or counted as unsolved
template <int NT>
__device__ void als_solve(const AlsArgs &a, int row, int n, f32x16 (&acc)[AlsShape<NT>::per_wave], float *lds) {
    constexpr int pairs = AlsShape<NT>::pairs;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int F = a.p.n_factors, D = F + 1;  // system order D; row D of the augmented triangle is the right-hand side
    float *G = lds, *col = G + tri(D + 1), *x = col + (D + 3), *xo = x + (D + 3);
    int *bad = reinterpret_cast<int *>(xo + (D + 3));  // (no __syncthreads_or: its static LDS would cap the dynamic LDS below 160 KiB)
    __syncthreads();  // G overlays the staging area
    const float nf = static_cast<float>(n);
#pragma unroll
    for (int s = 0; s < AlsShape<NT>::per_wave; ++s) {
        const int p = wave + kAlsWaves * s;
        if (p < pairs) {
            int ti, tj;
            pair_tiles(p, ti, tj);
            const int j = 32 * tj + r;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = 32 * ti + acc_row(reg, h);
                if (j <= i && i <= D) {
                    float v = acc[s][reg];
                    if (i == j && i < D) v = v + nf * (i < F ? a.p.reg : a.p.reg_bias);
                    G[tri(i) + j] = v;
                }
            }
        }
    }
    bool ok = true;
    for (int k = 0; k < D; ++k) {
        __syncthreads();
        const float d = G[tri(k) + k];  // the same value in every thread: the exit is uniform
        if (!(d > 0.f && d <= 3.402823466e38f)) {
            ok = false;
            break;
        }
        const float l = sqrtf(d);
        for (int i = k + 1 + tid; i <= D; i += kAlsThreads) {
            const float v = G[tri(i) + k] / l;
            G[tri(i) + k] = v;
            col[i] = v;
        }
        __syncthreads();
        if (tid == 0) G[tri(k) + k] = l;  // after the barrier: every wave has read the pivot by now
        for (int i = k + 1 + wave; i <= D; i += kAlsWaves) {  // trailing update; row D only up to column D - 1
            const float ci = col[i];
            const int jmax = min(i, D - 1);
            float *gi = G + tri(i);
            for (int j = k + 1 + lane; j <= jmax; j += 64) gi[j] = gi[j] - ci * col[j];
        }
    }
    if (!ok) {
        if (tid == 0) atomicAdd(a.unsolved, 1);
        return;
    }
    __syncthreads();
    if (tid == 0) *bad = 0;
    for (int i = tid; i < D; i += kAlsThreads) x[i] = G[tri(D) + i];  // y = L^-1 b
    for (int k = D - 1; k >= 0; --k) {                                 // L^T x = y, column by column
        __syncthreads();
        const float xk = x[k] / G[tri(k) + k];
        const float *lk = G + tri(k);
        for (int i = tid; i < k; i += kAlsThreads) x[i] = x[i] - lk[i] * xk;
        if (tid == 0) xo[k] = xk;
    }
    __syncthreads();
    for (int i = tid; i < D; i += kAlsThreads)
        if (!isfinite(xo[i])) *bad = 1;
    __syncthreads();
    if (*bad) {
        if (tid == 0) atomicAdd(a.unsolved, 1);
        return;
    }
    float *y = a.p.Y + static_cast<size_t>(row) * a.p.ldy;
    for (int c = tid; c < a.p.ldy; c += kAlsThreads) y[c] = c < F ? xo[c] : 0.f;
    if (tid == 0) a.p.yb[row] = xo[F];
}

template <int NT>
__device__ inline void zero_acc(f32x16 (&acc)[AlsShape<NT>::per_wave]) {
#pragma unroll
    for (int s = 0; s < AlsShape<NT>::per_wave; ++s)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
}

// rows of 1 .. kAlsChunk ratings: one workgroup each, gather, Gram and solve
template <int NT>
__global__ __launch_bounds__(kAlsThreads) void als_short_kernel(AlsArgs a) {
    extern __shared__ float4 als_smem[];
    float *lds = reinterpret_cast<float *>(als_smem);
    const int row = blockIdx.x;
    const int lo = a.indptr[row], hi = a.indptr[row + 1];
    if (hi <= lo || hi - lo > kAlsChunk) return;
    f32x16 acc[AlsShape<NT>::per_wave];
    zero_acc<NT>(acc);
    als_accumulate<NT>(a, lo, hi, acc, lds);
    als_solve<NT>(a, row, hi - lo, acc, lds);
}

// one chunk of a long row: its partial Gram to the batch workspace, lane-major (coalesced)
template <int NT>
__global__ __launch_bounds__(kAlsThreads) void als_chunk_kernel(AlsArgs a) {
    extern __shared__ float4 als_smem[];
    float *lds = reinterpret_cast<float *>(als_smem);
    constexpr int pairs = AlsShape<NT>::pairs;
    const int c = a.chunk0 + blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x16 acc[AlsShape<NT>::per_wave];
    zero_acc<NT>(acc);
    als_accumulate<NT>(a, a.chunk_lo[c], a.chunk_hi[c], acc, lds);
#pragma unroll
    for (int s = 0; s < AlsShape<NT>::per_wave; ++s) {
        const int p = wave + kAlsWaves * s;
        if (p < pairs) {
            float *dst = a.ws + (static_cast<size_t>(blockIdx.x) * pairs + p) * 16 * 64 + lane;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) dst[reg * 64] = acc[s][reg];
        }
    }
}

// a long row: its chunks' partial Grams summed in chunk order, then the solve
template <int NT>
__global__ __launch_bounds__(kAlsThreads) void als_long_kernel(AlsArgs a) {
    extern __shared__ float4 als_smem[];
    float *lds = reinterpret_cast<float *>(als_smem);
    constexpr int pairs = AlsShape<NT>::pairs;
    const int lr = a.row0 + blockIdx.x, row = a.long_rows[lr], wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c_begin = a.long_first_chunk[lr] - a.chunk0, c_end = a.long_first_chunk[lr + 1] - a.chunk0;
    f32x16 acc[AlsShape<NT>::per_wave];
    zero_acc<NT>(acc);
    for (int c = c_begin; c < c_end; ++c) {
#pragma unroll
        for (int s = 0; s < AlsShape<NT>::per_wave; ++s) {
            const int p = wave + kAlsWaves * s;
            if (p < pairs) {
                const float *src = a.ws + (static_cast<size_t>(c) * pairs + p) * 16 * 64 + lane;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) acc[s][reg] = acc[s][reg] + src[reg * 64];
            }
        }
    }
    als_solve<NT>(a, row, a.indptr[row + 1] - a.indptr[row], acc, lds);
}

template <int NT>
int run_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream) {
    constexpr int pairs = AlsShape<NT>::pairs;
    const size_t stage_bytes = static_cast<size_t>(kAlsStep) * AlsShape<NT>::C * sizeof(float);
    const size_t solve_bytes = (solve_lds_floats(p.n_factors) * sizeof(float) + 15) & ~static_cast<size_t>(15);
    const size_t short_bytes = std::max(stage_bytes, solve_bytes);
    if (short_bytes > kMaxLds) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_als: n_factors too large for the LDS of one workgroup");
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_short_kernel<NT>), kMaxLds);
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_chunk_kernel<NT>), kMaxLds);
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_long_kernel<NT>), kMaxLds);
    if (!c.unsolved.ptr) c.unsolved.allocate(1);
    CU2REC_HIP(hipMemsetAsync(c.unsolved.ptr, 0, sizeof(int), stream));
    AlsArgs a{};
    a.indptr = side.indptr;
    a.indices = side.indices;
    a.data = side.data;
    a.p = p;
    a.long_rows = side.d_long_rows.ptr;
    a.long_first_chunk = side.d_long_first_chunk.ptr;
    a.chunk_lo = side.d_chunk_lo.ptr;
    a.chunk_hi = side.d_chunk_hi.ptr;
    a.unsolved = c.unsolved.ptr;
    const int grid = std::min(side.rows, max_rows);
    if (grid > 0)
        hipLaunchKernelGGL(als_short_kernel<NT>, dim3(grid), dim3(kAlsThreads), short_bytes, stream, a);
    CU2REC_HIP(hipGetLastError());
    const int L = static_cast<int>(side.long_rows.size());
    if (L > 0) {
        // batches of whole rows whose partial Grams fit the workspace (at least kAlsMaxChunks: any one row)
        const size_t gram_floats = static_cast<size_t>(pairs) * 16 * 64;
        const int batch_chunks = static_cast<int>(kAlsWorkspaceBytes / (gram_floats * sizeof(float)));
        static_assert(kAlsWorkspaceBytes / (36 * 16 * 64 * sizeof(float)) >= kAlsMaxChunks, "workspace below one row's chunks");
        const int needed = std::min(batch_chunks, side.long_first_chunk[L]);
        if (c.workspace.count < needed * gram_floats) c.workspace.allocate(needed * gram_floats);
        a.ws = c.workspace.ptr;
        for (int r = 0; r < L;) {
            const int c0 = side.long_first_chunk[r];
            int r1 = r + 1;
            while (r1 < L && side.long_first_chunk[r1 + 1] - c0 <= batch_chunks) ++r1;
            a.chunk0 = c0;
            a.row0 = r;
            hipLaunchKernelGGL(als_chunk_kernel<NT>, dim3(side.long_first_chunk[r1] - c0), dim3(kAlsThreads), stage_bytes, stream, a);
            CU2REC_HIP(hipGetLastError());
            hipLaunchKernelGGL(als_long_kernel<NT>, dim3(r1 - r), dim3(kAlsThreads), solve_bytes, stream, a);
            CU2REC_HIP(hipGetLastError());
            r = r1;
        }
    }
    int unsolved = 0;
    CU2REC_HIP(hipMemcpyAsync(&unsolved, c.unsolved.ptr, sizeof(int), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    return unsolved;
}

// ---- the item-major view -------------------------------------------------------------------------------------------------
__global__ void als_row_of_kernel(const int *__restrict__ indptr, int rows, int nnz, int *__restrict__ row_of,
                                  int *__restrict__ pos) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += gridDim.x * blockDim.x) {
        int lo = 0, hi = rows;  // the last u with indptr[u] <= k
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (indptr[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        row_of[k] = lo;
        pos[k] = k;
    }
}

__global__ void als_transpose_kernel(const unsigned *__restrict__ sorted_items, const int *__restrict__ sorted_pos,
                                     const int *__restrict__ row_of, const float *__restrict__ data, int nnz, int cols,
                                     int *__restrict__ t_indptr, int *__restrict__ t_indices, float *__restrict__ t_data) {
    const int stride = gridDim.x * blockDim.x;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) {
        const int k = sorted_pos[p];
        t_indices[p] = row_of[k];
        t_data[p] = data[k];
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= cols; i += stride) {  // first position of item i
        int lo = 0, hi = nnz;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sorted_items[mid] < static_cast<unsigned>(i)) lo = mid + 1;
            else hi = mid;
        }
        t_indptr[i] = lo;
    }
}

}  // namespace

void als_build_transpose(AlsCache &c, const int *indptr, const int *indices, const float *data, int rows, int cols, int nnz,
                         hipStream_t stream) {
    c.t_indptr.allocate(static_cast<size_t>(cols) + 1);
    c.t_indices.allocate(std::max(nnz, 1));
    c.t_data.allocate(std::max(nnz, 1));
    if (nnz == 0) {
        CU2REC_HIP(hipMemsetAsync(c.t_indptr.ptr, 0, (static_cast<size_t>(cols) + 1) * sizeof(int), stream));
        CU2REC_HIP(hipStreamSynchronize(stream));
        return;
    }
    DeviceBuffer<int> row_of(nnz), pos(nnz), pos_sorted(nnz);
    DeviceBuffer<unsigned> items_sorted(nnz);
    const int threads = 256, blocks = static_cast<int>(std::min<size_t>((static_cast<size_t>(nnz) + threads - 1) / threads, 8192));
    hipLaunchKernelGGL(als_row_of_kernel, dim3(blocks), dim3(threads), 0, stream, indptr, rows, nnz, row_of.ptr, pos.ptr);
    CU2REC_HIP(hipGetLastError());
    unsigned bits = 1;
    while (bits < 31 && (1u << bits) < static_cast<unsigned>(cols)) ++bits;
    // LSD radix sort: a chain of stable counting sorts, so rating positions (users ascending) keep their order within an item
    size_t temp_bytes = 0;
    const unsigned *keys_in = reinterpret_cast<const unsigned *>(indices);
    CU2REC_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, items_sorted.ptr, pos.ptr, pos_sorted.ptr, nnz, 0u, bits, stream));
    DeviceBuffer<unsigned char> temp(temp_bytes + 16);
    CU2REC_HIP(rocprim::radix_sort_pairs(temp.ptr, temp_bytes, keys_in, items_sorted.ptr, pos.ptr, pos_sorted.ptr, nnz, 0u, bits, stream));
    const int tblocks = static_cast<int>(std::min<size_t>((static_cast<size_t>(std::max(nnz, cols + 1)) + threads - 1) / threads, 8192));
    hipLaunchKernelGGL(als_transpose_kernel, dim3(tblocks), dim3(threads), 0, stream, items_sorted.ptr, pos_sorted.ptr, row_of.ptr,
                       data, nnz, cols, c.t_indptr.ptr, c.t_indices.ptr, c.t_data.ptr);
    CU2REC_HIP(hipGetLastError());
    CU2REC_HIP(hipStreamSynchronize(stream));  // before the temporaries are freed
}

void als_plan_side(AlsSide &side, hipStream_t stream) {
    std::vector<int> indptr(static_cast<size_t>(side.rows) + 1);
    CU2REC_HIP(hipMemcpyAsync(indptr.data(), side.indptr, indptr.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    std::vector<int> lo, hi;
    side.long_rows.clear();
    side.long_first_chunk.assign(1, 0);
    side.rows_with_ratings = 0;
    side.max_len = 0;
    for (int r = 0; r < side.rows; ++r) {
        const int n = indptr[r + 1] - indptr[r];
        side.rows_with_ratings += n > 0;
        side.max_len = std::max(side.max_len, n);
        if (n <= kAlsChunk) continue;
        const int len = als_chunk_len(n);
        for (int b = indptr[r]; b < indptr[r + 1]; b += len) {
            lo.push_back(b);
            hi.push_back(std::min(b + len, indptr[r + 1]));
        }
        side.long_rows.push_back(r);
        side.long_first_chunk.push_back(static_cast<int>(lo.size()));
    }
    auto put = [](DeviceBuffer<int> &d, const std::vector<int> &h) {
        d.allocate(std::max<size_t>(h.size(), 1));
        if (!h.empty()) d.upload(h.data(), h.size());
    };
    put(side.d_long_rows, side.long_rows);
    put(side.d_long_first_chunk, side.long_first_chunk);
    put(side.d_chunk_lo, lo);
    put(side.d_chunk_hi, hi);
}

int als_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream) {
    const int nt = (p.n_factors + 2 + 31) / 32;  // columns f + 2: factors, the 1, t
    return dispatch_1_to_8(nt, "cu2rec_model_als: n_factors above 252 is not supported",
                           [&](auto tiles) { return run_half_step<tiles()>(c, side, p, max_rows, stream); });
}

}  // namespace cu2rec
