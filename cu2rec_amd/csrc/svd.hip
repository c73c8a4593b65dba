// PureSVD (svd.hpp; include/cu2rec_amd.h: cu2rec_model_svd): block subspace iteration on the rating matrix X,
//   each sweep:  Y = orth(X Q)   Q = orth(X^T Y)      at the end:  P = X Q,  both biases 0
// so that the scores P Q^T = X Q Q^T are X projected on the span of Q.  Only the span matters: no singular values, no Rayleigh-Ritz.
//
// The product (svd_multiply): one wavefront per row in row_wave.hpp's ENTRY map -- four groups of 16 lanes take the row's entries
// g, g + 4, ..., two per group in flight, each lane E float4 of the gathered row of D -- the groups' sums added in group order.  A row
// longer than kAlsChunk is cut by the ALS row plan of its side (one wavefront per chunk, the chunks' partial rows in the ALS
// workspace, added in chunk order by svd_long_sum_kernel).  The order of every sum is a function of the row's length and f alone.
//
// orth (svd_orthonormalize) is Cholesky-QR, twice.  One pass: G = Y^T Y by the implicit half-step's global Gram kernels
// (als_global_gram, unpacked to a dense matrix as als_cg.hip does); svd_factor_kernel, ONE workgroup, factors G = L L^T in LDS as a
// packed lower triangle (right-looking, ALS's solve), inverts L in place row by row (L W = I: row k is scaled by 1 / L_kk and taken off
// the rows below it, position (i, k) of the triangle turning from L_ik into W_ik as it goes) and writes W = L^-1 dense, zero above the
// diagonal and in the padding, beside a status word; svd_apply_kernel forms Y <- Y W^T on v_mfma_f32_32x32x2_f32: a workgroup stages 64
// rows of Y in LDS -- which is what makes the product safe in place -- and each wavefront takes whole 32-column tiles of the result
// for both 32-row halves, reading W through L2 and stopping the contraction at the tile's diagonal block (W is lower triangular).
// Orthonormalising after every single multiply keeps cond(G) at (sigma_1 / sigma_f)^2.  A pivot that is not a finite number above
// 2^-22 of its own diagonal entry (EASE's rule) stops the pass: the host reads the status word once per pass -- the one
// synchronisation per pass -- and the call is refused.  The sweeps run in scratch buffers; the model is written at the end, so a
// refused call leaves it bit for bit.
//
// No float atomics anywhere: a model built twice is bit-identical, and since Q is the only carried state two sweeps twice are four
// sweeps once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "device.hpp"
#include "hip_check.hpp"
#include "mfma_f32.hpp"
#include "objective_pass.hpp"
#include "row_wave.hpp"
#include "svd.hpp"

namespace cu2rec {

namespace {

constexpr float kPivotNoise = 0x1p-22f;  // EASE's
constexpr int kFactorThreads = 1024, kFactorWaves = kFactorThreads / 64;
constexpr int kApplyThreads = 256, kApplyRows = 64;

// ---- the product ---------------------------------------------------------------------------------------------------------------
struct MulArgs {
    const int *indptr, *indices;
    const float *data;
    int rows;
    const float *D;
    int ldd;
    float *out;
    int ldo, f;
    const int *long_rows, *long_first_chunk, *chunk_lo, *chunk_hi;
    int chunk0, row0, n_chunks;  // the batch's first chunk and first long row, and its chunks
    float *ws;                   // the batch's partial rows: [chunk][64 E]
};

// entries [lo, hi) of one row -> sum data * D[idx, :] in the OWNER map; part: the wavefront's [4][64 E] floats
template <int E>
__device__ __forceinline__ void row_product(const MulArgs &a, int lo, int hi, float *part, float (&out)[E]) {
    const int lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    float4 acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e0 = lo; e0 < hi; e0 += 8) {  // two entries per group in flight; each group still adds its entries in ascending order
        float4 q[2][E];
        float r[2];
        bool on[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = e0 + 4 * u + g;
            on[u] = e < hi;
            const int ec = on[u] ? e : hi - 1;
            const int idx = a.indices[ec];
            r[u] = a.data[ec];
#pragma unroll
            for (int k = 0; k < E; ++k) q[u][k] = load_partner4<false>(a.D, a.ldd, a.f, idx, 4 * l16 + 64 * k);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (on[u]) {
#pragma unroll
                for (int k = 0; k < E; ++k) axpy4(r[u], q[u][k], acc[k]);
            }
    }
    float *mine = part + g * (64 * E) + 4 * l16;
    wave_sync();  // the row before has read part
    combine_groups<E>(acc, part, mine, lane, out);
}

// rows of at most kAlsChunk entries (none: the zero row), a wavefront each, the workgroups striding over the rows
template <int E>
__global__ __launch_bounds__(kRowThreads) void svd_multiply_kernel(MulArgs a) {
    __shared__ float4 part_s[kRowWaves][64 * E];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *part = reinterpret_cast<float *>(part_s[wave]);
    for (int row = blockIdx.x * kRowWaves + wave; row < a.rows; row += gridDim.x * kRowWaves) {
        const int lo = a.indptr[row], hi = a.indptr[row + 1];
        if (hi - lo > kAlsChunk) continue;  // the chunk and sum kernels' row
        float v[E];
        row_product<E>(a, lo, hi, part, v);
        float *y = a.out + static_cast<size_t>(row) * a.ldo;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int c = lane + 64 * k;
            if (c < a.ldo) y[c] = c < a.f ? v[k] : 0.f;
        }
        for (int c = lane + 64 * E; c < a.ldo; c += 64) y[c] = 0.f;
    }
}

// one chunk of a long row per wavefront: its partial row to the batch workspace
template <int E>
__global__ __launch_bounds__(kRowThreads) void svd_chunk_kernel(MulArgs a) {
    __shared__ float4 part_s[kRowWaves][64 * E];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * kRowWaves + wave;
    if (c >= a.n_chunks) return;  // no workgroup-wide barrier below: the wavefronts are independent
    float v[E];
    row_product<E>(a, a.chunk_lo[a.chunk0 + c], a.chunk_hi[a.chunk0 + c], reinterpret_cast<float *>(part_s[wave]), v);
    float *dst = a.ws + static_cast<size_t>(c) * (64 * E);
#pragma unroll
    for (int k = 0; k < E; ++k) dst[lane + 64 * k] = v[k];
}

// a long row per workgroup: its chunks' partial rows added in chunk order, a thread per column
template <int E>
__global__ __launch_bounds__(64 * E) void svd_long_sum_kernel(MulArgs a) {
    const int lr = a.row0 + blockIdx.x, row = a.long_rows[lr], c = threadIdx.x;
    const int c_begin = a.long_first_chunk[lr] - a.chunk0, c_end = a.long_first_chunk[lr + 1] - a.chunk0;
    float s = a.ws[static_cast<size_t>(c_begin) * (64 * E) + c];
    for (int k = c_begin + 1; k < c_end; ++k) s = s + a.ws[static_cast<size_t>(k) * (64 * E) + c];
    float *y = a.out + static_cast<size_t>(row) * a.ldo;
    for (int j = c; j < a.ldo; j += 64 * E) y[j] = j < a.f ? s : 0.f;  // j == c for every column that holds data
}

template <int E>
void run_multiply(AlsCache &c, const AlsSide &side, MulArgs a, hipStream_t stream) {
    hipLaunchKernelGGL(svd_multiply_kernel<E>, dim3(row_grid(a.rows)), dim3(kRowThreads), 0, stream, a);
    CU2REC_HIP(hipGetLastError());
    const int L = static_cast<int>(side.long_rows.size());
    if (L == 0) return;
    // batches of whole rows whose partial rows fit the workspace (any one row: at most kAlsMaxChunks chunks)
    const int batch_chunks = static_cast<int>(kAlsWorkspaceBytes / (64 * E * sizeof(float)));
    static_assert(kAlsWorkspaceBytes / (256 * sizeof(float)) >= static_cast<size_t>(kAlsMaxChunks), "workspace below one row's chunks");
    const size_t needed = static_cast<size_t>(std::min(batch_chunks, side.long_first_chunk[L])) * (64 * E);
    if (c.workspace.count < needed) c.workspace.allocate(needed);
    a.ws = c.workspace.ptr;
    for (int r = 0; r < L;) {
        const int c0 = side.long_first_chunk[r];
        int r1 = r + 1;
        while (r1 < L && side.long_first_chunk[r1 + 1] - c0 <= batch_chunks) ++r1;
        a.chunk0 = c0;
        a.row0 = r;
        a.n_chunks = side.long_first_chunk[r1] - c0;
        hipLaunchKernelGGL(svd_chunk_kernel<E>, dim3((a.n_chunks + kRowWaves - 1) / kRowWaves), dim3(kRowThreads), 0, stream, a);
        hipLaunchKernelGGL(svd_long_sum_kernel<E>, dim3(r1 - r), dim3(64 * E), 0, stream, a);
        CU2REC_HIP(hipGetLastError());
        r = r1;
    }
}

// ---- orth: the factor and its inverse -------------------------------------------------------------------------------------------
__host__ __device__ inline size_t factor_lds_floats(int f) { return static_cast<size_t>(tri(f)) + 3 * static_cast<size_t>((f + 3) & ~3); }

// G: dense [f][S], its lower triangle read.  -> W = L^-1: dense [C][C] (C = f rounded up to 32), zero above the diagonal and from f on.
// status[0] != 0: pivot status[1] was refused and W is not written.
__global__ __launch_bounds__(kFactorThreads) void svd_factor_kernel(const float *__restrict__ G, int f, int S, float *__restrict__ W, int C,
                                                                    int *__restrict__ status) {
    extern __shared__ float4 svd_factor_smem[];
    float *L = reinterpret_cast<float *>(svd_factor_smem);
    const int F4 = (f + 3) & ~3;
    float *col = L + tri(f), *rowk = col + F4, *diag = rowk + F4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < f * f; e += kFactorThreads) {
        const int i = e / f, j = e - i * f;
        if (j <= i) L[tri(i) + j] = G[i * S + j];
        if (j == i) diag[i] = G[i * S + j];
    }
    for (int k = 0; k < f; ++k) {  // G = L L^T, right-looking
        __syncthreads();
        const float d = L[tri(k) + k];  // the same value in every thread: the exit is the workgroup's
        if (!(d > 0.f) || !(d > kPivotNoise * diag[k]) || !(d <= 3.402823466e+38f)) {
            if (tid == 0) {
                status[1] = k;
                status[0] = 1;
            }
            return;
        }
        const float l = sqrtf(d);
        for (int i = k + 1 + tid; i < f; i += kFactorThreads) {
            const float v = L[tri(i) + k] / l;
            L[tri(i) + k] = v;
            col[i] = v;
        }
        __syncthreads();
        if (tid == 0) L[tri(k) + k] = l;  // after the barrier: every thread has read the pivot by now
        for (int i = k + 1 + wave; i < f; i += kFactorWaves) {
            const float ci = col[i];
            float *gi = L + tri(i);
            for (int j = k + 1 + lane; j <= i; j += 64) gi[j] = fmaf(-ci, col[j], gi[j]);
        }
    }
    for (int k = 0; k < f; ++k) {  // L W = I in place: row k of W is finished, then taken off the rows below it
        __syncthreads();
        const float p = 1.f / L[tri(k) + k];
        for (int i = k + 1 + tid; i < f; i += kFactorThreads) col[i] = L[tri(i) + k];
        for (int j = tid; j < k; j += kFactorThreads) rowk[j] = L[tri(k) + j] * p;
        __syncthreads();
        if (tid == 0) L[tri(k) + k] = p;
        for (int j = tid; j < k; j += kFactorThreads) L[tri(k) + j] = rowk[j];
        for (int i = k + 1 + wave; i < f; i += kFactorWaves) {
            const float m = col[i];
            float *gi = L + tri(i);
            for (int j = lane; j < k; j += 64) gi[j] = fmaf(-m, rowk[j], gi[j]);
            if (lane == 0) gi[k] = -(m * p);
        }
    }
    __syncthreads();
    for (int e = tid; e < C * C; e += kFactorThreads) {
        const int i = e / C, j = e - i * C;
        W[e] = i < f && j <= i ? L[tri(i) + j] : 0.f;
    }
}

// ---- orth: Y <- Y W^T --------------------------------------------------------------------------------------------------------------
// Workgroup b: rows [64 b, 64 b + 64) of Y, staged in LDS with the columns from f on as zeros.  Column tile t of the result
// (columns 32 t .. 32 t + 31) is out[r][j] = sum_{k < 32 (t + 1)} y[r][k] W[j][k]; the wavefront that owns t keeps both 32-row halves'
// accumulators and reads W once for the two.  The contraction takes k in blocks of 8: the lanes of half h hold k = 8 m + 4 h .. + 3
// (one float4 of the staged row, one of W's row), MFMA step s of the block pairs k = 8 m + s with 8 m + 4 + s.
__global__ __launch_bounds__(kApplyThreads) void svd_apply_kernel(float *__restrict__ Y, int ld, int n, int f, const float *__restrict__ W,
                                                                  int C, const int *__restrict__ status) {
    extern __shared__ float4 svd_apply_smem[];
    if (status[0]) return;
    float *ys = reinterpret_cast<float *>(svd_apply_smem);
    const int LS = C + 4;  // rows stay 16-byte aligned and a column of float4 reads spreads over the banks
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * kApplyRows;
    for (int e = tid; e < kApplyRows * C; e += kApplyThreads) {
        const int i = e / C, c = e - i * C, row = row0 + i;
        ys[i * LS + c] = row < n && c < f ? Y[static_cast<size_t>(row) * ld + c] : 0.f;
    }
    __syncthreads();  // from here on Y is only written: every row this workgroup reads is in LDS
    const int NT = C / 32;
    for (int t = 0; t < NT; ++t) {
        if ((t < 4 ? t : 7 - t) != wave) continue;  // tiles t and 7 - t: the same work for every wavefront at f > 224
        f32x16 acc0, acc1;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc0[reg] = acc1[reg] = 0.f;
        const float *w = W + static_cast<size_t>(32 * t + r) * C + 4 * h;
        const float *y0 = ys + r * LS + 4 * h, *y1 = y0 + 32 * LS;
        for (int m = 0; m < 4 * (t + 1); ++m) {
            const float4 b = *reinterpret_cast<const float4 *>(w + 8 * m);
            const float4 x0 = *reinterpret_cast<const float4 *>(y0 + 8 * m), x1 = *reinterpret_cast<const float4 *>(y1 + 8 * m);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, b.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, b.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, b.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, b.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, b.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, b.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, b.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, b.w, acc1, 0, 0, 0);
        }
        const int c = 32 * t + r;
        if (c < f) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i0 = row0 + acc_row(reg, h), i1 = i0 + 32;
                if (i0 < n) Y[static_cast<size_t>(i0) * ld + c] = acc0[reg];
                if (i1 < n) Y[static_cast<size_t>(i1) * ld + c] = acc1[reg];
            }
        }
    }
    const int pad = ld - f;  // the padding columns are written as zero
    for (int e = tid; e < kApplyRows * pad; e += kApplyThreads) {
        const int i = e / pad, c = f + (e - i * pad), row = row0 + i;
        if (row < n) Y[static_cast<size_t>(row) * ld + c] = 0.f;
    }
}

// ---- the norms -------------------------------------------------------------------------------------------------------------------
constexpr int kNormMaxBlocks = 1024;

// per-block partial sums of x[i][0 .. f)^2 over n rows of stride ld, in double
__global__ __launch_bounds__(kObjThreads) void svd_sum_squares_kernel(const float *__restrict__ x, size_t n, int f, int ld,
                                                                      double *__restrict__ partials) {
    __shared__ double red[1][kObjThreads];
    const size_t total = n * static_cast<size_t>(f);
    double s[1] = {0.0};
    for (size_t e = static_cast<size_t>(blockIdx.x) * kObjThreads + threadIdx.x; e < total; e += static_cast<size_t>(gridDim.x) * kObjThreads) {
        const size_t i = e / f;
        const double v = static_cast<double>(x[i * ld + (e - i * f)]);
        s[0] += v * v;
    }
    block_reduce(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0][0];
}

// the same over the values of a row-sorted view, a run of one column within a row added up (in float, in stored order) first
__global__ __launch_bounds__(kObjThreads) void svd_total_kernel(const int *__restrict__ indptr, const int *__restrict__ row_of,
                                                                const int *__restrict__ idx, const float *__restrict__ val, int nnz,
                                                                double *__restrict__ partials) {
    __shared__ double red[1][kObjThreads];
    double s[1] = {0.0};
    for (int e = blockIdx.x * kObjThreads + threadIdx.x; e < nnz; e += gridDim.x * kObjThreads) {
        const int u = row_of[e], lo = indptr[u], hi = indptr[u + 1];
        if (e > lo && idx[e - 1] == idx[e]) continue;  // inside a run: its first entry's
        float v = val[e];
        for (int j = e + 1; j < hi && idx[j] == idx[e]; ++j) v = v + val[j];
        s[0] += static_cast<double>(v) * static_cast<double>(v);
    }
    block_reduce(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0][0];
}

int norm_blocks(size_t work) {
    return static_cast<int>(std::min<size_t>(std::max<size_t>((work + kObjThreads * 8 - 1) / (kObjThreads * 8), 1), kNormMaxBlocks));
}

void check_strides(const char *what, int ld, int f) {
    if (ld % 4 != 0 || ld < ((f + 3) & ~3)) fail(CU2REC_EINVAL, std::string(what) + ": a row stride must be a multiple of 4 and >= n_factors rounded up to 4");
}

}  // namespace

void svd_multiply(AlsCache &c, const AlsSide &side, const float *D, int ldd, float *out, int ldo, int f, hipStream_t stream) {
    if (f < 1 || f > kAlsMaxFactors) fail(CU2REC_EUNSUPPORTED, "svd_multiply: n_factors must be in [1, CU2REC_ALS_MAX_FACTORS]");
    check_strides("svd_multiply", ldd, f);
    check_strides("svd_multiply", ldo, f);
    if (side.rows <= 0) return;
    MulArgs a{side.indptr, side.indices, side.data, side.rows, D, ldd, out, ldo, f, side.d_long_rows.ptr, side.d_long_first_chunk.ptr,
              side.d_chunk_lo.ptr, side.d_chunk_hi.ptr, 0, 0, 0, nullptr};
    dispatch_1_to_4(f, [&](auto elems) { run_multiply<elems()>(c, side, a, stream); });
}

int svd_orthonormalize(AlsCache &c, SvdOrthScratch &s, float *Y, int ld, int n, int f, hipStream_t stream) {
    if (f < 1 || f > kAlsMaxFactors) fail(CU2REC_EUNSUPPORTED, "svd_orthonormalize: n_factors must be in [1, CU2REC_ALS_MAX_FACTORS]");
    check_strides("svd_orthonormalize", ld, f);
    const int S = (f + 3) & ~3, C = (f + 31) & ~31;
    if (s.dense.count < static_cast<size_t>(f) * S) s.dense.allocate(static_cast<size_t>(f) * S);
    if (s.inverse.count < static_cast<size_t>(C) * C) s.inverse.allocate(static_cast<size_t>(C) * C);
    if (!s.status.ptr) s.status.allocate(2);
    const size_t factor_bytes = (factor_lds_floats(f) * sizeof(float) + 15) & ~static_cast<size_t>(15);
    const size_t apply_bytes = static_cast<size_t>(kApplyRows) * (C + 4) * sizeof(float);
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&svd_factor_kernel));
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&svd_apply_kernel));
    for (int pass = 0; pass < 2; ++pass) {
        CU2REC_HIP(hipMemsetAsync(s.status.ptr, 0, 2 * sizeof(int), stream));
        als_global_gram(c, Y, ld, n, f, s.gram, stream);
        als_unpack_gram(s.gram.ptr, s.dense.ptr, f, S, stream);
        hipLaunchKernelGGL(svd_factor_kernel, dim3(1), dim3(kFactorThreads), factor_bytes, stream, s.dense.ptr, f, S, s.inverse.ptr, C, s.status.ptr);
        CU2REC_HIP(hipGetLastError());
        if (n > 0) {
            hipLaunchKernelGGL(svd_apply_kernel, dim3((n + kApplyRows - 1) / kApplyRows), dim3(kApplyThreads), apply_bytes, stream, Y, ld, n, f,
                               s.inverse.ptr, C, s.status.ptr);
            CU2REC_HIP(hipGetLastError());
        }
        int h_status[2] = {0, 0};
        CU2REC_HIP(hipMemcpyAsync(h_status, s.status.ptr, sizeof(h_status), hipMemcpyDeviceToHost, stream));
        CU2REC_HIP(hipStreamSynchronize(stream));  // the pass's one synchronisation
        if (h_status[0]) return h_status[1];
    }
    return -1;
}

namespace {
double sum_partials(DeviceBuffer<double> &partials, int blocks, hipStream_t stream) {
    double out[1];
    sum_block_partials(partials, blocks, out, stream);
    return out[0];
}
}  // namespace

double svd_sum_squares(const float *x, int n, int f, int ld, hipStream_t stream) {
    if (n <= 0 || f <= 0) return 0.0;
    const int blocks = norm_blocks(static_cast<size_t>(n) * f);
    DeviceBuffer<double> partials(blocks);
    hipLaunchKernelGGL(svd_sum_squares_kernel, dim3(blocks), dim3(kObjThreads), 0, stream, x, static_cast<size_t>(n), f, ld, partials.ptr);
    CU2REC_HIP(hipGetLastError());
    return sum_partials(partials, blocks, stream);
}

double svd_total(const DeviceCsr &csr, hipStream_t stream) {
    if (csr.nnz <= 0) return 0.0;
    if (!row_sorted_view(csr, false, stream).has_duplicate) return svd_sum_squares(csr.data.ptr, 1, csr.nnz, csr.nnz, stream);
    const RowSortedView &rows = row_sorted_view(csr, true, stream);
    const int *row_of = row_of_view(csr, stream);
    const int blocks = norm_blocks(static_cast<size_t>(csr.nnz));
    DeviceBuffer<double> partials(blocks);
    hipLaunchKernelGGL(svd_total_kernel, dim3(blocks), dim3(kObjThreads), 0, stream, csr.indptr.ptr, row_of, rows.idx.ptr, rows.val.ptr, csr.nnz,
                       partials.ptr);
    CU2REC_HIP(hipGetLastError());
    return sum_partials(partials, blocks, stream);
}

namespace {

std::string pivot_message(const char *fn, const char *what, int column) {
    return std::string(fn) + ": " + what + ": the pivot of column " + std::to_string(column) +
           " is not a finite number above 2^-22 of its diagonal entry (n_factors above the numerical rank, a zero matrix or a NaN value)";
}

void check_svd_shapes(const Need &need, const DeviceModel &m, const DeviceCsr &train) {
    need(train.rows <= m.rows && train.cols <= m.cols && train.max_item < m.cols, CU2REC_EINVAL, ": ratings exceed the model's shape");
    need(m.n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
    need(train.rows >= m.n_factors && train.cols >= m.n_factors, CU2REC_EUNSUPPORTED, ": fewer rows or columns than n_factors");
}

void enter(DeviceModel &m) {
    require_device();
    check_faults();
    m.finish_swap();
}

}  // namespace

// include/cu2rec_amd.h: cu2rec_model_svd
void model_svd(DeviceModel &m, const DeviceCsr &train, int sweeps, cu2rec_svd_report *report, hipStream_t stream) {
    const Need need{"cu2rec_model_svd"};
    need(sweeps >= 1, CU2REC_EINVAL, ": sweeps must be >= 1");
    check_svd_shapes(need, m, train);
    enter(m);
    const int f = m.n_factors;
    const AlsSide &users = als_side(train, true, stream), &items = als_side(train, false, stream);
    // the sweeps run beside the model: Q's start is copied, Y and P are scratch; rows of the model outside the matrix stay zero
    DeviceBuffer<float> Qs(m.Q.count), Ps(m.P.count), Y(std::max<size_t>(static_cast<size_t>(train.rows) * m.ld, 4));
    CU2REC_HIP(hipMemsetAsync(Qs.ptr, 0, Qs.count * sizeof(float), stream));
    CU2REC_HIP(hipMemsetAsync(Ps.ptr, 0, Ps.count * sizeof(float), stream));
    CU2REC_HIP(hipMemcpyAsync(Qs.ptr, m.Q.ptr, static_cast<size_t>(train.cols) * m.ldq * sizeof(float), hipMemcpyDeviceToDevice, stream));
    SvdOrthScratch scratch;
    for (int s = 0; s < sweeps; ++s) {
        svd_multiply(train.als, users, Qs.ptr, m.ldq, Y.ptr, m.ld, f, stream);
        int bad = svd_orthonormalize(train.als, scratch, Y.ptr, m.ld, train.rows, f, stream);
        if (bad >= 0) fail(CU2REC_EUNSUPPORTED, pivot_message("cu2rec_model_svd", ("sweep " + std::to_string(s) + ", X Q").c_str(), bad));
        svd_multiply(train.als, items, Y.ptr, m.ld, Qs.ptr, m.ldq, f, stream);
        bad = svd_orthonormalize(train.als, scratch, Qs.ptr, m.ldq, train.cols, f, stream);
        if (bad >= 0) fail(CU2REC_EUNSUPPORTED, pivot_message("cu2rec_model_svd", ("sweep " + std::to_string(s) + ", X^T Y").c_str(), bad));
    }
    svd_multiply(train.als, users, Qs.ptr, m.ldq, Ps.ptr, m.ld, f, stream);
    const double captured = svd_sum_squares(Ps.ptr, train.rows, f, m.ld, stream), total = svd_total(train, stream);
    CU2REC_HIP(hipMemcpyAsync(m.Q.ptr, Qs.ptr, Qs.count * sizeof(float), hipMemcpyDeviceToDevice, stream));
    CU2REC_HIP(hipMemcpyAsync(m.P.ptr, Ps.ptr, Ps.count * sizeof(float), hipMemcpyDeviceToDevice, stream));
    CU2REC_HIP(hipMemsetAsync(m.user_bias.ptr, 0, m.user_bias.count * sizeof(float), stream));
    CU2REC_HIP(hipMemsetAsync(m.item_bias.ptr, 0, m.item_bias.count * sizeof(float), stream));
    CU2REC_HIP(hipStreamSynchronize(stream));  // before the scratch buffers are freed
    m.other_in_sync = false;                   // Q moved on without the ping-pong pair
    if (report) *report = cu2rec_svd_report{sweeps, captured, total};
}

// include/cu2rec_amd.h: cu2rec_model_project
void model_project(DeviceModel &m, const DeviceCsr &history, float *out_host, hipStream_t stream) {
    const Need need{"cu2rec_model_project"};
    need(history.cols == m.cols, CU2REC_EINVAL, ": the history's column count differs from the model's");
    need(m.n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
    if (history.rows == 0) return;
    enter(m);
    const AlsSide &rows = als_side(history, true, stream);
    DeviceBuffer<float> out(static_cast<size_t>(history.rows) * m.ld);
    svd_multiply(history.als, rows, m.Q.ptr, m.ldq, out.ptr, m.ld, m.n_factors, stream);
    CU2REC_HIP(hipStreamSynchronize(stream));
    download_padded(out, out_host, history.rows, m.n_factors, m.ld);
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_model_svd(cu2rec_model *m, const cu2rec_csr *train, int sweeps, cu2rec_svd_report *report) {
    return guarded([&] {
        require(m && train, "cu2rec_model_svd: null argument");
        model_svd(unwrap(m), unwrap(train), sweeps, report, nullptr);
    });
}

int cu2rec_model_project(cu2rec_model *m, const cu2rec_csr *history, float *out) {
    return guarded([&] {
        require(m && history && out, "cu2rec_model_project: null argument");
        model_project(unwrap(m), unwrap(history), out, nullptr);
    });
}

int cu2rec_train_svd(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, int verbose, cu2rec_svd_report *report) {
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_svd: null argument");
        DeviceModel &m = unwrap(model);
        const DeviceCsr &t = unwrap(train);
        const Need need{"cu2rec_train_svd"};
        need(cfg->n_factors == m.n_factors, CU2REC_EINVAL, ": cfg.n_factors differs from the model's");
        need(cfg->total_iterations >= 1, CU2REC_EINVAL, ": total_iterations (the sweeps) must be >= 1");
        need(m.global_bias == 0.f, CU2REC_EINVAL, ": the model's global_bias must be 0 (the scores are p . q)");
        check_svd_shapes(need, m, t);
        if (cfg->seed != 42) {  // a fresh model's arrays are the seed-42 draw: another seed draws the start again
            require_device();
            std::vector<float> q(static_cast<size_t>(m.cols) * m.n_factors);
            cu2rec_init_normal(q.data(), q.size(), m.n_factors, 0.f, 1.f, cfg->seed);
            if (m.cols)
                CU2REC_HIP(hipMemcpy2D(m.Q.ptr, static_cast<size_t>(m.ldq) * sizeof(float), q.data(), static_cast<size_t>(m.n_factors) * sizeof(float),
                                       static_cast<size_t>(m.n_factors) * sizeof(float), m.cols, hipMemcpyHostToDevice));
        }
        cu2rec_svd_report rep{};
        model_svd(m, t, cfg->total_iterations, &rep, nullptr);
        cfg->cur_iterations += rep.sweeps;
        if (verbose) std::printf("SVD: Factors: %d Sweeps: %d Captured: %f Total: %f Share: %f\n", m.n_factors, rep.sweeps, rep.captured, rep.total,
                                 rep.total > 0.0 ? rep.captured / rep.total : 0.0);
        if (report) *report = rep;
    });
}

int cu2rec_csr_multiply(const cu2rec_csr *csr, int transpose, const float *D, int f, float *out) {
    return guarded([&] {
        require(csr && D && out, "cu2rec_csr_multiply: null argument");
        Need{"cu2rec_csr_multiply"}(f >= 1 && f <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": f must be in [1, CU2REC_ALS_MAX_FACTORS]");
        const DeviceCsr &m = unwrap(csr);
        // the model's strides: the user side's rows at f rounded up to 4, the item side's at f rounded up to 32
        const int ld_users = (f + 3) & ~3, ld_items = (f + 31) & ~31;
        const int n_in = transpose ? m.rows : m.cols, n_out = transpose ? m.cols : m.rows;
        const int ld_in = transpose ? ld_users : ld_items, ld_out = transpose ? ld_items : ld_users;
        if (n_out == 0) return;
        require_device();
        check_faults();
        hipStream_t stream = nullptr;
        DeviceBuffer<float> d_in(std::max<size_t>(static_cast<size_t>(n_in) * ld_in, 4)), d_out(static_cast<size_t>(n_out) * ld_out);
        CU2REC_HIP(hipMemset(d_in.ptr, 0xFF, d_in.count * sizeof(float)));  // the padding columns hold NaNs: they are never read as data
        if (n_in)
            CU2REC_HIP(hipMemcpy2D(d_in.ptr, static_cast<size_t>(ld_in) * sizeof(float), D, static_cast<size_t>(f) * sizeof(float),
                                   static_cast<size_t>(f) * sizeof(float), n_in, hipMemcpyHostToDevice));
        CU2REC_HIP(hipMemset(d_out.ptr, 0xFF, d_out.count * sizeof(float)));
        svd_multiply(m.als, als_side(m, !transpose, stream), d_in.ptr, ld_in, d_out.ptr, ld_out, f, stream);
        CU2REC_HIP(hipStreamSynchronize(stream));
        // the whole padded rows come back: out is n_out x ld_out
        d_out.download(out, d_out.count);
    });
}

int cu2rec_csr_multiply_stride(int transpose, int f) { return transpose ? (f + 31) & ~31 : (f + 3) & ~3; }

int cu2rec_orthonormalize(float *Y, int n, int f, int *bad_column) {
    return guarded([&] {
        require(Y && n >= 0, "cu2rec_orthonormalize: null argument or negative n");
        if (bad_column) *bad_column = -1;
        Need{"cu2rec_orthonormalize"}(f >= 1 && f <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": f must be in [1, CU2REC_ALS_MAX_FACTORS]");
        if (n < f) {
            if (bad_column) *bad_column = n;
            fail(CU2REC_EUNSUPPORTED, "cu2rec_orthonormalize: fewer rows than columns: column " + std::to_string(n) + " depends on the ones before it");
        }
        require_device();
        check_faults();
        hipStream_t stream = nullptr;
        const int ld = (f + 3) & ~3;
        DeviceBuffer<float> d(static_cast<size_t>(n) * ld);
        CU2REC_HIP(hipMemset(d.ptr, 0xFF, d.count * sizeof(float)));  // NaNs in the padding: never read as data
        CU2REC_HIP(hipMemcpy2D(d.ptr, static_cast<size_t>(ld) * sizeof(float), Y, static_cast<size_t>(f) * sizeof(float),
                               static_cast<size_t>(f) * sizeof(float), n, hipMemcpyHostToDevice));
        AlsCache cache;
        SvdOrthScratch scratch;
        const int bad = svd_orthonormalize(cache, scratch, d.ptr, ld, n, f, stream);
        if (bad >= 0) {
            if (bad_column) *bad_column = bad;
            fail(CU2REC_EUNSUPPORTED, pivot_message("cu2rec_orthonormalize", "Y", bad));
        }
        download_padded(d, Y, n, f, ld);
    });
}

}  // extern "C"
