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
//
// The implicit-feedback half-step (cu2rec_model_als_implicit) is the same machinery with three differences, each a case of AlsKind
// in the templates below.  (1) Every partner row counts, so a half-step first forms G0 = X^T X over partner rows [0, n): the rows
// are tiled kAlsChunk at a time, one workgroup per tile gathers BY ROW NUMBER and accumulates exactly as above (AlsKind::Gram),
// the tiles' partial Grams go to the workspace and a second kernel adds them in tile order into a buffer kept in the accumulator
// layout [pair][16][64].  (2) A row's own entries are staged as two operands, A = [w q | 1 + w] and B = [q | 0] (w = alpha r), so
// that the product's first f rows are sum w q q^T and its row f is the right-hand side sum (1 + w) q; the accumulators start from
// G0 (AlsKind::Implicit).  (3) The system has order f (no bias), plain reg on the diagonal, and a row without entries is written
// as zeros.  With cg_steps > 0 (cu2rec_model_als_implicit_cg) the rows of at most kAlsChunk entries go to als_cg.hip instead of the
// short kernel; G0 and the long rows' kernels are the same.  The explicit half-step has the same switch (cu2rec_model_als_cg): its
// short rows go to als_cg.hip's explicit instantiation, which needs no G0 at all.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "als.hpp"
#include "kernels.hpp"
#include "objective_pass.hpp"
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
    int chunk0, row0;  // first chunk / first long row of the batch (AlsKind::Gram: chunk = tile of kAlsChunk partner rows)
    float *ws;         // the batch's partial Grams: [chunk][pair][16][64]
    const float *g0;   // AlsKind::Implicit: X^T X over partner rows [0, p.x_rows), [pair][16][64]
    int *unsolved;
};

template <int NT>
struct AlsShape {
    static constexpr int C = 32 * NT;  // staged columns
    static constexpr int pairs = NT * (NT + 1) / 2;
    static constexpr int per_wave = (pairs + kAlsWaves - 1) / kAlsWaves;
};

__device__ inline void pair_tiles(int p, int &ti, int &tj) {  // pair p of the row-major lower triangle of tiles
    ti = 0;
    while (tri(ti + 1) <= p) ++ti;
    tj = p - tri(ti);
}

__host__ __device__ inline size_t solve_lds_floats(int f) {  // packed augmented triangle + three vectors of order f + 2 + a flag
    return static_cast<size_t>(tri(f + 2)) + 3 * static_cast<size_t>(f + 4) + 4;
}

// acc += the augmented Gram of ratings [lo, hi) of the current row, kAlsStep ratings per LDS stage.  AlsKind::Gram: [lo, hi) are
// partner row numbers.  AlsKind::Implicit: the A operand is staged at zs, the B operand kAlsStep x C floats behind it.
template <int NT, AlsKind K>
__device__ void als_accumulate(const AlsArgs &a, int lo, int hi, f32x16 (&acc)[AlsShape<NT>::per_wave], float *zs) {
    constexpr int C = AlsShape<NT>::C, S4 = C / 4, pairs = AlsShape<NT>::pairs;
    constexpr int b_off = K == AlsKind::Implicit ? kAlsStep * C : 0;  // the B operand's stage (the A operand's own otherwise)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int F = a.p.n_factors;
    float4 *zs4 = reinterpret_cast<float4 *>(zs);
    for (int k0 = lo; k0 < hi; k0 += kAlsStep) {
        __syncthreads();  // the previous stage's operands have been read
        for (int e = tid; e < kAlsStep * S4; e += kAlsThreads) {
            const int row = e / S4, s = e - row * S4, k = k0 + row, c0 = 4 * s;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            [[maybe_unused]] float4 va = v;  // AlsKind::Implicit: [w x | 1 + w | 0]
            if (k < hi) {
                const int idx = K == AlsKind::Gram ? k : a.indices[k];
                if (c0 < F) v = *reinterpret_cast<const float4 *>(a.p.X + static_cast<size_t>(idx) * a.p.ldx + c0);
                if constexpr (K == AlsKind::Explicit) {
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
                } else {
                    if (c0 + 3 >= F) {  // zero fill from column F on
                        if (c0 >= F) v.x = 0.f;
                        if (c0 + 1 >= F) v.y = 0.f;
                        if (c0 + 2 >= F) v.z = 0.f;
                        if (c0 + 3 >= F) v.w = 0.f;
                    }
                    if constexpr (K == AlsKind::Implicit) {
                        const float w = a.p.alpha * a.data[k];
                        va = make_float4(w * v.x, w * v.y, w * v.z, w * v.w);
                        if (c0 == F) va.x = 1.f + w;  // column F of the A operand: the right-hand side's weight
                        if (c0 + 1 == F) va.y = 1.f + w;
                        if (c0 + 2 == F) va.z = 1.f + w;
                        if (c0 + 3 == F) va.w = 1.f + w;
                    }
                }
            }
            if constexpr (K == AlsKind::Implicit) {
                zs4[row * S4 + s] = va;
                zs4[b_off / 4 + row * S4 + s] = v;
            } else {
                zs4[row * S4 + s] = v;
            }
        }
        __syncthreads();
        // A[i][k] = Z[k][32 ti + i], B[k][j] = Z[k][32 tj + j]: lane (r, h) feeds row 2 kk + h of the stage
#pragma unroll
        for (int s = 0; s < AlsShape<NT>::per_wave; ++s) {
            const int p = wave + kAlsWaves * s;
            if (p < pairs) {
                int ti, tj;
                pair_tiles(p, ti, tj);
                const float *za = zs + h * C + 32 * ti + r, *zb = zs + b_off + h * C + 32 * tj + r;
#pragma unroll
                for (int kk = 0; kk < kAlsStep / 2; ++kk)
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[2 * kk * C], zb[2 * kk * C], acc[s], 0, 0, 0);
            }
        }
    }
}

// the accumulated augmented Gram of `row` (n ratings) -> Cholesky in LDS -> the row's factors and bias, or counted as unsolved.
// AlsKind::Implicit: order f, plain reg on the diagonal, the bias written as 0.
template <int NT, AlsKind K>
__device__ void als_solve(const AlsArgs &a, int row, int n, f32x16 (&acc)[AlsShape<NT>::per_wave], float *lds) {
    constexpr int pairs = AlsShape<NT>::pairs;
    constexpr bool with_bias = K == AlsKind::Explicit;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int F = a.p.n_factors, D = F + (with_bias ? 1 : 0);  // system order D; row D of the augmented triangle is the right-hand side
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
                    if (i == j && i < D) v = v + (with_bias ? nf * (i < F ? a.p.reg : a.p.reg_bias) : a.p.reg);
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
    if (tid == 0) a.p.yb[row] = with_bias ? xo[F] : 0.f;
}

template <int NT>
__device__ inline void zero_acc(f32x16 (&acc)[AlsShape<NT>::per_wave]) {
#pragma unroll
    for (int s = 0; s < AlsShape<NT>::per_wave; ++s)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
}

// acc += one Gram in the accumulator layout [pair][16][64] (a chunk's partial Gram, or G0)
template <int NT>
__device__ inline void add_gram(f32x16 (&acc)[AlsShape<NT>::per_wave], const float *gram) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < AlsShape<NT>::per_wave; ++s) {
        const int p = wave + kAlsWaves * s;
        if (p < AlsShape<NT>::pairs) {
            const float *src = gram + static_cast<size_t>(p) * 16 * 64 + lane;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc[s][reg] = acc[s][reg] + src[reg * 64];
        }
    }
}

// the accumulators a row starts from: zero, or G0 for the implicit half-step
template <int NT, AlsKind K>
__device__ inline void seed_acc(const AlsArgs &a, f32x16 (&acc)[AlsShape<NT>::per_wave]) {
    zero_acc<NT>(acc);
    if constexpr (K == AlsKind::Implicit) add_gram<NT>(acc, a.g0);
}

// rows of 1 .. kAlsChunk ratings: one workgroup each, gather, Gram and solve.  AlsKind::Implicit: a row without entries has right-hand
// side 0, so its minimiser is the zero row: written, not factorised, not counted.
template <int NT, AlsKind K>
__global__ __launch_bounds__(kAlsThreads) void als_short_kernel(AlsArgs a) {
    extern __shared__ float4 als_smem[];
    float *lds = reinterpret_cast<float *>(als_smem);
    const int row = blockIdx.x;
    const int lo = a.indptr[row], hi = a.indptr[row + 1];
    if (hi <= lo) {
        if constexpr (K == AlsKind::Implicit) {
            float *y = a.p.Y + static_cast<size_t>(row) * a.p.ldy;
            for (int c = threadIdx.x; c < a.p.ldy; c += kAlsThreads) y[c] = 0.f;
            if (threadIdx.x == 0) a.p.yb[row] = 0.f;
        }
        return;
    }
    if (hi - lo > kAlsChunk) return;
    f32x16 acc[AlsShape<NT>::per_wave];
    seed_acc<NT, K>(a, acc);
    als_accumulate<NT, K>(a, lo, hi, acc, lds);
    als_solve<NT, K>(a, row, hi - lo, acc, lds);
}

// one chunk of a long row (AlsKind::Gram: one tile of kAlsChunk partner rows): its partial Gram to the batch workspace, lane-major
// (coalesced)
template <int NT, AlsKind K>
__global__ __launch_bounds__(kAlsThreads) void als_chunk_kernel(AlsArgs a) {
    extern __shared__ float4 als_smem[];
    float *lds = reinterpret_cast<float *>(als_smem);
    constexpr int pairs = AlsShape<NT>::pairs;
    const int c = a.chunk0 + blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lo = K == AlsKind::Gram ? c * kAlsChunk : a.chunk_lo[c];
    const int hi = K == AlsKind::Gram ? min(lo + kAlsChunk, a.p.x_rows) : a.chunk_hi[c];
    f32x16 acc[AlsShape<NT>::per_wave];
    zero_acc<NT>(acc);
    als_accumulate<NT, K>(a, lo, hi, acc, lds);
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

// a long row: its chunks' partial Grams summed in chunk order (AlsKind::Implicit: onto G0), then the solve
template <int NT, AlsKind K>
__global__ __launch_bounds__(kAlsThreads) void als_long_kernel(AlsArgs a) {
    extern __shared__ float4 als_smem[];
    float *lds = reinterpret_cast<float *>(als_smem);
    constexpr size_t gram_floats = static_cast<size_t>(AlsShape<NT>::pairs) * 16 * 64;
    const int lr = a.row0 + blockIdx.x, row = a.long_rows[lr];
    const int c_begin = a.long_first_chunk[lr] - a.chunk0, c_end = a.long_first_chunk[lr + 1] - a.chunk0;
    f32x16 acc[AlsShape<NT>::per_wave];
    seed_acc<NT, K>(a, acc);
    for (int c = c_begin; c < c_end; ++c) add_gram<NT>(acc, a.ws + c * gram_floats);
    als_solve<NT, K>(a, row, a.indptr[row + 1] - a.indptr[row], acc, lds);
}

// G0: the tiles' partial Grams added in tile order, element by element; `first`: the first batch of tiles starts from zero
__global__ void als_gram_sum_kernel(const float *__restrict__ ws, int tiles, size_t gram_floats, float *__restrict__ g0, int first) {
    const size_t e = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= gram_floats) return;
    float s = first ? 0.f : g0[e];
    for (int t = 0; t < tiles; ++t) s = s + ws[t * gram_floats + e];
    g0[e] = s;
}

void ensure_workspace(AlsCache &c, size_t floats) {
    if (c.workspace.count < floats) c.workspace.allocate(floats);
}

// out = X^T X over rows [0, n) of X in the accumulator layout of NT tiles, through the workspace in batches of whole tiles
template <int NT>
void run_global_gram(AlsCache &c, const float *X, int ldx, int n, int n_factors, DeviceBuffer<float> &out, hipStream_t stream) {
    constexpr size_t gram_floats = static_cast<size_t>(AlsShape<NT>::pairs) * 16 * 64;
    const size_t stage_bytes = static_cast<size_t>(kAlsStep) * AlsShape<NT>::C * sizeof(float);
    if (out.count < gram_floats) out.allocate(gram_floats);
    const int tiles = (n + kAlsChunk - 1) / kAlsChunk;
    if (tiles == 0) {
        CU2REC_HIP(hipMemsetAsync(out.ptr, 0, gram_floats * sizeof(float), stream));
        return;
    }
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_chunk_kernel<NT, AlsKind::Gram>), kMaxLds);
    const int batch_tiles = static_cast<int>(kAlsWorkspaceBytes / (gram_floats * sizeof(float)));
    ensure_workspace(c, std::min(batch_tiles, tiles) * gram_floats);
    AlsArgs a{};
    a.p.X = X;
    a.p.ldx = ldx;
    a.p.n_factors = n_factors;
    a.p.x_rows = n;
    a.ws = c.workspace.ptr;
    const int sum_threads = 256, sum_blocks = static_cast<int>((gram_floats + sum_threads - 1) / sum_threads);
    for (int t0 = 0; t0 < tiles; t0 += batch_tiles) {
        const int nt = std::min(batch_tiles, tiles - t0);
        a.chunk0 = t0;
        hipLaunchKernelGGL((als_chunk_kernel<NT, AlsKind::Gram>), dim3(nt), dim3(kAlsThreads), stage_bytes, stream, a);
        CU2REC_HIP(hipGetLastError());
        hipLaunchKernelGGL(als_gram_sum_kernel, dim3(sum_blocks), dim3(sum_threads), 0, stream, c.workspace.ptr, nt, gram_floats, out.ptr,
                           t0 == 0 ? 1 : 0);
        CU2REC_HIP(hipGetLastError());
    }
}

template <int NT, AlsKind K>
int run_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream, int cg_steps = 0) {
    constexpr int pairs = AlsShape<NT>::pairs;
    constexpr int operands = K == AlsKind::Implicit ? 2 : 1;
    const size_t stage_bytes = static_cast<size_t>(operands) * kAlsStep * AlsShape<NT>::C * sizeof(float);
    const size_t solve_bytes = (solve_lds_floats(p.n_factors) * sizeof(float) + 15) & ~static_cast<size_t>(15);
    const size_t short_bytes = std::max(stage_bytes, solve_bytes);
    if (short_bytes > kMaxLds)
        fail(CU2REC_EUNSUPPORTED, std::string(K == AlsKind::Implicit ? "cu2rec_model_als_implicit" : "cu2rec_model_als") +
                                      ": n_factors too large for the LDS of one workgroup");
    if (cg_steps <= 0) ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_short_kernel<NT, K>), kMaxLds);
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_chunk_kernel<NT, K>), kMaxLds);
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_long_kernel<NT, K>), kMaxLds);
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
    if constexpr (K == AlsKind::Implicit) {  // once per half-step, before the workspace holds the long rows' chunks
        run_global_gram<NT>(c, p.X, p.ldx, p.x_rows, p.n_factors, c.g0, stream);
        a.g0 = c.g0.ptr;
    }
    const int grid = std::min(side.rows, max_rows);
    if (cg_steps > 0) {  // the short rows by conjugate gradients (als_cg.hip); the long rows as always
        if constexpr (K == AlsKind::Implicit) ials_cg_short_rows(c, side, p, max_rows, cg_steps, stream);
        else als_cg_short_rows(c, side, p, max_rows, cg_steps, stream);
    } else if (grid > 0)
        hipLaunchKernelGGL((als_short_kernel<NT, K>), dim3(grid), dim3(kAlsThreads), short_bytes, stream, a);
    CU2REC_HIP(hipGetLastError());
    const int L = static_cast<int>(side.long_rows.size());
    if (L > 0) {
        // batches of whole rows whose partial Grams fit the workspace (at least kAlsMaxChunks: any one row)
        const size_t gram_floats = static_cast<size_t>(pairs) * 16 * 64;
        const int batch_chunks = static_cast<int>(kAlsWorkspaceBytes / (gram_floats * sizeof(float)));
        static_assert(kAlsWorkspaceBytes / (36 * 16 * 64 * sizeof(float)) >= kAlsMaxChunks, "workspace below one row's chunks");
        const int needed = std::min(batch_chunks, side.long_first_chunk[L]);
        ensure_workspace(c, needed * gram_floats);
        a.ws = c.workspace.ptr;
        for (int r = 0; r < L;) {
            const int c0 = side.long_first_chunk[r];
            int r1 = r + 1;
            while (r1 < L && side.long_first_chunk[r1 + 1] - c0 <= batch_chunks) ++r1;
            a.chunk0 = c0;
            a.row0 = r;
            hipLaunchKernelGGL((als_chunk_kernel<NT, K>), dim3(side.long_first_chunk[r1] - c0), dim3(kAlsThreads), stage_bytes, stream, a);
            CU2REC_HIP(hipGetLastError());
            hipLaunchKernelGGL((als_long_kernel<NT, K>), dim3(r1 - r), dim3(kAlsThreads), solve_bytes, stream, a);
            CU2REC_HIP(hipGetLastError());
            r = r1;
        }
    }
    int unsolved = 0;
    CU2REC_HIP(hipMemcpyAsync(&unsolved, c.unsolved.ptr, sizeof(int), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    return unsolved;
}

// ---- the implicit objective ----------------------------------------------------------------------------------------------
struct IalsObjectiveArgs {
    const int *indptr, *indices;
    const float *data;
    const float *P, *Q;
    int ldp, ldq, rows, cols, nnz, n_factors;
    float alpha;
    double *partials;  // [blocks][3]: entries term, sum |p_u|^2, sum |q_i|^2
};

// one pass over the entries and the rows of both sides, a 16-lane group per entry / row, sums in double; per-block partials
__global__ __launch_bounds__(kObjThreads) void ials_objective_kernel(IalsObjectiveArgs a) {
    __shared__ double red[3][kObjThreads];
    const int tid = threadIdx.x, lane16 = tid & (kObjGroup - 1);
    const int group = (blockIdx.x * kObjThreads + tid) / kObjGroup, groups = gridDim.x * (kObjThreads / kObjGroup);
    double s_e = 0.0, s_p = 0.0, s_q = 0.0;
    for (int k = group; k < a.nnz; k += groups) {
        const int u = row_of_entry(a.indptr, a.rows, k);
        const double s = group_dot(a.P + static_cast<size_t>(u) * a.ldp, a.Q + static_cast<size_t>(a.indices[k]) * a.ldq, a.n_factors, lane16);
        const double w = static_cast<double>(a.alpha * a.data[k]);
        if (lane16 == 0) s_e += w * (1.0 - s) * (1.0 - s) + 1.0 - 2.0 * s;
    }
    for (int u = group; u < a.rows; u += groups) {
        const float *x = a.P + static_cast<size_t>(u) * a.ldp;
        const double n2 = group_dot(x, x, a.n_factors, lane16);
        if (lane16 == 0) s_p += n2;
    }
    for (int i = group; i < a.cols; i += groups) {
        const float *x = a.Q + static_cast<size_t>(i) * a.ldq;
        const double n2 = group_dot(x, x, a.n_factors, lane16);
        if (lane16 == 0) s_q += n2;
    }
    const double sums[3] = {s_e, s_p, s_q};
    block_reduce(sums, red);
    if (tid == 0)
        for (int j = 0; j < 3; ++j) a.partials[3 * blockIdx.x + j] = red[j][0];
}

// out[0..2] = the block partials added in block order; out[3] = <G_P, G_Q> over the full symmetric matrices: the Grams hold the
// tile pairs ti >= tj as whole 32 x 32 tiles, so an off-diagonal pair counts twice.  One workgroup, fixed order.
__global__ __launch_bounds__(kObjThreads) void ials_objective_reduce_kernel(const double *__restrict__ partials, int blocks,
                                                                            const float *__restrict__ gp, const float *__restrict__ gq,
                                                                            int pairs, double *__restrict__ out) {
    __shared__ double red[4][kObjThreads];
    const int tid = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < blocks; b += kObjThreads)
        for (int j = 0; j < 3; ++j) s[j] += partials[3 * b + j];
    for (int e = tid; e < pairs * 16 * 64; e += kObjThreads) {
        int ti, tj;
        pair_tiles(e / (16 * 64), ti, tj);
        s[3] += (ti == tj ? 1.0 : 2.0) * (static_cast<double>(gp[e]) * static_cast<double>(gq[e]));
    }
    block_reduce(s, red);
    if (tid == 0)
        for (int j = 0; j < 4; ++j) out[j] = red[j][0];
}

}  // namespace

void als_plan_side(AlsSide &side, hipStream_t stream) {
    std::vector<int> indptr(static_cast<size_t>(side.rows) + 1);
    CU2REC_HIP(hipMemcpyAsync(indptr.data(), side.indptr, indptr.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    std::vector<int> lo, hi;
    side.long_rows.clear();
    side.long_first_chunk.assign(1, 0);
    side.rows_with_ratings = 0;
    for (int r = 0; r < side.rows; ++r) {
        const int n = indptr[r + 1] - indptr[r];
        side.rows_with_ratings += n > 0;
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
    side.planned = true;
}

int als_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream, int cg_steps) {
    const int nt = (p.n_factors + 2 + 31) / 32;  // columns f + 2: factors, the 1, t
    return dispatch_1_to_8(nt, "cu2rec_model_als: n_factors above 252 is not supported",
                           [&](auto tiles) { return run_half_step<tiles(), AlsKind::Explicit>(c, side, p, max_rows, stream, cg_steps); });
}

int ials_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream, int cg_steps) {
    return dispatch_1_to_8(ials_tiles(p.n_factors), "cu2rec_model_als_implicit: n_factors above 252 is not supported",
                           [&](auto tiles) { return run_half_step<tiles(), AlsKind::Implicit>(c, side, p, max_rows, stream, cg_steps); });
}

void als_global_gram(AlsCache &c, const float *X, int ldx, int n, int f, DeviceBuffer<float> &out, hipStream_t stream) {
    dispatch_1_to_8((f + 31) / 32, "n_factors above 252 is not supported",
                    [&](auto tiles) { run_global_gram<tiles()>(c, X, ldx, n, f, out, stream); });
}

double ials_objective(AlsCache &c, const AlsObjectiveProblem &o, hipStream_t stream) {
    const int nt = ials_tiles(o.n_factors);
    dispatch_1_to_8(nt, "cu2rec_model_implicit_objective: n_factors above 252 is not supported", [&](auto tiles) {
        run_global_gram<tiles()>(c, o.P, o.ldp, o.rows, o.n_factors, c.g0, stream);
        run_global_gram<tiles()>(c, o.Q, o.ldq, o.cols, o.n_factors, c.g0_other, stream);
    });
    const int blocks = objective_blocks(static_cast<size_t>(std::max(o.nnz, std::max(o.rows, o.cols))));
    if (c.objective.count < 3 * static_cast<size_t>(kObjMaxBlocks) + 4) c.objective.allocate(3 * static_cast<size_t>(kObjMaxBlocks) + 4);
    IalsObjectiveArgs a{o.indptr, o.indices, o.data, o.P, o.Q, o.ldp, o.ldq, o.rows, o.cols, o.nnz, o.n_factors, o.alpha, c.objective.ptr};
    hipLaunchKernelGGL(ials_objective_kernel, dim3(blocks), dim3(kObjThreads), 0, stream, a);
    CU2REC_HIP(hipGetLastError());
    double *out = c.objective.ptr + 3 * static_cast<size_t>(kObjMaxBlocks);
    hipLaunchKernelGGL(ials_objective_reduce_kernel, dim3(1), dim3(kObjThreads), 0, stream, c.objective.ptr, blocks, c.g0.ptr, c.g0_other.ptr,
                       tri(nt), out);
    CU2REC_HIP(hipGetLastError());
    double sums[4];
    CU2REC_HIP(hipMemcpyAsync(sums, out, sizeof(sums), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    return 0.5 * (sums[3] + sums[0] + static_cast<double>(o.P_reg) * sums[1] + static_cast<double>(o.Q_reg) * sums[2]);
}

}  // namespace cu2rec
