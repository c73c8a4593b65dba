// EASE (include/cu2rec_amd.h: cu2rec_ease_*): B from the dense inverse of the regularised Gram matrix, in five stages that all run in
// ONE ld x ld float buffer (ld = items rounded up to whole blocks of nb = kEaseBlock; the padding is an identity block, so every tile
// below is a whole nb x nb tile and no tile kernel checks a bound).
//
//   1 Gram      ease_gram_kernel: one wavefront per (item i, slice of kKnnSliceItems ids) -- knn_product_kernel's walk over the users of
//               column i with the selection removed: the slice of row i of G, dense, l2 added to the finished diagonal sum.
//   2 Cholesky  right-looking over block columns kb: ease_potrf_kernel factorises the diagonal tile in LDS (one workgroup),
//               ease_trsm_kernel solves one panel tile per workgroup (a thread per row), ease_syrk_kernel takes L21 L21^T off the
//               lower-triangle tiles of the trailing matrix on v_mfma_f32_32x32x2_f32 (a wavefront per 32 x 32 quarter).
//   3 L^-1      block columns from the last to the first: ease_trtri_kernel inverts the diagonal tile in LDS, the column's panel is
//               copied aside (the O(items x nb) workspace) and ease_trtri_panel_kernel forms -(W22 L21) W11 tile by tile on MFMA.
//   4 P         block rows from the first to the last: ease_lauum_kernel forms the row's tiles of L^-T L^-1 on MFMA (the row's
//               diagonal tile copied aside first: every tile of the row reads it, one overwrites it); ease_mirror_kernel fills the
//               upper triangle.
//   5 B         ease_diag_kernel keeps P's diagonal aside, ease_weights_kernel scales in place.
//
// Every sum is an fmaf or MFMA chain (bitwise the same thing) in an order fixed by the indices alone -- a tile product from zero, the
// products of successive tiles added one after the other -- with no float atomics.  A pivot that is not a finite number above the
// rounding noise of its diagonal entry is written with its index to a device flag by the one workgroup that meets it; every later
// launch of the build returns at once, and the host reads the flag when the stream has drained.
//
// The lists: ease_score_kernel, one wavefront per (query, slice), folds r * B[i, slice] for the query's entries in ascending id --
// each B row segment one coalesced read -- into LDS, clears the excluded ids from a bitmap of ALL the slice's ids and keeps the best
// 256 keys of select.hpp; ease_merge_kernel folds a query's slices.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "device.hpp"
#include "ease.hpp"
#include "ease_tile.hpp"
#include "hip_check.hpp"
#include "mfma_f32.hpp"
#include "rank_stage.hpp"
#include "rocprim_temp.hpp"
#include "select.hpp"

namespace cu2rec {

namespace {

constexpr int kSlice = kKnnSliceItems;
constexpr int kSliceWords = kSlice / 32;
constexpr int kChunk = 256;  // candidates that enter one sort beside the best 256 so far
constexpr float kPivotNoise = 0x1p-22f;
static_assert(kSliceWords == 64 && kSlice % kChunk == 0 && kSlice % kNb == 0, "one bitmap word per lane; whole chunks; whole blocks");

// the wavefront's LDS accesses before this point are done before those after it
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int first_not_below(const int *__restrict__ a, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- 1: the Gram matrix ------------------------------------------------------------------------------------------------------
struct EaseGram {
    const int *t_indptr, *t_users;  // the item-major view: column i's users are positions [t_indptr[i], t_indptr[i + 1])
    const float *t_data;
    const int *indptr, *s_idx;  // the row-sorted view: user u's ascending columns are positions [indptr[u], indptr[u + 1])
    const float *s_val;
    int items, ld, n_slices;
    float l2;
};

// wavefront w of the grid = (row w / n_slices of the padded matrix, slice w % n_slices) -> g[row][slice]
__global__ __launch_bounds__(256) void ease_gram_kernel(EaseGram a, float *__restrict__ g) {
    __shared__ float acc_s[4][kSlice];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + wave;
    if (w >= a.ld * a.n_slices) return;  // no workgroup-wide barrier below: the wavefronts are independent
    float *acc = acc_s[wave];
    const int i = w / a.n_slices, slice = w % a.n_slices;
    const int slice_lo = slice * kSlice, slice_hi = min(slice_lo + kSlice, a.ld);
    for (int j = lane; j < kSlice; j += 64) acc[j] = 0.f;
    wave_lds_sync();
    const int q_lo = i < a.items ? a.t_indptr[i] : 0, q_hi = i < a.items ? a.t_indptr[i + 1] : 0;
    for (int base = q_lo; base < q_hi; base += 64) {
        const int p = base + lane;
        int seg_lo = 0, seg_hi = 0;
        float alpha = 0.f;
        if (p < q_hi) {
            const int u = a.t_users[p];
            const int lo = a.indptr[u], hi = a.indptr[u + 1];
            alpha = a.t_data[p];
            seg_lo = first_not_below(a.s_idx, lo, hi, slice_lo);
            seg_hi = first_not_below(a.s_idx, seg_lo, hi, slice_hi);
        }
        unsigned long long live = __ballot(seg_hi > seg_lo);
        while (live) {  // user after user, in ascending order
            const int t = __ffsll(static_cast<long long>(live)) - 1;
            live &= live - 1;
            const int lo = __shfl(seg_lo, t), hi = __shfl(seg_hi, t);
            const float al = __shfl(alpha, t);
            for (int e = lo + lane; e < hi; e += 64) {  // distinct ids within one row
                const int j = a.s_idx[e] - slice_lo;
                acc[j] = fmaf(al, a.s_val[e], acc[j]);
            }
            wave_lds_sync();
        }
    }
    float *row = g + static_cast<size_t>(i) * a.ld;
    for (int j = lane; j < slice_hi - slice_lo; j += 64) {
        float v = acc[j];
        if (slice_lo + j == i) v = i < a.items ? v + a.l2 : 1.f;
        row[slice_lo + j] = v;
    }
}

// ---- 2: the Cholesky factor --------------------------------------------------------------------------------------------------
// one workgroup: the diagonal tile kb, right-looking column by column in LDS; written back with zeros above the diagonal
// g0: the diagonal of G before the factorisation.  A pivot must be finite and above the rounding noise of its own diagonal entry,
// 4 x 2^-24 x G_jj: G_jj = fl(sum + l2) is itself known to half an ulp, and the squares taken off it are rounded ones
__global__ __launch_bounds__(256) void ease_potrf_kernel(float *__restrict__ g, int ld, int kb, const float *__restrict__ g0,
                                                         int *__restrict__ flag) {
    __shared__ float t[kNb][kLs];
    if (flag[0]) return;
    float *a = tile_at(g, ld, kb, kb);
    load_tile(t, a, ld, 256);
    __syncthreads();
    for (int j = 0; j < kNb; ++j) {
        const float d = t[j][j];  // the same value in every thread: the branch is the workgroup's
        if (!(d > 0.f) || !(d > kPivotNoise * g0[kb * kNb + j]) || !(d <= 3.402823466e+38f)) {
            if (threadIdx.x == 0) {
                flag[1] = kb * kNb + j;
                flag[0] = 1;
            }
            return;
        }
        const float l = sqrtf(d);
        __syncthreads();  // every thread has read d
        const int i = threadIdx.x;
        if (i == j) t[j][j] = l;
        else if (i > j && i < kNb) t[i][j] = t[i][j] / l;
        __syncthreads();
        for (int x = threadIdx.x; x < kNb * kNb; x += 256) {
            const int r = x >> 6, c = x & 63;
            if (c > j && r >= c) t[r][c] = fmaf(-t[r][j], t[c][j], t[r][c]);
        }
        __syncthreads();
    }
    for (int x = threadIdx.x; x < kNb * kNb; x += 256) {
        const int r = x >> 6, c = x & 63;
        a[static_cast<size_t>(r) * ld + c] = c <= r ? t[r][c] : 0.f;
    }
}

// workgroup b (one wavefront): the panel tile (kb + 1 + b, kb) <- A L_kk^-T; thread r substitutes forward along row r
__global__ __launch_bounds__(64) void ease_trsm_kernel(float *__restrict__ g, int ld, int kb, const int *__restrict__ flag) {
    __shared__ float l[kNb][kLs], x[kNb][kLs];
    if (flag[0]) return;
    float *a = tile_at(g, ld, kb + 1 + blockIdx.x, kb);
    load_tile(l, tile_at(g, ld, kb, kb), ld, 64);
    load_tile(x, a, ld, 64);
    __syncthreads();
    const int r = threadIdx.x;
    for (int j = 0; j < kNb; ++j) {
        float s = x[r][j];
        for (int c = 0; c < j; ++c) s = fmaf(-x[r][c], l[j][c], s);
        x[r][j] = s / l[j][j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kNb * kNb; e += 64) a[static_cast<size_t>(e >> 6) * ld + (e & 63)] = x[e >> 6][e & 63];
}

// workgroup (bx, by): the trailing tile (bi, bj) = (kb + 1 + by, kb + 1 + bx), bj <= bi, -= L[bi, kb] L[bj, kb]^T
__global__ __launch_bounds__(256) void ease_syrk_kernel(float *__restrict__ g, int ld, int kb, const int *__restrict__ flag) {
    __shared__ float li[kNb][kLs], lj[kNb][kLs];
    if (blockIdx.x > blockIdx.y || flag[0]) return;
    const int bi = kb + 1 + blockIdx.y, bj = kb + 1 + blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wi = wave >> 1, wj = wave & 1;
    load_tile(li, tile_at(g, ld, bi, kb), ld, 256);
    load_tile(lj, tile_at(g, ld, bj, kb), ld, 256);
    __syncthreads();
    f32x16 part = zero_tile();
    tile_mma<false, true, false>(part, li, lj, wi, wj, lane);
    float *c = tile_at(g, ld, bi, bj);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        float *at = c + static_cast<size_t>(wi * 32 + acc_row(reg, lane >> 5)) * ld + wj * 32 + (lane & 31);
        *at = *at - part[reg];
    }
}

// ---- 3: the inverse of the factor --------------------------------------------------------------------------------------------
// one workgroup (one wavefront): the diagonal tile j <- its inverse; thread c solves column c; zeros above the diagonal
__global__ __launch_bounds__(64) void ease_trtri_kernel(float *__restrict__ g, int ld, int j, const int *__restrict__ flag) {
    __shared__ float l[kNb][kLs], x[kNb][kLs];
    if (flag[0]) return;
    float *a = tile_at(g, ld, j, j);
    load_tile(l, a, ld, 64);
    __syncthreads();
    const int c = threadIdx.x;
    for (int i = 0; i < c; ++i) x[i][c] = 0.f;
    x[c][c] = 1.f / l[c][c];
    for (int i = c + 1; i < kNb; ++i) {
        float s = 0.f;
        for (int k = c; k < i; ++k) s = fmaf(l[i][k], x[k][c], s);
        x[i][c] = -s / l[i][i];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kNb * kNb; e += 64) a[static_cast<size_t>(e >> 6) * ld + (e & 63)] = x[e >> 6][e & 63];
}

// rows x kNb floats of row stride ld -> dst, dense
__global__ void ease_copy_panel_kernel(const float *__restrict__ src, int ld, int rows, float *__restrict__ dst, const int *__restrict__ flag) {
    if (flag[0]) return;
    const size_t total = static_cast<size_t>(rows) * kNb;
    for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += static_cast<size_t>(gridDim.x) * blockDim.x)
        dst[t] = src[(t >> 6) * ld + (t & 63)];
}

// workgroup b: the tile (bi, j), bi = j + 1 + b, <- -(sum_{c = j + 1 .. bi} W[bi, c] L[c, j]) W[j, j]; panel: L[j + 1 .., j], copied aside
__global__ __launch_bounds__(256) void ease_trtri_panel_kernel(float *__restrict__ g, int ld, int j, const float *__restrict__ panel,
                                                               const int *__restrict__ flag) {
    __shared__ float x[kNb][kLs], y[kNb][kLs];
    if (flag[0]) return;
    const int bi = j + 1 + blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wi = wave >> 1, wj = wave & 1;
    f32x16 acc = zero_tile();
    for (int c = j + 1; c <= bi; ++c) {
        __syncthreads();  // the tiles of the step before have been read
        load_tile(x, tile_at(g, ld, bi, c), ld, 256);
        load_tile(y, panel + static_cast<size_t>(c - j - 1) * kNb * kNb, kNb, 256);
        __syncthreads();
        f32x16 part = zero_tile();
        tile_mma<false, false, false>(part, x, y, wi, wj, lane);
        acc += part;
    }
    __syncthreads();
    store_quarter(acc, &x[0][0], kLs, wi, wj, lane);
    load_tile(y, tile_at(g, ld, j, j), ld, 256);
    __syncthreads();
    acc = zero_tile();
    tile_mma<false, false, true>(acc, x, y, wi, wj, lane);
    store_quarter(acc, tile_at(g, ld, bi, j), ld, wi, wj, lane);
}

// ---- 4: P = W^T W ------------------------------------------------------------------------------------------------------------
// workgroup y: the tile (r, y), y <= r, <- sum_{c = r .. T - 1} W[c, r]^T W[c, y]; diag: W[r, r], copied aside
__global__ __launch_bounds__(256) void ease_lauum_kernel(float *__restrict__ g, int ld, int r, int n_tiles, const float *__restrict__ diag,
                                                         const int *__restrict__ flag) {
    __shared__ float x[kNb][kLs], yt[kNb][kLs];
    if (flag[0]) return;
    const int y = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wi = wave >> 1, wj = wave & 1;
    f32x16 acc = zero_tile();
    for (int c = r; c < n_tiles; ++c) {
        __syncthreads();
        if (c == r) load_tile(x, diag, kNb, 256);
        else load_tile(x, tile_at(g, ld, c, r), ld, 256);
        if (c == r && y == r) load_tile(yt, diag, kNb, 256);
        else load_tile(yt, tile_at(g, ld, c, y), ld, 256);
        __syncthreads();
        f32x16 part = zero_tile();
        tile_mma<true, false, false>(part, x, yt, wi, wj, lane);
        acc += part;
    }
    store_quarter(acc, tile_at(g, ld, r, y), ld, wi, wj, lane);
}

// workgroup (bx, by), bx < by: the tile (bx, by) <- the transpose of the tile (by, bx)
__global__ __launch_bounds__(256) void ease_mirror_kernel(float *__restrict__ g, int ld, const int *__restrict__ flag) {
    __shared__ float t[kNb][kLs];
    if (blockIdx.x >= blockIdx.y || flag[0]) return;
    load_tile(t, tile_at(g, ld, blockIdx.y, blockIdx.x), ld, 256);
    __syncthreads();
    float *dst = tile_at(g, ld, blockIdx.x, blockIdx.y);
    for (int x = threadIdx.x; x < kNb * kNb; x += 256) dst[static_cast<size_t>(x >> 6) * ld + (x & 63)] = t[x & 63][x >> 6];
}

// ---- 5: the weights ----------------------------------------------------------------------------------------------------------
__global__ void ease_diag_kernel(const float *__restrict__ g, int ld, float *__restrict__ d, const int *__restrict__ flag) {
    if (flag[0]) return;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ld; j += gridDim.x * blockDim.x) d[j] = g[static_cast<size_t>(j) * ld + j];
}

__global__ void ease_weights_kernel(float *__restrict__ g, int ld, const float *__restrict__ d, const int *__restrict__ flag) {
    if (flag[0]) return;
    const size_t total = static_cast<size_t>(ld) * ld;
    for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const size_t i = t / ld, j = t % ld;
        g[t] = i == j ? 0.f : -g[t] / d[j];
    }
}

// ---- the lists ---------------------------------------------------------------------------------------------------------------
struct EaseQuery {
    const int *q_begin, *q_end;  // query id q's entries: positions [q_begin[q], q_end[q]) of
    const int *q_idx;            //   the item ids, ascending (null: the one entry (q, 1.0f), and q is not its own candidate)
    const float *q_val;          //   and their values
    const int *ex_indptr, *ex_indices;  // exclusions by query id (null: none); rows past ex_rows exclude nothing
    int ex_rows;
    const float *B;
    int ld, n_cand, n_slices, k;
};

// wavefront w of the grid = (query position w / n_slices, slice w % n_slices) -> cand[w][k]: the slice's best k keys, best first
__global__ __launch_bounds__(256) void ease_score_kernel(EaseQuery a, const int *__restrict__ qids, int n_pos,
                                                         unsigned long long *__restrict__ cand) {
    __shared__ float acc_s[4][kSlice];
    __shared__ unsigned bits_s[4][kSliceWords];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + wave;
    if (w >= n_pos * a.n_slices) return;  // no workgroup-wide barrier below: the wavefronts are independent
    float *acc = acc_s[wave];
    unsigned *bits = bits_s[wave];
    const int pos = w / a.n_slices, slice = w % a.n_slices;
    const int q = qids[pos];
    const int slice_lo = slice * kSlice, slice_hi = min(slice_lo + kSlice, a.n_cand);
    const int width = max(slice_hi - slice_lo, 0);
    for (int j = lane; j < kSlice; j += 64) acc[j] = 0.f;
    const int have = width - lane * 32;  // every id of the slice is a candidate
    bits[lane] = have >= 32 ? 0xFFFFFFFFu : have > 0 ? (1u << have) - 1u : 0u;
    wave_lds_sync();
    const int e_lo = a.q_idx ? a.q_begin[q] : 0, e_hi = a.q_idx ? a.q_end[q] : 1;
    for (int e = e_lo; e < e_hi; ++e) {  // entry after entry, in ascending id order
        const int i = a.q_idx ? a.q_idx[e] : q;
        const float r = a.q_idx ? a.q_val[e] : 1.f;
        const float *row = a.B + static_cast<size_t>(i) * a.ld + slice_lo;
        for (int j = lane; j < width; j += 64) acc[j] = fmaf(r, row[j], acc[j]);
    }
    if (a.ex_indptr && q < a.ex_rows) {
        for (int e = a.ex_indptr[q] + lane; e < a.ex_indptr[q + 1]; e += 64) {
            const int it = a.ex_indices[e];
            if (it >= slice_lo && it < slice_hi) atomicAnd(&bits[(it - slice_lo) >> 5], ~(1u << ((it - slice_lo) & 31)));
        }
    }
    if (!a.q_idx && lane == 0 && q >= slice_lo && q < slice_hi) atomicAnd(&bits[(q - slice_lo) >> 5], ~(1u << ((q - slice_lo) & 31)));
    wave_lds_sync();
    unsigned long long v[8];  // slots 0 .. 255: the best so far, best first; slots 256 .. 511: the next chunk's candidates
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0ull;
    for (int c = 0; c * kChunk < width; ++c) {
        unsigned word[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            word[e] = bits[c * (kChunk / 32) + e * 2 + (lane >> 5)];
            any = any || word[e] != 0u;
        }
        if (!__any(any)) continue;  // the whole chunk is excluded
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = c * kChunk + e * 64 + lane;
            v[4 + e] = (word[e] >> (lane & 31)) & 1u ? topk_key(acc[j], slice_lo + j) : 0ull;
        }
        wave_sort_desc<8>(v, lane);
    }
    unsigned long long *out = cand + static_cast<size_t>(w) * a.k;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e * 64 + lane < a.k) out[e * 64 + lane] = v[e];
}

// one wavefront per query position: the slices' lists folded into the best k -> ids_out / vals_out [n_pos][k]
__global__ __launch_bounds__(256) void ease_merge_kernel(const unsigned long long *__restrict__ cand, int n_pos, int n_slices, int k,
                                                         int *__restrict__ ids_out, float *__restrict__ vals_out) {
    const int lane = threadIdx.x & 63;
    const int pos = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= n_pos) return;
    unsigned long long v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0ull;
    for (int s = 0; s < n_slices; ++s) {
        const unsigned long long *in = cand + (static_cast<size_t>(pos) * n_slices + s) * k;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 + e] = e * 64 + lane < k ? in[e * 64 + lane] : 0ull;
        wave_sort_desc<8>(v, lane);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = e * 64 + lane;
        if (j >= k) continue;
        int it;
        float sc;
        topk_decode(v[e], it, sc);
        ids_out[static_cast<size_t>(pos) * k + j] = it;
        vals_out[static_cast<size_t>(pos) * k + j] = sc;
    }
}

// The lists of a set of queries, in batches over a bounded workspace.
struct ListRunner {
    ListRunner(const EaseQuery &a_, int n_total) : a(a_) {
        const size_t per_query = (static_cast<size_t>(a.n_slices) + 1) * a.k * 8;  // the slices' keys and the list itself
        batch = static_cast<int>(std::min<size_t>(std::max<size_t>(1, kEaseWorkspaceBytes / per_query), std::max(n_total, 1)));
        cand.allocate(static_cast<size_t>(batch) * a.n_slices * a.k);
    }
    // query positions qids[0 .. n) -> ids_out / vals_out [n][k] (device)
    void run(const int *qids, int n, int *ids_out, float *vals_out, hipStream_t stream) {
        const int waves = n * a.n_slices;
        hipLaunchKernelGGL(ease_score_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, a, qids, n, cand.ptr);
        hipLaunchKernelGGL(ease_merge_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, cand.ptr, n, a.n_slices, a.k, ids_out, vals_out);
        CU2REC_HIP(hipGetLastError());
    }
    // the lists of host query ids q into host out_ids / out_vals [q.size()][k], batch after batch
    void run_to_host(const std::vector<int> &q, int *out_ids, float *out_vals, hipStream_t stream) {
        const int n = static_cast<int>(q.size()), k = a.k;
        DeviceBuffer<int> d_q(q.size()), d_ids(static_cast<size_t>(batch) * k);
        DeviceBuffer<float> d_vals(static_cast<size_t>(batch) * k);
        d_q.upload(q.data(), q.size());
        for (int p0 = 0; p0 < n; p0 += batch) {
            const int b = std::min(batch, n - p0);
            run(d_q.ptr + p0, b, d_ids.ptr, d_vals.ptr, stream);
            CU2REC_HIP(hipMemcpyAsync(out_ids + static_cast<size_t>(p0) * k, d_ids.ptr, static_cast<size_t>(b) * k * sizeof(int),
                                      hipMemcpyDeviceToHost, stream));
            CU2REC_HIP(hipMemcpyAsync(out_vals + static_cast<size_t>(p0) * k, d_vals.ptr, static_cast<size_t>(b) * k * sizeof(float),
                                      hipMemcpyDeviceToHost, stream));
        }  // stream order: a batch's copies are done before the next batch overwrites the workspace
        CU2REC_HIP(hipStreamSynchronize(stream));
    }
    const EaseQuery a;
    int batch;
    DeviceBuffer<unsigned long long> cand;
};

int slices_of(int n) { return std::max(1, (n + kSlice - 1) / kSlice); }

// the ids of a query list: `ids` (validated against rows) or, when null, every row
std::vector<int> query_ids(const int *ids, int n_ids, int rows, const char *who) {
    const int n = ids ? n_ids : rows;
    require(n >= 0, who);
    std::vector<int> out(n);
    for (int i = 0; i < n; ++i) {
        out[i] = ids ? ids[i] : i;
        require(out[i] >= 0 && out[i] < rows, who);
    }
    return out;
}

void check_k(const char *what, int k) { require(k >= 1 && k <= kEaseMaxK, what); }

void check_same_cols(const DeviceEase &m, const DeviceCsr *csr, const char *what) { require(!csr || csr->cols == m.items, what); }

// the lists of history rows: the row-sorted view's entries, every stored entry counted
EaseQuery recommend_query(const DeviceEase &m, const DeviceCsr &history, const DeviceCsr *exclude, int k, hipStream_t stream) {
    const RowSortedView &rows = row_sorted_view(history, true, stream);
    const bool ex = exclude && exclude->nnz > 0;
    return EaseQuery{history.indptr.ptr, history.indptr.ptr + 1, rows.idx.ptr, rows.val.ptr, ex ? exclude->indptr.ptr : nullptr,
                     ex ? exclude->indices.ptr : nullptr, ex ? exclude->rows : 0, m.B.ptr, m.ld, m.items, slices_of(m.items), k};
}

}  // namespace

int ease_padded(int items) { return (items + kNb - 1) / kNb * kNb; }

void ease_allocate_matrix(DeviceBuffer<float> &buf, size_t n, const char *fn) {
    if (n == 0) return;
    float *p = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(float));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        fail(CU2REC_ENOMEM, std::string(fn) + ": the " + std::to_string(n * sizeof(float)) + " bytes of the item x item matrix do not fit the device");
    }
    CU2REC_HIP(e);
    buf.ptr = p;
    buf.count = n;
}

void ease_check_l2(const char *fn, float l2) { Need{fn}(std::isfinite(l2) && l2 > 0.f, CU2REC_EINVAL, ": l2 must be finite and > 0"); }

void ease_gram(const DeviceCsr &csr, float l2, int ld, float *g, hipStream_t stream) {
    const RowSortedView &rows = row_sorted_view(csr, true, stream);
    if (rows.has_duplicate) fail(CU2REC_EINVAL, "cu2rec_ease: a row stores the same column twice");
    const ItemMajorView &view = item_major_view(csr, stream);
    const EaseGram a{view.indptr.ptr, view.indices.ptr, view.data.ptr, csr.indptr.ptr, rows.idx.ptr, rows.val.ptr, csr.cols, ld, slices_of(ld), l2};
    const long long waves = static_cast<long long>(ld) * a.n_slices;
    hipLaunchKernelGGL(ease_gram_kernel, dim3(static_cast<unsigned>((waves + 3) / 4)), dim3(256), 0, stream, a, g);
    CU2REC_HIP(hipGetLastError());
}

DeviceEase::DeviceEase(const DeviceCsr &train, float l2_) : items(train.cols), ld(ease_padded(train.cols)), l2(l2_) {
    ease_check_l2("cu2rec_ease_create", l2);
    if (items > kEaseMaxItems) fail(CU2REC_EUNSUPPORTED, "cu2rec_ease_create: more than CU2REC_EASE_MAX_ITEMS columns");
    if (items == 0) return;
    require_device();
    check_faults();
    hipStream_t stream = nullptr;
    const int T = ld / kNb;
    ease_allocate_matrix(B, static_cast<size_t>(ld) * ld, "cu2rec_ease_create");
    DeviceBuffer<float> panel(static_cast<size_t>(ld) * kNb), diag(ld);
    DeviceBuffer<int> flag(2);
    flag.zero();
    float *g = B.ptr;
    ease_gram(train, l2, ld, g, stream);
    hipLaunchKernelGGL(ease_diag_kernel, dim3(element_grid(static_cast<size_t>(ld))), dim3(256), 0, stream, g, ld, diag.ptr, flag.ptr);
    for (int kb = 0; kb < T; ++kb) {
        const int m = T - kb - 1;
        hipLaunchKernelGGL(ease_potrf_kernel, dim3(1), dim3(256), 0, stream, g, ld, kb, diag.ptr, flag.ptr);
        if (m == 0) break;
        hipLaunchKernelGGL(ease_trsm_kernel, dim3(m), dim3(64), 0, stream, g, ld, kb, flag.ptr);
        hipLaunchKernelGGL(ease_syrk_kernel, dim3(m, m), dim3(256), 0, stream, g, ld, kb, flag.ptr);
    }
    CU2REC_HIP(hipGetLastError());
    for (int j = T - 1; j >= 0; --j) {
        const int m = T - j - 1;
        hipLaunchKernelGGL(ease_trtri_kernel, dim3(1), dim3(64), 0, stream, g, ld, j, flag.ptr);
        if (m == 0) continue;
        const float *below = g + static_cast<size_t>(j + 1) * kNb * ld + static_cast<size_t>(j) * kNb;
        hipLaunchKernelGGL(ease_copy_panel_kernel, dim3(element_grid(static_cast<size_t>(m) * kNb * kNb)), dim3(256), 0, stream, below, ld,
                           m * kNb, panel.ptr, flag.ptr);
        hipLaunchKernelGGL(ease_trtri_panel_kernel, dim3(m), dim3(256), 0, stream, g, ld, j, panel.ptr, flag.ptr);
    }
    CU2REC_HIP(hipGetLastError());
    for (int r = 0; r < T; ++r) {
        hipLaunchKernelGGL(ease_copy_panel_kernel, dim3(element_grid(static_cast<size_t>(kNb) * kNb)), dim3(256), 0, stream,
                           g + static_cast<size_t>(r) * kNb * ld + static_cast<size_t>(r) * kNb, ld, kNb, panel.ptr, flag.ptr);
        hipLaunchKernelGGL(ease_lauum_kernel, dim3(r + 1), dim3(256), 0, stream, g, ld, r, T, panel.ptr, flag.ptr);
    }
    hipLaunchKernelGGL(ease_mirror_kernel, dim3(T, T), dim3(256), 0, stream, g, ld, flag.ptr);
    hipLaunchKernelGGL(ease_diag_kernel, dim3(element_grid(static_cast<size_t>(ld))), dim3(256), 0, stream, g, ld, diag.ptr, flag.ptr);
    hipLaunchKernelGGL(ease_weights_kernel, dim3(element_grid(static_cast<size_t>(ld) * ld)), dim3(256), 0, stream, g, ld, diag.ptr, flag.ptr);
    CU2REC_HIP(hipGetLastError());
    int h_flag[2] = {0, 0};
    CU2REC_HIP(hipMemcpyAsync(h_flag, flag.ptr, sizeof(h_flag), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));  // also before the temporaries are freed
    if (h_flag[0])
        fail(CU2REC_EUNSUPPORTED, "cu2rec_ease_create: the pivot of item " + std::to_string(h_flag[1]) +
                                      " is not a finite number above 2^-22 of its diagonal entry (not positive definite in float: raise l2)");
}

void DeviceEase::weights(const int *ids, int n, float *out) const {
    require(out, "cu2rec_ease_weights: null output");
    const std::vector<int> q = query_ids(ids, n, items, "cu2rec_ease_weights: item id out of range (or negative n)");
    if (q.empty()) return;
    require_device();
    const size_t row = static_cast<size_t>(items) * sizeof(float);
    if (!ids) {
        CU2REC_HIP(hipMemcpy2D(out, row, B.ptr, static_cast<size_t>(ld) * sizeof(float), row, items, hipMemcpyDeviceToHost));
        return;
    }
    for (size_t p = 0; p < q.size(); ++p)
        CU2REC_HIP(hipMemcpy(out + p * items, B.ptr + static_cast<size_t>(q[p]) * ld, row, hipMemcpyDeviceToHost));
}

void DeviceEase::neighbors(const int *ids_in, int n_ids, int k, int *out_ids, float *out_vals) const {
    check_k("cu2rec_ease_neighbors: k must be in [1, 256]", k);
    require(out_ids && out_vals, "cu2rec_ease_neighbors: null output");
    const std::vector<int> q = query_ids(ids_in, n_ids, items, "cu2rec_ease_neighbors: item id out of range (or negative n)");
    if (q.empty()) return;
    require_device();
    hipStream_t stream = nullptr;
    const EaseQuery a{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, B.ptr, ld, items, slices_of(items), k};
    ListRunner run(a, static_cast<int>(q.size()));
    run.run_to_host(q, out_ids, out_vals, stream);
}

void DeviceEase::recommend(const DeviceCsr &history, const DeviceCsr *exclude, const int *users, int n_users, int k, int *out_items,
                           float *out_scores) const {
    check_k("cu2rec_ease_recommend: k must be in [1, 256]", k);
    require(out_items && out_scores, "cu2rec_ease_recommend: null output");
    check_same_cols(*this, &history, "cu2rec_ease_recommend: the history's column count differs from the model's");
    check_same_cols(*this, exclude, "cu2rec_ease_recommend: the exclusions' column count differs from the model's");
    const std::vector<int> q = query_ids(users, n_users, history.rows, "cu2rec_ease_recommend: row id out of range (or negative n)");
    if (q.empty()) return;
    require_device();
    hipStream_t stream = nullptr;
    ListRunner run(recommend_query(*this, history, exclude, k, stream), static_cast<int>(q.size()));
    run.run_to_host(q, out_items, out_scores, stream);
}

void DeviceEase::rank_metrics(const DeviceCsr &history, const DeviceCsr *exclude, const DeviceCsr &test, int k, float threshold,
                              cu2rec_rank_metrics *out, double *per_user) const {
    check_k("cu2rec_ease_rank_metrics: k must be in [1, 256]", k);
    require(out, "cu2rec_ease_rank_metrics: null output");
    require(!std::isnan(threshold), "cu2rec_ease_rank_metrics: threshold is NaN");
    check_same_cols(*this, &history, "cu2rec_ease_rank_metrics: the history's column count differs from the model's");
    check_same_cols(*this, exclude, "cu2rec_ease_rank_metrics: the exclusions' column count differs from the model's");
    check_same_cols(*this, &test, "cu2rec_ease_rank_metrics: the test set's column count differs from the model's");
    require(test.rows <= history.rows, "cu2rec_ease_rank_metrics: the test set has rows past the history's rows");
    *out = empty_rank_metrics(k, history.rows);
    if (history.rows == 0) return;
    require_device();
    hipStream_t stream = nullptr;
    const int n = test.rows;  // rows past the test set's last row have no relevant items
    DeviceBuffer<int> d_all(std::max(n, 1));
    fill_iota(d_all.ptr, n, stream);
    ListRunner run(recommend_query(*this, history, exclude, k, stream), n);
    // the stage's own workspace per row counts against the same budget
    const size_t per_row = (static_cast<size_t>(run.a.n_slices) + 1) * k * 8 + RankStage::bytes_per_row(items);
    const int batch = static_cast<int>(std::min<size_t>(run.batch, std::max<size_t>(1, kEaseWorkspaceBytes / per_row)));
    DeviceBuffer<int> d_items(static_cast<size_t>(batch) * k);
    DeviceBuffer<float> d_scores(static_cast<size_t>(batch) * k);
    RankStage stage(history.rows, items, batch, stream);
    for (int p0 = 0; p0 < n; p0 += batch) {  // stream order keeps the workspace of one batch until the next needs it
        const int b = std::min(batch, n - p0);
        run.run(d_all.ptr + p0, b, d_items.ptr, d_scores.ptr, stream);
        stage.add(test, threshold, d_items.ptr, k, p0, b);
    }
    stage.finish(k, out, per_user);
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_ease_block_items(void) { return kEaseBlock; }

int cu2rec_ease_create(const cu2rec_csr *train, float l2, cu2rec_ease **out) {
    return guarded([&] {
        require(out, "cu2rec_ease_create: null argument");
        *out = nullptr;
        ease_check_l2("cu2rec_ease_create", l2);
        require(train, "cu2rec_ease_create: null argument");
        *out = new cu2rec_ease(unwrap(train), l2);
    });
}

void cu2rec_ease_destroy(cu2rec_ease *ease) { delete ease; }

int cu2rec_ease_info(const cu2rec_ease *ease, int *items, float *l2) {
    return guarded([&] {
        require(ease, "cu2rec_ease_info: null argument");
        if (items) *items = ease->impl.items;
        if (l2) *l2 = ease->impl.l2;
    });
}

int cu2rec_csr_ease_gram(const cu2rec_csr *csr, float l2, float *out) {
    return guarded([&] {
        ease_check_l2("cu2rec_csr_ease_gram", l2);
        require(csr && out, "cu2rec_csr_ease_gram: null argument");
        const DeviceCsr &m = unwrap(csr);
        if (m.cols > kEaseMaxItems) fail(CU2REC_EUNSUPPORTED, "cu2rec_csr_ease_gram: more than CU2REC_EASE_MAX_ITEMS columns");
        if (m.cols == 0) return;
        require_device();
        check_faults();
        const int ld = ease_padded(m.cols);
        DeviceBuffer<float> g;
        ease_allocate_matrix(g, static_cast<size_t>(ld) * ld, "cu2rec_csr_ease_gram");
        ease_gram(m, l2, ld, g.ptr, nullptr);
        const size_t row = static_cast<size_t>(m.cols) * sizeof(float);
        CU2REC_HIP(hipMemcpy2D(out, row, g.ptr, static_cast<size_t>(ld) * sizeof(float), row, m.cols, hipMemcpyDeviceToHost));
    });
}

int cu2rec_ease_weights(const cu2rec_ease *ease, const int *ids, int n, float *out) {
    return guarded([&] {
        require(ease, "cu2rec_ease_weights: null argument");
        ease->impl.weights(ids, n, out);
    });
}

int cu2rec_ease_neighbors(const cu2rec_ease *ease, const int *ids, int n, int k, int *out_ids, float *out_vals) {
    return guarded([&] {
        check_k("cu2rec_ease_neighbors: k must be in [1, 256]", k);
        require(ease, "cu2rec_ease_neighbors: null argument");
        ease->impl.neighbors(ids, n, k, out_ids, out_vals);
    });
}

int cu2rec_ease_recommend(const cu2rec_ease *ease, const cu2rec_csr *history, const cu2rec_csr *exclude, const int *users, int n, int k,
                          int *out_items, float *out_scores) {
    return guarded([&] {
        check_k("cu2rec_ease_recommend: k must be in [1, 256]", k);
        require(ease && history, "cu2rec_ease_recommend: null argument");
        ease->impl.recommend(unwrap(history), exclude ? &unwrap(exclude) : nullptr, users, n, k, out_items, out_scores);
    });
}

int cu2rec_ease_rank_metrics(const cu2rec_ease *ease, const cu2rec_csr *history, const cu2rec_csr *exclude, const cu2rec_csr *test, int k,
                             float threshold, cu2rec_rank_metrics *out, double *per_user) {
    return guarded([&] {
        check_k("cu2rec_ease_rank_metrics: k must be in [1, 256]", k);
        require(ease && history && test, "cu2rec_ease_rank_metrics: null argument");
        ease->impl.rank_metrics(unwrap(history), exclude ? &unwrap(exclude) : nullptr, unwrap(test), k, threshold, out, per_user);
    });
}

}  // extern "C"
