// Item-based nearest-neighbour recommendation (include/cu2rec_amd.h: cu2rec_knn_*).
//
// Building the model and recommending from it are one product.  A query has a list of (partner, alpha); every partner has a sparse
// row sorted by id; score[j] = sum alpha * row_partner[j]; the best few touched candidates are kept.
//   build:      the query is item i, its partners the users of column i in ascending item-major position with alpha = w_ui, the
//               partner rows the row-sorted weighted user rows;
//   recommend:  the query is a history row, its partners the row's items in ascending id order with alpha = r, the partner rows
//               the neighbour lists re-sorted by id (made once, at create time).
// knn_product_kernel: a wavefront owns one (query, slice of kKnnSliceItems consecutive candidate ids) with the slice's fp32
// accumulators and a touched bitmap in LDS.  64 partners at a time, every lane finds the slice's segment of one partner's row by
// binary search; then, partner after partner in list order, the lanes take consecutive entries of the segment -- distinct ids, so
// the update acc[j] = fmaf(alpha, v, acc[j]) is a plain LDS read-add-write, and the order of every sum is the partner list's.  No
// float atomics anywhere; the bitmap takes integer atomics.  Excluded and self ids are cleared from the bitmap, the touched
// entries become topk's 64-bit keys 256 at a time and the wavefront bitonic sort (select.hpp) keeps the slice's best 256;
// knn_merge_kernel folds the slices' lists of a query with the same sort.  Nothing of size items x items is ever written.
//
// The weights (knn_weights_kernel) are evaluated in double and rounded once; the per-column sums run lane-strided over the column
// in ascending item-major position and then down a fixed shuffle tree, bm25's mean over the columns in one workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device.hpp"
#include "hip_check.hpp"
#include "knn.hpp"
#include "rank_stage.hpp"
#include "rocprim_temp.hpp"
#include "select.hpp"

namespace cu2rec {

namespace {

constexpr int kSlice = kKnnSliceItems;
constexpr int kSliceWords = kSlice / 32;
constexpr int kChunk = 256;  // candidates that enter one sort beside the best 256 so far
static_assert(kSliceWords == 64 && kSlice % kChunk == 0, "one bitmap word per lane; whole chunks");

// ---- the weights -----------------------------------------------------------------------------------------------------------
__global__ void knn_idf_kernel(const int *__restrict__ indptr, int rows, int cols, double *__restrict__ idf) {
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < rows; u += gridDim.x * blockDim.x)
        idf[u] = log(static_cast<double>(cols)) - log(1.0 + static_cast<double>(indptr[u + 1] - indptr[u]));
}

// what a column's sum adds up per entry: r^2 (cosine), t^2 (tfidf), r (bm25)
__device__ __forceinline__ double knn_term(int weighting, double r, double idf) {
    if (weighting == CU2REC_KNN_COSINE) return r * r;
    if (weighting == CU2REC_KNN_TFIDF) {
        const double t = sqrt(r) * idf;
        return t * t;
    }
    return r;
}

// one wavefront per column of the item-major view: lane l adds entries l, l + 64, ... in ascending position, then a fixed tree
__global__ __launch_bounds__(256) void knn_column_sums_kernel(const int *__restrict__ t_indptr, const int *__restrict__ t_users,
                                                              const float *__restrict__ t_data, const double *__restrict__ idf,
                                                              int cols, int weighting, double *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cols; i += gridDim.x * 4) {
        double s = 0.0;
        for (int p = t_indptr[i] + lane; p < t_indptr[i + 1]; p += 64)
            s += knn_term(weighting, static_cast<double>(t_data[p]), weighting == CU2REC_KNN_TFIDF ? idf[t_users[p]] : 0.0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) sums[i] = s;
    }
}

// one workgroup: the mean of the column sums over all columns, thread-strided and then a fixed tree
__global__ __launch_bounds__(256) void knn_mean_kernel(const double *__restrict__ sums, int cols, double *__restrict__ mean) {
    __shared__ double part[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < cols; i += 256) s += sums[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *mean = part[0] / static_cast<double>(cols);
}

// one thread per item-major position p: the entry's weight into w (CSR entry order) and t_w (item-major order)
__global__ void knn_weights_kernel(const int *__restrict__ indices, const int *__restrict__ t_users, const float *__restrict__ t_data,
                                   const int *__restrict__ t_pos, const double *__restrict__ idf, const double *__restrict__ sums,
                                   const double *__restrict__ mean, int nnz, int weighting, double k1, double b,
                                   float *__restrict__ w, float *__restrict__ t_w) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += gridDim.x * blockDim.x) {
        const int e = t_pos[p];
        const double r = static_cast<double>(t_data[p]);
        double x = r;
        if (weighting == CU2REC_KNN_COSINE || weighting == CU2REC_KNN_TFIDF) {
            const double s = sums[indices[e]];
            const double t = weighting == CU2REC_KNN_COSINE ? r : sqrt(r) * idf[t_users[p]];
            x = s > 0.0 ? t / sqrt(s) : 0.0;
        } else if (weighting == CU2REC_KNN_BM25) {
            const double m = *mean;
            const double len = (1.0 - b) + (m != 0.0 ? b * sums[indices[e]] / m : 0.0);
            const double den = k1 * len + r;
            x = den != 0.0 ? r * (k1 + 1.0) / den * idf[t_users[p]] : 0.0;
        }
        const float xf = static_cast<float>(x);
        w[e] = xf;
        if (t_w) t_w[p] = xf;
    }
}

// ---- the product -----------------------------------------------------------------------------------------------------------
struct KnnProduct {
    const int *q_begin, *q_end;  // query id q's partner list: positions [q_begin[q], q_end[q]) of
    const int *q_partner;        //   the partner ids
    const float *q_alpha;        //   and their alphas
    const int *r_begin, *r_end;  // partner p's row: positions [r_begin[p], r_end[p]) of
    const int *r_idx;            //   candidate ids, ascending
    const float *r_val;          //   and values
    const int *ex_indptr, *ex_indices;  // exclusions by query id (null: none); rows past ex_rows exclude nothing
    int ex_rows;
    int n_cand, n_slices;
    int self;  // the query id is not its own candidate
    int k;
};

__device__ __forceinline__ int first_not_below(const int *__restrict__ a, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the wavefront's LDS accesses before this point are done before those after it (one wavefront shares acc / bits across lanes)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// wavefront w of the grid = (query position w / n_slices, slice w % n_slices) -> cand[w][k]: the slice's best k keys, best first
__global__ __launch_bounds__(256) void knn_product_kernel(KnnProduct a, const int *__restrict__ qids, int n_pos,
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
    for (int j = lane; j < kSlice; j += 64) acc[j] = 0.f;
    bits[lane] = 0u;
    wave_lds_sync();
    const int q_lo = a.q_begin[q], q_hi = a.q_end[q];
    for (int base = q_lo; base < q_hi; base += 64) {
        const int p = base + lane;
        int seg_lo = 0, seg_hi = 0;
        float alpha = 0.f;
        if (p < q_hi) {
            const int partner = a.q_partner[p];
            const int lo = a.r_begin[partner], hi = a.r_end[partner];
            alpha = a.q_alpha[p];
            seg_lo = first_not_below(a.r_idx, lo, hi, slice_lo);
            seg_hi = first_not_below(a.r_idx, seg_lo, hi, slice_hi);
        }
        unsigned long long live = __ballot(seg_hi > seg_lo);
        while (live) {  // partner after partner, in list order
            const int t = __ffsll(static_cast<long long>(live)) - 1;
            live &= live - 1;
            const int lo = __shfl(seg_lo, t), hi = __shfl(seg_hi, t);
            const float al = __shfl(alpha, t);
            for (int e = lo + lane; e < hi; e += 64) {  // distinct ids within one row
                const int j = a.r_idx[e] - slice_lo;
                acc[j] = fmaf(al, a.r_val[e], acc[j]);
                atomicOr(&bits[j >> 5], 1u << (j & 31));
            }
            wave_lds_sync();
        }
    }
    if (a.ex_indptr && q < a.ex_rows) {
        for (int e = a.ex_indptr[q] + lane; e < a.ex_indptr[q + 1]; e += 64) {
            const int it = a.ex_indices[e];
            if (it >= slice_lo && it < slice_hi) atomicAnd(&bits[(it - slice_lo) >> 5], ~(1u << ((it - slice_lo) & 31)));
        }
    }
    if (a.self && lane == 0 && q >= slice_lo && q < slice_hi) atomicAnd(&bits[(q - slice_lo) >> 5], ~(1u << ((q - slice_lo) & 31)));
    wave_lds_sync();
    unsigned long long v[8];  // slots 0 .. 255: the best so far, best first; slots 256 .. 511: the next chunk's candidates
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0ull;
    for (int c = 0; c * kChunk < slice_hi - slice_lo; ++c) {
        unsigned word[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            word[e] = bits[c * (kChunk / 32) + e * 2 + (lane >> 5)];
            any = any || word[e] != 0u;
        }
        if (!__any(any)) continue;  // nobody touched this chunk
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

// one wavefront per query position: the slices' lists folded into the best k -> ids_out / vals_out [n_pos][ld], first k columns
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long *__restrict__ cand, int n_pos, int n_slices, int k,
                                                        int ld, int *__restrict__ ids_out, float *__restrict__ vals_out) {
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
        ids_out[static_cast<size_t>(pos) * ld + j] = it;
        vals_out[static_cast<size_t>(pos) * ld + j] = sc;
    }
}

// one wavefront per item: its list by ascending id, the padding last -> s_idx / s_val, and the row's bounds
__global__ __launch_bounds__(256) void knn_sort_lists_kernel(const int *__restrict__ ids, const float *__restrict__ sims, int items,
                                                             int n, int *__restrict__ s_begin, int *__restrict__ s_end,
                                                             int *__restrict__ s_idx, float *__restrict__ s_val) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= items) return;
    unsigned long long v[4];
    int listed = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = e * 64 + lane;
        const int id = j < n ? ids[static_cast<size_t>(i) * n + j] : -1;
        // a smaller id is a larger key; the high word of a listed entry is never 0
        v[e] = id < 0 ? 0ull
                      : (static_cast<unsigned long long>(0x80000000u - static_cast<unsigned>(id)) << 32) |
                            __float_as_uint(sims[static_cast<size_t>(i) * n + j]);
        listed += __popcll(__ballot(id >= 0));
    }
    wave_sort_desc<4>(v, lane);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = e * 64 + lane;
        if (j >= n) continue;
        const bool empty = v[e] == 0ull;
        s_idx[static_cast<size_t>(i) * n + j] = empty ? -1 : static_cast<int>(0x80000000u - static_cast<unsigned>(v[e] >> 32));
        s_val[static_cast<size_t>(i) * n + j] = empty ? 0.f : __uint_as_float(static_cast<unsigned>(v[e]));
    }
    if (lane == 0) {
        s_begin[i] = i * n;
        s_end[i] = i * n + listed;
    }
}

__global__ void knn_take_kernel(const int *__restrict__ ids, const float *__restrict__ sims, int n, const int *__restrict__ qids,
                                int n_pos, int k, int *__restrict__ ids_out, float *__restrict__ sims_out) {
    const size_t total = static_cast<size_t>(n_pos) * k;
    for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const size_t pos = t / k, j = t % k;
        ids_out[t] = ids[static_cast<size_t>(qids[pos]) * n + j];
        sims_out[t] = sims[static_cast<size_t>(qids[pos]) * n + j];
    }
}

// The product for a list of queries, in batches over a bounded workspace.
struct ProductRunner {
    ProductRunner(const KnnProduct &a_, int n_total) : a(a_) {
        const size_t per_query = (static_cast<size_t>(a.n_slices) + 1) * a.k * 8;  // the slices' keys and the list itself
        batch = static_cast<int>(std::min<size_t>(std::max<size_t>(1, kKnnWorkspaceBytes / per_query), std::max(n_total, 1)));
        cand.allocate(static_cast<size_t>(batch) * a.n_slices * a.k);
    }
    // query positions qids[0 .. n) -> ids_out / vals_out [n][ld] (device), first k columns
    void run(const int *qids, int n, int ld, int *ids_out, float *vals_out, hipStream_t stream) {
        const int waves = n * a.n_slices;
        hipLaunchKernelGGL(knn_product_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, a, qids, n, cand.ptr);
        hipLaunchKernelGGL(knn_merge_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, cand.ptr, n, a.n_slices, a.k, ld, ids_out,
                           vals_out);
        CU2REC_HIP(hipGetLastError());
    }
    const KnnProduct a;
    int batch;
    DeviceBuffer<unsigned long long> cand;
};

int slices_of(int n_cand) { return std::max(1, (n_cand + kSlice - 1) / kSlice); }

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

void check_k(const char *what, int k, int top) { require(k >= 1 && k <= top, what); }

// the recommend product over `history` (its row-sorted view) and the model's id-sorted lists
KnnProduct recommend_product(const DeviceKnn &m, const DeviceCsr &history, const DeviceCsr *exclude, int k, hipStream_t stream) {
    const RowSortedView &rows = row_sorted_view(history, true, stream);
    if (rows.has_duplicate) fail(CU2REC_EINVAL, "cu2rec_knn: a history row stores the same column twice");
    const bool ex = exclude && exclude->nnz > 0;
    return KnnProduct{history.indptr.ptr, history.indptr.ptr + 1, rows.idx.ptr, rows.val.ptr, m.s_begin.ptr, m.s_end.ptr, m.s_idx.ptr,
                      m.s_val.ptr, ex ? exclude->indptr.ptr : nullptr, ex ? exclude->indices.ptr : nullptr, ex ? exclude->rows : 0,
                      m.items, slices_of(m.items), 0, k};
}

void check_same_cols(const DeviceKnn &m, const DeviceCsr *csr, const char *what) { require(!csr || csr->cols == m.items, what); }

}  // namespace

void knn_check_weighting(const char *fn, int weighting, float k1, float b) {
    const Need need{fn};
    need(weighting >= CU2REC_KNN_COUNT && weighting <= CU2REC_KNN_BM25, CU2REC_EINVAL, ": weighting is none of count, cosine, tfidf, bm25");
    need(std::isfinite(k1) && k1 >= 0.f, CU2REC_EINVAL, ": k1 must be finite and >= 0");
    need(b >= 0.f && b <= 1.f, CU2REC_EINVAL, ": b must be in [0, 1]");
}

void knn_weights(const DeviceCsr &csr, int weighting, float k1, float b, float *w, float *t_w, hipStream_t stream) {
    if (csr.nnz == 0) return;
    const ItemMajorView &view = item_major_view(csr, stream);
    DeviceBuffer<double> idf(std::max(csr.rows, 1)), sums(std::max(csr.cols, 1)), mean(1);
    if (weighting == CU2REC_KNN_TFIDF || weighting == CU2REC_KNN_BM25)  // the other two never read it
        hipLaunchKernelGGL(knn_idf_kernel, dim3(element_grid(static_cast<size_t>(csr.rows))), dim3(256), 0, stream, csr.indptr.ptr, csr.rows,
                           csr.cols, idf.ptr);
    if (weighting != CU2REC_KNN_COUNT)
        hipLaunchKernelGGL(knn_column_sums_kernel, dim3(element_grid(static_cast<size_t>(csr.cols), 4)), dim3(256), 0, stream, view.indptr.ptr,
                           view.indices.ptr, view.data.ptr, idf.ptr, csr.cols, weighting, sums.ptr);
    if (weighting == CU2REC_KNN_BM25) hipLaunchKernelGGL(knn_mean_kernel, dim3(1), dim3(256), 0, stream, sums.ptr, csr.cols, mean.ptr);
    hipLaunchKernelGGL(knn_weights_kernel, dim3(element_grid(static_cast<size_t>(csr.nnz))), dim3(256), 0, stream, csr.indices.ptr,
                       view.indices.ptr, view.data.ptr, view.pos.ptr, idf.ptr, sums.ptr, mean.ptr, csr.nnz, weighting, static_cast<double>(k1),
                       static_cast<double>(b), w, t_w);
    CU2REC_HIP(hipGetLastError());
    CU2REC_HIP(hipStreamSynchronize(stream));  // before the temporaries are freed
}

DeviceKnn::DeviceKnn(const DeviceCsr &train, int weighting_, float k1, float b, int neighbours_)
    : items(train.cols), neighbours(neighbours_), weighting(weighting_) {
    knn_check_weighting("cu2rec_knn_create", weighting, k1, b);
    check_k("cu2rec_knn_create: neighbours must be in [1, 256]", neighbours, kKnnMaxK);
    require(items >= 1, "cu2rec_knn_create: no items");
    require(static_cast<long long>(items) * neighbours <= 0x7FFFFFFFll, "cu2rec_knn_create: items x neighbours exceeds 2^31 - 1");
    require_device();
    check_faults();
    hipStream_t stream = nullptr;
    const RowSortedView &rows = row_sorted_view(train, true, stream);
    if (rows.has_duplicate) fail(CU2REC_EINVAL, "cu2rec_knn_create: a row stores the same column twice");
    const size_t nnz = static_cast<size_t>(std::max(train.nnz, 1)), total = static_cast<size_t>(items) * neighbours;
    DeviceBuffer<float> w(nnz), t_w(nnz), sw(nnz);
    knn_weights(train, weighting, k1, b, w.ptr, t_w.ptr, stream);
    const ItemMajorView &view = item_major_view(train, stream);
    gather(w.ptr, rows.pos.ptr, train.nnz, sw.ptr, stream);
    ids.allocate(total);
    sims.allocate(total);
    s_begin.allocate(items);
    s_end.allocate(items);
    s_idx.allocate(total);
    s_val.allocate(total);
    const KnnProduct build{view.indptr.ptr, view.indptr.ptr + 1, view.indices.ptr, t_w.ptr, train.indptr.ptr, train.indptr.ptr + 1, rows.idx.ptr,
                           sw.ptr, nullptr, nullptr, 0, items, slices_of(items), 1, neighbours};
    DeviceBuffer<int> d_all(items);
    fill_iota(d_all.ptr, items, stream);
    ProductRunner run(build, items);
    for (int p0 = 0; p0 < items; p0 += run.batch)  // stream order: a batch's merge is done before the next product overwrites the keys
        run.run(d_all.ptr + p0, std::min(run.batch, items - p0), neighbours, ids.ptr + static_cast<size_t>(p0) * neighbours,
                sims.ptr + static_cast<size_t>(p0) * neighbours, stream);
    hipLaunchKernelGGL(knn_sort_lists_kernel, dim3((items + 3) / 4), dim3(256), 0, stream, ids.ptr, sims.ptr, items, neighbours,
                       s_begin.ptr, s_end.ptr, s_idx.ptr, s_val.ptr);
    CU2REC_HIP(hipGetLastError());
    CU2REC_HIP(hipStreamSynchronize(stream));  // before the temporaries are freed
}

void DeviceKnn::neighbors(const int *ids_in, int n_ids, int k, int *out_ids, float *out_sims) const {
    require(k >= 1 && k <= neighbours, "cu2rec_knn_neighbors: k must be in [1, neighbours]");
    require(out_ids && out_sims, "cu2rec_knn_neighbors: null output");
    const std::vector<int> q = query_ids(ids_in, n_ids, items, "cu2rec_knn_neighbors: item id out of range (or negative n)");
    if (q.empty()) return;
    require_device();
    hipStream_t stream = nullptr;
    const size_t total = q.size() * k;
    DeviceBuffer<int> d_q(q.size()), d_ids(total);
    DeviceBuffer<float> d_sims(total);
    d_q.upload(q.data(), q.size());
    hipLaunchKernelGGL(knn_take_kernel, dim3(element_grid(total)), dim3(256), 0, stream, ids.ptr, sims.ptr, neighbours, d_q.ptr,
                       static_cast<int>(q.size()), k, d_ids.ptr, d_sims.ptr);
    CU2REC_HIP(hipGetLastError());
    d_ids.download(out_ids, total);
    d_sims.download(out_sims, total);
}

void DeviceKnn::recommend(const DeviceCsr &history, const DeviceCsr *exclude, const int *users, int n_users, int k, int *out_items,
                          float *out_scores) const {
    check_k("cu2rec_knn_recommend: k must be in [1, 256]", k, kKnnMaxK);
    require(out_items && out_scores, "cu2rec_knn_recommend: null output");
    check_same_cols(*this, &history, "cu2rec_knn_recommend: the history's column count differs from the model's");
    check_same_cols(*this, exclude, "cu2rec_knn_recommend: the exclusions' column count differs from the model's");
    const std::vector<int> q = query_ids(users, n_users, history.rows, "cu2rec_knn_recommend: row id out of range (or negative n)");
    if (q.empty()) return;
    require_device();
    hipStream_t stream = nullptr;
    const int n = static_cast<int>(q.size());
    DeviceBuffer<int> d_q(q.size());
    d_q.upload(q.data(), q.size());
    ProductRunner run(recommend_product(*this, history, exclude, k, stream), n);
    DeviceBuffer<int> d_items(static_cast<size_t>(run.batch) * k);
    DeviceBuffer<float> d_scores(static_cast<size_t>(run.batch) * k);
    for (int p0 = 0; p0 < n; p0 += run.batch) {
        const int b = std::min(run.batch, n - p0);
        run.run(d_q.ptr + p0, b, k, d_items.ptr, d_scores.ptr, stream);
        CU2REC_HIP(hipMemcpyAsync(out_items + static_cast<size_t>(p0) * k, d_items.ptr, static_cast<size_t>(b) * k * sizeof(int),
                                  hipMemcpyDeviceToHost, stream));
        CU2REC_HIP(hipMemcpyAsync(out_scores + static_cast<size_t>(p0) * k, d_scores.ptr, static_cast<size_t>(b) * k * sizeof(float),
                                  hipMemcpyDeviceToHost, stream));
    }  // stream order: a batch's copies are done before the next batch overwrites the workspace
    CU2REC_HIP(hipStreamSynchronize(stream));
}

void DeviceKnn::rank_metrics(const DeviceCsr &history, const DeviceCsr *exclude, const DeviceCsr &test, int k, float threshold,
                             cu2rec_rank_metrics *out, double *per_user) const {
    check_k("cu2rec_knn_rank_metrics: k must be in [1, 256]", k, kKnnMaxK);
    require(out, "cu2rec_knn_rank_metrics: null output");
    require(!std::isnan(threshold), "cu2rec_knn_rank_metrics: threshold is NaN");
    check_same_cols(*this, &history, "cu2rec_knn_rank_metrics: the history's column count differs from the model's");
    check_same_cols(*this, exclude, "cu2rec_knn_rank_metrics: the exclusions' column count differs from the model's");
    check_same_cols(*this, &test, "cu2rec_knn_rank_metrics: the test set's column count differs from the model's");
    require(test.rows <= history.rows, "cu2rec_knn_rank_metrics: the test set has rows past the history's rows");
    *out = empty_rank_metrics(k, history.rows);
    if (history.rows == 0) return;
    require_device();
    hipStream_t stream = nullptr;
    const int n = test.rows;  // rows past the test set's last row have no relevant items
    DeviceBuffer<int> d_all(std::max(n, 1));
    fill_iota(d_all.ptr, n, stream);
    ProductRunner run(recommend_product(*this, history, exclude, k, stream), n);
    // the stage's own workspace per row counts against the same budget
    const size_t per_row = (static_cast<size_t>(run.a.n_slices) + 1) * k * 8 + RankStage::bytes_per_row(items);
    const int batch = static_cast<int>(std::min<size_t>(run.batch, std::max<size_t>(1, kKnnWorkspaceBytes / per_row)));
    DeviceBuffer<int> d_items(static_cast<size_t>(batch) * k);
    DeviceBuffer<float> d_scores(static_cast<size_t>(batch) * k);
    RankStage stage(history.rows, items, batch, stream);
    for (int p0 = 0; p0 < n; p0 += batch) {  // stream order keeps the workspace of one batch until the next needs it
        const int b = std::min(batch, n - p0);
        run.run(d_all.ptr + p0, b, k, d_items.ptr, d_scores.ptr, stream);
        stage.add(test, threshold, d_items.ptr, k, p0, b);
    }
    stage.finish(k, out, per_user);
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_knn_slice_items(void) { return kKnnSliceItems; }

int cu2rec_knn_create(const cu2rec_csr *train, int weighting, float k1, float b, int neighbours, cu2rec_knn **out) {
    return guarded([&] {
        require(train && out, "cu2rec_knn_create: null argument");
        *out = nullptr;
        *out = new cu2rec_knn(unwrap(train), weighting, k1, b, neighbours);
    });
}

void cu2rec_knn_destroy(cu2rec_knn *knn) { delete knn; }

int cu2rec_knn_info(const cu2rec_knn *knn, int *items, int *neighbours, int *weighting) {
    return guarded([&] {
        require(knn, "cu2rec_knn_info: null argument");
        if (items) *items = knn->impl.items;
        if (neighbours) *neighbours = knn->impl.neighbours;
        if (weighting) *weighting = knn->impl.weighting;
    });
}

int cu2rec_csr_knn_weights(const cu2rec_csr *csr, int weighting, float k1, float b, float *out_nnz) {
    return guarded([&] {
        require(csr && out_nnz, "cu2rec_csr_knn_weights: null argument");
        knn_check_weighting("cu2rec_csr_knn_weights", weighting, k1, b);
        const DeviceCsr &m = unwrap(csr);
        if (m.nnz == 0) return;
        require(m.cols >= 1, "cu2rec_csr_knn_weights: no items");
        require_device();
        check_faults();
        DeviceBuffer<float> w(m.nnz);
        knn_weights(m, weighting, k1, b, w.ptr, nullptr, nullptr);
        w.download(out_nnz, m.nnz);
    });
}

int cu2rec_knn_neighbors(const cu2rec_knn *knn, const int *ids, int n, int k, int *out_ids, float *out_sims) {
    return guarded([&] {
        require(knn, "cu2rec_knn_neighbors: null argument");
        knn->impl.neighbors(ids, n, k, out_ids, out_sims);
    });
}

int cu2rec_knn_recommend(const cu2rec_knn *knn, const cu2rec_csr *history, const cu2rec_csr *exclude, const int *users, int n, int k,
                         int *out_items, float *out_scores) {
    return guarded([&] {
        require(knn && history, "cu2rec_knn_recommend: null argument");
        knn->impl.recommend(unwrap(history), exclude ? &unwrap(exclude) : nullptr, users, n, k, out_items, out_scores);
    });
}

int cu2rec_knn_rank_metrics(const cu2rec_knn *knn, const cu2rec_csr *history, const cu2rec_csr *exclude, const cu2rec_csr *test, int k,
                            float threshold, cu2rec_rank_metrics *out, double *per_user) {
    return guarded([&] {
        require(knn && history && test, "cu2rec_knn_rank_metrics: null argument");
        knn->impl.rank_metrics(unwrap(history), exclude ? &unwrap(exclude) : nullptr, unwrap(test), k, threshold, out, per_user);
    });
}

}  // extern "C"
