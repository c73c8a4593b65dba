// Bayesian Personalized Ranking, deterministic and full batch (bpr.hpp; include/cu2rec_amd.h: cu2rec_model_bpr).
//
// With x_e = (ib_i - ib_j) + p_u . (q_i - q_j) for the triple (u, i, j_e) of entry e and c_e = sigma(-x_e):
//   g_u  = sum_(triples of u) c_e (q_i - q_j) - P_reg p_u                                   (the bias' gradient is a zero)
//   g_i  = sum_(e: item(e) = i) c_e p_u - sum_(e: j_e = i) c_e p_u - Q_reg q_i,   gb_i = sum_pos c_e - sum_neg c_e - item_bias_reg ib_i
//
// NEGATIVES (bpr_negatives_kernel): one thread per entry draws up to kBprAttempts items from sampler.hpp and takes the first that a
// binary search does not find in the row's ascending items (csr_views.hpp: the row-sorted view).
// USERS (bpr_user_kernel): one wavefront per user on row_wave.hpp's ENTRY map, exactly lmf_sparse_kernel's walk: group g takes the
// row's entries g, g + 4, ... in ascending order, gathers q_i and q_j, forms the difference once, dots it with the staged p_u, and
// adds c_e times it to the group's sums; the four groups are added in group order.  The CoefOnly instantiation stores c_e instead.
// REGROUPING: a stable radix sort of the entries by j_e (-1 as `cols`, past the end) and the first position of every item in it.
// ITEMS (bpr_item_kernel): one wavefront per item on the same map: its positives in ascending item-major position (the CSR's
// item-major view, whose kept sort values name each one's entry), then its negatives in ascending entry, gathering [p_u | 1] and c_e.
// Every sum's order is a function of positions alone: no float atomics, bit-identical run to run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bpr.hpp"
#include "device.hpp"
#include "logistic.hpp"
#include "objective_pass.hpp"
#include "rocprim_temp.hpp"
#include "row_wave.hpp"
#include "sampler.hpp"

namespace cu2rec {

namespace {

__global__ __launch_bounds__(kElementThreads) void bpr_negatives_kernel(const int *__restrict__ indptr, const int *__restrict__ sorted,
                                                                        const int *__restrict__ row_of, int cols, int nnz, uint64_t seed,
                                                                        uint32_t sweep, int *__restrict__ neg,
                                                                        unsigned *__restrict__ neg_key) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += gridDim.x * blockDim.x) {
        const int u = row_of[e];
        const int lo = indptr[u], hi = indptr[u + 1];
        const uint32_t k = static_cast<uint32_t>(e - lo);
        int j = -1;
        for (uint32_t a = 0; a < static_cast<uint32_t>(kBprAttempts); ++a) {
            const uint64_t iteration = (static_cast<uint64_t>(sweep * kBprAttempts + a) << 32) | k;
            const int cand = sampler_index(seed, static_cast<uint64_t>(u), iteration, 0, cols);
            const int l = first_at_least(sorted, lo, hi, cand);  // in the row's ascending items
            if (l == hi || sorted[l] != cand) {
                j = cand;
                break;
            }
        }
        neg[e] = j;
        neg_key[e] = j < 0 ? static_cast<unsigned>(cols) : static_cast<unsigned>(j);
    }
}

struct BprRowArgs {
    BprProblem p;
    const int *neg, *row_of, *neg_e, *n_indptr;
    float *coef;
    float *grad;  // [own rows][ldg]
    int ldg;
};

__device__ __forceinline__ float4 sub4(const float4 &a, const float4 &b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// E = ceil((f + 1) / 64) elements per lane, as in lmf_sparse_kernel.  CoefOnly: coef[e] = c_e (0 where e has no triple), no gradient
template <int E, bool CoefOnly>
__global__ __launch_bounds__(kRowThreads) void bpr_user_kernel(BprRowArgs a) {
    __shared__ float4 lds4[kRowWaves * 5 * 16 * E];
    constexpr int FS = 64 * E;
    const BprProblem &p = a.p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int F = p.n_factors;
    float *pv = reinterpret_cast<float *>(lds4) + wave * 5 * FS;
    [[maybe_unused]] float *part = pv + FS;
    for (int row = blockIdx.x * kRowWaves + wave; row < p.rows; row += gridDim.x * kRowWaves) {
        const int lo = p.indptr[row], hi = p.indptr[row + 1];
        const float *x = p.P + static_cast<size_t>(row) * p.ldp;
        float xr[E];
        wave_sync();  // the previous row has read pv and part
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int c = lane + 64 * k;
            xr[k] = c < F ? x[c] : 0.f;
            pv[c] = xr[k];  // zero from F on
        }
        wave_sync();
        float4 v[E];
        [[maybe_unused]] float4 acc[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            v[k] = *reinterpret_cast<const float4 *>(pv + 4 * l16 + 64 * k);
            acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int e0 = lo; e0 < hi; e0 += 4) {  // group g takes entries g, g + 4, ... in ascending order
            const int e = e0 + g;
            const bool on = e < hi;
            const int ec = on ? e : hi - 1;
            const int i = p.indices[ec], j = a.neg[ec];
            const bool triple = on && j >= 0;
            const int jc = j >= 0 ? j : i;  // no triple: a row that exists, its values unused
            const float db = p.item_bias[i] - p.item_bias[jc];
            float4 q[E];
#pragma unroll
            for (int k = 0; k < E; ++k)
                q[k] = sub4(load_partner4<false>(p.Q, p.ldq, F, i, 4 * l16 + 64 * k), load_partner4<false>(p.Q, p.ldq, F, jc, 4 * l16 + 64 * k));
            const float d = group_dot4<E>(q, v);
            const float c = lmf_sigmoid(-(db + d));  // 1 - sigma(x), without the cancellation
            if constexpr (CoefOnly) {
                if (on && l16 == 0) a.coef[e] = triple ? c : 0.f;
            } else if (triple) {
#pragma unroll
                for (int k = 0; k < E; ++k) axpy4(c, q[k], acc[k]);
            }
        }
        if constexpr (!CoefOnly) {
            float t[E];
            combine_groups<E>(acc, part, part + g * FS + 4 * l16, lane, t);
            float *gr = a.grad + static_cast<size_t>(row) * a.ldg;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = lane + 64 * k;
                // the bias' zero is the negative one: lmf_step_kernel's x + (lr g) / sqrt(a') then returns x's bits for every x,
                // -0 included, and a + g g returns a's
                if (i <= F) gr[i] = i < F ? t[k] - p.P_reg * xr[k] : -0.f;
            }
        }
    }
}

template <int E>
__global__ __launch_bounds__(kRowThreads) void bpr_item_kernel(BprRowArgs a) {
    __shared__ float4 lds4[kRowWaves * 4 * 16 * E];
    constexpr int FS = 64 * E;
    const BprProblem &p = a.p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int F = p.n_factors;
    float *part = reinterpret_cast<float *>(lds4) + wave * 4 * FS;
    for (int row = blockIdx.x * kRowWaves + wave; row < p.cols; row += gridDim.x * kRowWaves) {
        float4 acc[E];
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int lo = p.t_indptr[row], hi = p.t_indptr[row + 1];
        for (int t = lo + g; t < hi; t += 4) {  // the positives, ascending item-major position
            const int e = p.t_pos[t];
            if (a.neg[e] < 0) continue;  // no triple: contributes nothing
            const int u = p.t_indices[t];
            const float c = a.coef[e];
#pragma unroll
            for (int k = 0; k < E; ++k) axpy4(c, load_partner4<true>(p.P, p.ldp, F, u, 4 * l16 + 64 * k), acc[k]);
        }
        const int nlo = a.n_indptr[row], nhi = a.n_indptr[row + 1];
        for (int t = nlo + g; t < nhi; t += 4) {  // then the negatives, ascending entry
            const int e = a.neg_e[t];
            const int u = a.row_of[e];
            const float c = -a.coef[e];
#pragma unroll
            for (int k = 0; k < E; ++k) axpy4(c, load_partner4<true>(p.P, p.ldp, F, u, 4 * l16 + 64 * k), acc[k]);
        }
        float s[E];
        wave_sync();  // the previous row has read part
        combine_groups<E>(acc, part, part + g * FS + 4 * l16, lane, s);
        const float *y = p.Q + static_cast<size_t>(row) * p.ldq;
        float *gr = a.grad + static_cast<size_t>(row) * a.ldg;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = lane + 64 * k;
            if (i > F) continue;
            gr[i] = i < F ? s[k] - p.Q_reg * y[i] : s[k] - p.item_bias_reg * p.item_bias[row];
        }
    }
}

// the triples' term, the three norms and the two counts, a 16-lane group per entry / row, in double; partials[block][6]
__global__ __launch_bounds__(kObjThreads) void bpr_objective_kernel(BprProblem p, const int *__restrict__ neg, const int *__restrict__ row_of,
                                                                    double *__restrict__ partials) {
    __shared__ double red[6][kObjThreads];
    const int tid = threadIdx.x, lane16 = tid & (kObjGroup - 1);
    const int group = (blockIdx.x * kObjThreads + tid) / kObjGroup, groups = gridDim.x * (kObjThreads / kObjGroup);
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = group; e < p.nnz; e += groups) {
        const int j = neg[e];
        if (j < 0) continue;  // the whole group: e is the group's
        const int u = row_of[e], i = p.indices[e];
        const float *x = p.P + static_cast<size_t>(u) * p.ldp;
        const double di = group_dot(x, p.Q + static_cast<size_t>(i) * p.ldq, p.n_factors, lane16);
        const double dj = group_dot(x, p.Q + static_cast<size_t>(j) * p.ldq, p.n_factors, lane16);
        const double xe = (static_cast<double>(p.item_bias[i]) - static_cast<double>(p.item_bias[j])) + (di - dj);
        if (lane16 == 0) {
            s[0] -= lmf_softplus(-xe);  // ln sigma(x)
            s[4] += 1.0;
            if (xe > 0.0) s[5] += 1.0;
        }
    }
    for (int u = group; u < p.rows; u += groups) {
        const float *x = p.P + static_cast<size_t>(u) * p.ldp;
        const double n2 = group_dot(x, x, p.n_factors, lane16);
        if (lane16 == 0) s[1] += n2;
    }
    for (int i = group; i < p.cols; i += groups) {
        const float *y = p.Q + static_cast<size_t>(i) * p.ldq;
        const double n2 = group_dot(y, y, p.n_factors, lane16);
        if (lane16 == 0) {
            s[2] += n2;
            s[3] += static_cast<double>(p.item_bias[i]) * static_cast<double>(p.item_bias[i]);
        }
    }
    block_reduce(s, red);
    if (tid == 0)
        for (int j = 0; j < 6; ++j) partials[6 * blockIdx.x + j] = red[j][0];
}

// once per CSR: the buffers of its size
void allocate(BprCache &c, const BprProblem &p, hipStream_t stream) {
    if (c.allocated) return;
    const size_t n = static_cast<size_t>(std::max(p.nnz, 1));
    c.iota.allocate(n);
    c.neg.allocate(n);
    c.neg_key.allocate(n);
    c.key_sorted.allocate(n);
    c.neg_e.allocate(n);
    c.coef.allocate(n);
    c.n_indptr.allocate(static_cast<size_t>(p.cols) + 1);
    fill_iota(c.iota.ptr, p.nnz, stream);
    c.allocated = true;
}

// once per (seed, sweep): the entries by ascending (j_e, e) and every item's first position among them
void regroup(BprCache &c, const BprProblem &p, hipStream_t stream) {
    if (c.grouped) return;
    sort_pairs_into_groups(c.sort_temp, c.neg_key.ptr, c.key_sorted.ptr, c.iota.ptr, c.neg_e.ptr, p.nnz, key_bits(p.cols) /* -1 sorts as `cols` */,
                           p.cols, c.n_indptr.ptr, stream);
    c.grouped = true;
}

BprRowArgs row_args(const DeviceCsr &train, const BprProblem &p, float *grad, int ldg, hipStream_t stream) {
    const BprCache &c = train.bpr;
    return {p, c.neg.ptr, row_of_view(train, stream), c.neg_e.ptr, c.n_indptr.ptr, c.coef.ptr, grad, ldg};
}

}  // namespace

void bpr_negatives(const DeviceCsr &train, const BprProblem &p, uint64_t seed, int sweep, hipStream_t stream) {
    BprCache &c = train.bpr;
    allocate(c, p, stream);
    if (c.have_neg && c.seed == seed && c.sweep == sweep) return;
    c.have_neg = c.grouped = false;
    const int *row_of = row_of_view(train, stream), *sorted = row_sorted_view(train, false, stream).idx.ptr;
    if (p.nnz > 0) {
        hipLaunchKernelGGL(bpr_negatives_kernel, dim3(element_grid(p.nnz)), dim3(kElementThreads), 0, stream, p.indptr, sorted, row_of, p.cols,
                           p.nnz, seed, static_cast<uint32_t>(sweep), c.neg.ptr, c.neg_key.ptr);
        CU2REC_HIP(hipGetLastError());
    }
    c.seed = seed;
    c.sweep = sweep;
    c.have_neg = true;
}

void bpr_user_gradient(const DeviceCsr &train, const BprProblem &p, float *grad, int ldg, hipStream_t stream) {
    if (p.rows <= 0) return;
    const BprRowArgs a = row_args(train, p, grad, ldg, stream);
    dispatch_1_to_4(p.n_factors + 1, [&](auto elems) {
        hipLaunchKernelGGL((bpr_user_kernel<elems(), false>), dim3(row_grid(p.rows)), dim3(kRowThreads), 0, stream, a);
    });
    CU2REC_HIP(hipGetLastError());
}

void bpr_item_gradient(const DeviceCsr &train, const BprProblem &p, float *grad, int ldg, hipStream_t stream) {
    if (p.cols <= 0) return;
    regroup(train.bpr, p, stream);
    const BprRowArgs a = row_args(train, p, grad, ldg, stream);
    dispatch_1_to_4(p.n_factors + 1, [&](auto elems) {
        if (p.rows > 0 && p.nnz > 0)
            hipLaunchKernelGGL((bpr_user_kernel<elems(), true>), dim3(row_grid(p.rows)), dim3(kRowThreads), 0, stream, a);
        hipLaunchKernelGGL((bpr_item_kernel<elems()>), dim3(row_grid(p.cols)), dim3(kRowThreads), 0, stream, a);
    });
    CU2REC_HIP(hipGetLastError());
}

void bpr_objective(const DeviceCsr &train, const BprProblem &p, double (&out)[6], hipStream_t stream) {
    BprCache &c = train.bpr;
    const int blocks = objective_blocks(static_cast<size_t>(std::max(p.nnz, std::max(p.rows, p.cols))));
    if (c.partials.count < 6 * static_cast<size_t>(blocks)) c.partials.allocate(6 * static_cast<size_t>(blocks));
    hipLaunchKernelGGL(bpr_objective_kernel, dim3(blocks), dim3(kObjThreads), 0, stream, p, c.neg.ptr, row_of_view(train, stream), c.partials.ptr);
    CU2REC_HIP(hipGetLastError());
    sum_block_partials(c.partials, blocks, out, stream);
}

}  // namespace cu2rec
