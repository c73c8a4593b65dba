// Fused top-k ranking and ranking metrics (include/cu2rec_amd.h: cu2rec_model_topk, cu2rec_model_rank_metrics).
//
// cu2rec_model_recommend writes the dense score matrix of a batch to HBM and radix-sorts every (user, item) pair to keep k of
// them.  Here a workgroup owns 32 users and walks the whole catalogue 128 items at a time: the four wavefronts score their
// 32 x 32 blocks exactly as scores_kernel does (score_tile.hpp: same staging chunks, same MFMA order, same bias sums), and
// each score goes straight into selection -- nothing of size users x items is ever written.
//
// Selection ("Fused top-k"; the keys and the wavefront sort are select.hpp's, shared with knn.hip): every score becomes a 64-bit key whose unsigned order is recommend's order -- the
// high word is rocPRIM's radix code of the float (descending sort; +0.0 and -0.0 one key), the low word the item index
// reversed, so equal scores rank by ascending item.  A user keeps a running threshold (its k-th best key so far, in LDS)
// and a candidate buffer of S = 256 or 512 keys (k <= 128 / k <= 256) in global workspace; a score that is not excluded, not
// -inf and above the threshold is appended (LDS atomic on the user's count).  After each 128-item step, a user whose
// buffer could overflow in the next step (count > S - 128) is compacted by one wavefront: bitonic sort of the S keys in
// registers, the best k written back, the threshold raised to the k-th.  A last sort emits the list.
//
// Excluded items are a bitmap in global workspace, one bit per (listed user, item), built for each batch of users with
// atomicOr from the exclusion CSR (rows unsorted, repeats harmless).  Batches bound the workspace: 256 MiB, or one
// 32-user tile where a single tile needs more (4 bytes per catalogue item: less than Q itself).
//
// Ranking metrics run the same selection over the model's rows, then one thread per user checks its list against a
// relevance bitmap of the test row and reduces in double (one final block-wide sum; one host synchronisation per call).
//
// The neighbour queries (cu2rec_model_similar, cu2rec_model_top_users) are the same kernel over other query and candidate
// matrices (TopkKind below): "user" and "item" in the comments here stand for query and candidate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <optional>
#include <vector>

#include "device.hpp"
#include "hip_check.hpp"
#include "rank_stage.hpp"
#include "score_tile.hpp"
#include "select.hpp"

namespace cu2rec {

namespace {

constexpr int kTopkMaxK = 256;
constexpr int kStep = 4 * kTile;                        // items scored per workgroup step
constexpr size_t kWorkspaceBudget = size_t(256) << 20;  // per batch of users
constexpr unsigned kEncNegInf = 0x007FFFFFu;            // radix code of -inf: never listed (recommend's mask value)

// What a selection ranks (include/cu2rec_amd.h): the query rows X and the candidate rows Y of the score tile, and the score
//   kUserItems   X = P, Y = Q                  ((gb + ub[query]) + ib[cand]) + x . y            cu2rec_model_topk
//   kSimilarDot  X = Y = P or Q                x . y, the query row itself not a candidate       cu2rec_model_similar, DOT
//   kSimilarCos  X = Y = unit rows of P or Q   x . y, ditto; +NaN where bad[query] or bad[cand]  cu2rec_model_similar, COSINE
//   kItemUsers   X = Q, Y = P                  ((gb + ub[cand]) + ib[query]) + y . x            cu2rec_model_top_users
// kItemUsers keeps P in the MFMA A operand as scores_kernel does (the candidate tile is A): the accumulator's rows are then
// candidates and its columns queries, so a lane owns one query and 16 candidates -- the same floats as cu2rec_model_scores.
enum TopkKind { kUserItems = 0, kSimilarDot = 1, kSimilarCos = 2, kItemUsers = 3 };

// One workgroup = 32 listed queries (positions pos0 .. pos0 + 31 of `qids`, rows of X) against every row of Y.  LDS: the query
// tile and four candidate tiles of scores_kernel, then the 32 thresholds and counts.  cand: [n_pos][64 E] keys of workspace.
// qbias / cbias: per-row values of the score (biases, or unit_rows_kernel's flags for kSimilarCos; unused by kSimilarDot).
template <int E, int Kind>
__global__ __launch_bounds__(256) void topk_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ qbias,
                                                   const int *__restrict__ qids, int n_pos, const float *__restrict__ Y, int ldy,
                                                   const float *__restrict__ cbias, int n_cand, float global_bias, int nslots,
                                                   int chunk, const unsigned *__restrict__ mask, int words, int k,
                                                   unsigned long long *__restrict__ cand, int *__restrict__ items_out,
                                                   float *__restrict__ scores_out) {
    constexpr int S = 64 * E;
    constexpr bool self = Kind == kSimilarDot || Kind == kSimilarCos;
    extern __shared__ float4 smem[];
    const int RS = chunk | 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pos0 = blockIdx.x * kTile;
    float4 *qtile = smem, *ctile = smem + (1 + wave) * kTile * RS;
    unsigned long long *thr = reinterpret_cast<unsigned long long *>(smem + 5 * kTile * RS);
    int *cnt = reinterpret_cast<int *>(thr + kTile);
    const int r = lane & 31, h = lane >> 5;
    if (threadIdx.x < kTile) {
        thr[threadIdx.x] = 0ull;
        cnt[threadIdx.x] = 0;
    }
    float qb[16];  // the bias (cosine: the flag) of the query of each accumulator row
    int qid[16];   // and its row id, for the self-exclusion
    float lane_qb = 0.f;  // kItemUsers: the bias of this lane's query (accumulator column r)
    if constexpr (Kind == kItemUsers) {
        lane_qb = pos0 + r < n_pos ? qbias[qids[pos0 + r]] : 0.f;
    } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pos = pos0 + acc_row(reg, h);
            if constexpr (Kind != kSimilarDot) qb[reg] = pos < n_pos ? qbias[qids[pos]] : 0.f;
            if constexpr (self) qid[reg] = pos < n_pos ? qids[pos] : -1;
        }
    }
    // wave w stages rows 8 w .. 8 w + 7 of the query tile: the row of this lane, gathered from X (clamped, zero past n_pos)
    const int srow = 8 * wave + (lane >> 3), cs = lane & 7;
    const float4 *xrow = reinterpret_cast<const float4 *>(X + static_cast<size_t>(qids[min(pos0 + srow, n_pos - 1)]) * ldx);
    const bool whole = chunk >= nslots;  // the query tile is staged once and stays
    for (int cand_base = 0; cand_base < n_cand; cand_base += kStep) {
        const int cand0 = cand_base + wave * kTile;
        const bool active = cand0 < n_cand;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int slot0 = 0; slot0 < nslots; slot0 += chunk) {
            const int n = min(chunk, nslots - slot0);
            __syncthreads();  // every wave is done reading the tiles (previous chunk or step)
            if (!whole || cand_base == 0) {
                for (int c = 0; c < (n + 7) >> 3; ++c) {
                    const int slot = 8 * c + cs;
                    const float4 v = xrow[slot0 + min(slot, n - 1)];
                    if (slot < n) qtile[srow * RS + slot] = pos0 + srow < n_pos ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            if (active) stage_rows(ctile, Y, ldy, cand0, n_cand, slot0, n, RS, lane);
            __syncthreads();
            if constexpr (Kind == kItemUsers) {
                if (active) contract(acc, ctile, qtile, RS, n, r, h);  // A: users (P), B: items (Q), as scores_kernel
            } else {
                if (active) contract(acc, qtile, ctile, RS, n, r, h);
            }
        }
        if constexpr (Kind == kItemUsers) {
            const int pos = pos0 + r;  // accumulator column = lane & 31 = query; rows = candidates cand0 + acc_row
            if (active && pos < n_pos) {
                const unsigned word = mask ? mask[static_cast<size_t>(pos) * words + (cand0 >> 5)] : 0u;  // cand0 % 32 == 0
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int row = acc_row(reg, h), c = cand0 + row;
                    if (c >= n_cand) continue;
                    const float s = ((global_bias + cbias[c]) + lane_qb) + acc[reg];  // scores_kernel's expression
                    const unsigned long long key = topk_key(s, c);
                    if (!((word >> row) & 1u) && static_cast<unsigned>(key >> 32) > kEncNegInf && key > thr[r]) {
                        const int at = atomicAdd(&cnt[r], 1);
                        cand[static_cast<size_t>(pos) * S + at] = key;
                    }
                }
            }
        } else {
            const int item = cand0 + r;  // accumulator column = lane & 31
            if (active && item < n_cand) {
                const float ibv = Kind == kSimilarDot ? 0.f : cbias[item];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int row = acc_row(reg, h), pos = pos0 + row;
                    if (pos >= n_pos) continue;
                    float s;
                    if constexpr (Kind == kUserItems) s = ((global_bias + qb[reg]) + ibv) + acc[reg];  // scores_kernel's expression
                    else if constexpr (Kind == kSimilarDot) s = acc[reg];
                    else s = qb[reg] != 0.f || ibv != 0.f ? __uint_as_float(0x7FC00000u) : acc[reg];
                    bool masked = mask && ((mask[static_cast<size_t>(pos) * words + (item >> 5)] >> (item & 31)) & 1u);
                    if constexpr (self) masked = masked || item == qid[reg];
                    const unsigned long long key = topk_key(s, item);
                    if (!masked && static_cast<unsigned>(key >> 32) > kEncNegInf && key > thr[row]) {
                        const int at = atomicAdd(&cnt[row], 1);
                        cand[static_cast<size_t>(pos) * S + at] = key;
                    }
                }
            }
        }
        __syncthreads();  // every insertion of this step is in place
        for (int row = wave; row < kTile; row += 4) {
            const int pos = pos0 + row, count = cnt[row];
            if (pos >= n_pos || count <= S - kStep) continue;  // room for another step
            unsigned long long *buf = cand + static_cast<size_t>(pos) * S;
            unsigned long long v[E];
            load_sorted<E>(v, buf, count, lane);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e * 64 + lane < k) buf[e * 64 + lane] = v[e];
                if (e * 64 + lane == k - 1) thr[row] = v[e];
            }
            if (lane == 0) cnt[row] = k;
        }
    }
    __syncthreads();
    for (int row = wave; row < kTile; row += 4) {
        const int pos = pos0 + row;
        if (pos >= n_pos) continue;
        unsigned long long v[E];
        load_sorted<E>(v, cand + static_cast<size_t>(pos) * S, cnt[row], lane);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = e * 64 + lane;
            if (j >= k) continue;
            int it;
            float sc;
            topk_decode(v[e], it, sc);
            items_out[static_cast<size_t>(pos) * k + j] = it;
            scores_out[static_cast<size_t>(pos) * k + j] = sc;
        }
    }
}

// The cosine pre-pass, one wavefront per row of X: unit[row] = x / |x| with |x| and the quotient in double, rounded to float, so
// that every row of finite floats with a nonzero norm -- subnormal elements or elements near FLT_MAX -- becomes a unit row and
// cosine is the plain dot product of two of them.  A zero row stays zero (cosine 0 with everything).  A row holding an inf or a
// NaN (its sum of squares is not finite: no square of a finite float overflows a double) is written as zeros and flagged:
// bad[row] = 1, and every score with it is +NaN (topk_kernel, kSimilarCos).  Columns n_factors .. ld - 1 are written as zeros.
__global__ __launch_bounds__(256) void unit_rows_kernel(const float *__restrict__ X, int ld, int n_factors, int n,
                                                        float *__restrict__ unit, float *__restrict__ bad) {
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += gridDim.x * 4) {
        const float *x = X + static_cast<size_t>(row) * ld;
        float *y = unit + static_cast<size_t>(row) * ld;
        double s = 0.0;
        for (int j = lane; j < n_factors; j += 64) s += static_cast<double>(x[j]) * static_cast<double>(x[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const bool finite = s <= __DBL_MAX__;  // false for +inf and NaN
        const double norm = sqrt(s);
        for (int j = lane; j < ld; j += 64)
            y[j] = j < n_factors && finite && s > 0.0 ? static_cast<float>(static_cast<double>(x[j]) / norm) : 0.f;
        if (lane == 0) bad[row] = finite ? 0.f : 1.f;
    }
}

// bit (position p, item) for every excluded item of the listed users
__global__ __launch_bounds__(256) void exclude_mask_kernel(const int *__restrict__ indptr, const int *__restrict__ indices,
                                                           int ex_rows, const int *__restrict__ users, int n_pos, int words,
                                                           unsigned *__restrict__ mask) {
    for (int p = blockIdx.x; p < n_pos; p += gridDim.x) {
        const int u = users[p];
        if (u >= ex_rows) continue;  // rows past the CSR's last row exclude nothing
        for (int e = indptr[u] + threadIdx.x; e < indptr[u + 1]; e += blockDim.x) {
            const int it = indices[e];
            atomicOr(&mask[static_cast<size_t>(p) * words + (it >> 5)], 1u << (it & 31));
        }
    }
}

// relevance of test rows row0 .. row0 + n_pos - 1: bit (p, item) for relevant items of the catalogue, and |R_u| -- distinct
// relevant items, those past the catalogue included -- in n_rel[p]
__global__ __launch_bounds__(256) void relevant_kernel(const int *__restrict__ indptr, const int *__restrict__ indices,
                                                       const float *__restrict__ data, int row0, int n_pos, int n_items, bool all,
                                                       float threshold, int words, unsigned *__restrict__ rel, int *__restrict__ n_rel) {
    for (int p = blockIdx.x; p < n_pos; p += gridDim.x) {
        const int lo = indptr[row0 + p], hi = indptr[row0 + p + 1];
        for (int e = lo + threadIdx.x; e < hi; e += blockDim.x) {
            if (!(all || data[e] >= threshold)) continue;
            const int it = indices[e];
            bool first = true;
            if (it < n_items) {
                const unsigned bit = 1u << (it & 31);
                first = !(atomicOr(&rel[static_cast<size_t>(p) * words + (it >> 5)], bit) & bit);
            } else {  // no bit to claim: the first relevant occurrence in the row counts
                for (int e2 = lo; e2 < e && first; ++e2) first = !(indices[e2] == it && (all || data[e2] >= threshold));
            }
            if (first) atomicAdd(&n_rel[p], 1);
        }
    }
}

// per model row u = row0 + p: {precision, recall, ndcg, ap, hit} of its list (include/cu2rec_amd.h), NaN when |R_u| = 0
__global__ __launch_bounds__(256) void rank_metrics_kernel(const int *__restrict__ items, int k, const unsigned *__restrict__ rel,
                                                           int words, const int *__restrict__ n_rel, int row0, int n_pos,
                                                           double *__restrict__ per_user) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pos) return;
    double *o = per_user + static_cast<size_t>(row0 + p) * 5;
    const int nr = n_rel[p];
    if (nr == 0) {
        for (int i = 0; i < 5; ++i) o[i] = __builtin_nan("");
        return;
    }
    int hits = 0;
    double dcg = 0.0, ap = 0.0;
    for (int j = 0; j < k; ++j) {
        const int it = items[static_cast<size_t>(p) * k + j];
        if (it < 0) break;  // padding only follows the listed items
        if ((rel[static_cast<size_t>(p) * words + (it >> 5)] >> (it & 31)) & 1u) {
            ++hits;
            dcg += 1.0 / log2(static_cast<double>(j + 2));
            ap += static_cast<double>(hits) / static_cast<double>(j + 1);
        }
    }
    const int m = min(k, nr);
    double idcg = 0.0;
    for (int j = 0; j < m; ++j) idcg += 1.0 / log2(static_cast<double>(j + 2));
    o[0] = static_cast<double>(hits) / static_cast<double>(k);
    o[1] = static_cast<double>(hits) / static_cast<double>(nr);
    o[2] = dcg / idcg;
    o[3] = ap / static_cast<double>(m);
    o[4] = hits > 0 ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void fill_nan_kernel(double *__restrict__ x, size_t n) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256)
        x[i] = __builtin_nan("");
}

// one workgroup: sums of the five metrics over evaluated rows (first value not NaN) and their count, in double
__global__ __launch_bounds__(256) void rank_sum_kernel(const double *__restrict__ per_user, int rows, double *__restrict__ out) {
    __shared__ double part[6][256];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int u = threadIdx.x; u < rows; u += 256) {
        const double *o = per_user + static_cast<size_t>(u) * 5;
        if (isnan(o[0])) continue;
        for (int i = 0; i < 5; ++i) s[i] += o[i];
        s[5] += 1.0;
    }
    for (int i = 0; i < 6; ++i) part[i][threadIdx.x] = s[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w)
            for (int i = 0; i < 6; ++i) part[i][threadIdx.x] += part[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 6) out[threadIdx.x] = part[threadIdx.x][0];
}

void check_k(const char *who, int k) {
    require(k >= 1, who);
    if (k > kTopkMaxK)
        fail(CU2REC_EUNSUPPORTED, std::string(who) + ": k above 256 is not supported here; cu2rec_model_recommend ranks any k");
}

// exclusions of rows x cols: rows past the CSR's rows exclude nothing; every excluded id names a candidate
void check_exclude(const DeviceCsr *exclude, int rows, int cols, const char *what) {
    require(!exclude || (exclude->rows <= rows && exclude->max_item < cols), what);
}

// One selection: queries are rows of X (ids on the device), candidates rows 0 .. n_cand - 1 of Y; qbias / cbias as topk_kernel.
struct TopkProblem {
    int kind;
    const float *X;
    int ldx;
    const float *qbias;
    const float *Y;
    int ldy;
    const float *cbias;
    int n_cand, n_factors;
    float global_bias;
};

TopkProblem user_items(const DeviceModel &m) {
    return {kUserItems, m.P.ptr, m.ld, m.user_bias.ptr, m.Q.ptr, m.ldq, m.item_bias.ptr, m.cols, m.n_factors, m.global_bias};
}

template <int E>
const void *topk_kernel_ptr(int kind) {
    switch (kind) {
        case kUserItems: return reinterpret_cast<const void *>(topk_kernel<E, kUserItems>);
        case kSimilarDot: return reinterpret_cast<const void *>(topk_kernel<E, kSimilarDot>);
        case kSimilarCos: return reinterpret_cast<const void *>(topk_kernel<E, kSimilarCos>);
        default: return reinterpret_cast<const void *>(topk_kernel<E, kItemUsers>);
    }
}

// The selection for one list of queries, in batches over a bounded workspace.  extra: further workspace bytes the caller
// needs per listed query (rank metrics' relevance bitmap), counted in the batch size.
struct TopkRunner {
    TopkRunner(const TopkProblem &pb_, int k_, int n_total, bool masked, size_t extra) : pb(pb_), k(k_) {
        E = k + kStep <= 256 ? 4 : 8;
        nslots = (pb.n_factors + 3) / 4;
        chunk = nslots <= 63 ? nslots : 32;  // scores_kernel's chunking: the same scores
        lds = static_cast<size_t>(5) * kTile * (chunk | 1) * sizeof(float4) + kTile * (sizeof(unsigned long long) + sizeof(int));
        if (lds > kMaxLds) fail(CU2REC_EUNSUPPORTED, "top-k selection: the score tiles need more LDS than a workgroup has");
        words = (pb.n_cand + 31) / 32;
        const size_t per_pos = static_cast<size_t>(64 * E) * 8 + (masked ? static_cast<size_t>(words) * 4 : 0) +
                               static_cast<size_t>(k) * 8 + extra;
        const size_t fit = std::max<size_t>(kTile, kWorkspaceBudget / per_pos / kTile * kTile);
        batch = static_cast<int>(std::min<size_t>(fit, (static_cast<size_t>(n_total) + kTile - 1) / kTile * kTile));
        cand.allocate(static_cast<size_t>(batch) * 64 * E);
        if (masked) mask.allocate(static_cast<size_t>(batch) * words);
        items.allocate(static_cast<size_t>(batch) * k);
        scores.allocate(static_cast<size_t>(batch) * k);
    }
    // positions ids_dev[0 .. n) (rows of X) -> items / scores [n x k], device
    void run(const DeviceCsr *exclude, const int *ids_dev, int n, hipStream_t stream) {
        if (mask.ptr) {
            CU2REC_HIP(hipMemsetAsync(mask.ptr, 0, static_cast<size_t>(n) * words * sizeof(unsigned), stream));
            if (exclude->nnz > 0)
                hipLaunchKernelGGL(exclude_mask_kernel, dim3(std::min(n, 4096)), dim3(256), 0, stream, exclude->indptr.ptr,
                                   exclude->indices.ptr, exclude->rows, ids_dev, n, words, mask.ptr);
        }
        const void *kernel = E == 4 ? topk_kernel_ptr<4>(pb.kind) : topk_kernel_ptr<8>(pb.kind);
        ensure_max_dynamic_lds(kernel, kMaxLds);
        const dim3 grid((n + kTile - 1) / kTile);
        const float *X = pb.X, *qbias = pb.qbias, *Y = pb.Y, *cbias = pb.cbias;
        int ldx = pb.ldx, ldy = pb.ldy, n_cand = pb.n_cand;
        float global_bias = pb.global_bias;
        void *args[] = {&X, &ldx, &qbias, &ids_dev, &n, &Y, &ldy, &cbias, &n_cand, &global_bias, &nslots, &chunk, &mask.ptr, &words,
                        &k, &cand.ptr, &items.ptr, &scores.ptr};  // topk_kernel's parameters, in order
        CU2REC_HIP(hipLaunchKernel(kernel, grid, dim3(256), args, lds, stream));
    }
    const TopkProblem pb;
    int k, E, nslots, chunk, words, batch;
    size_t lds;
    DeviceBuffer<unsigned long long> cand;
    DeviceBuffer<unsigned> mask;
    DeviceBuffer<int> items;
    DeviceBuffer<float> scores;
};

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

// every listed query's k best candidates -> host items_out / scores_out [n x k], batch by batch
void select_to_host(const TopkProblem &pb, const DeviceCsr *exclude, const std::vector<int> &ids, int k, int *items_out,
                    float *scores_out, hipStream_t stream) {
    const int n = static_cast<int>(ids.size());
    DeviceBuffer<int> d_ids(ids.size());
    d_ids.upload(ids.data(), ids.size());
    TopkRunner run(pb, k, n, exclude && exclude->nnz > 0, 0);
    for (int p0 = 0; p0 < n; p0 += run.batch) {
        const int b = std::min(run.batch, n - p0);
        run.run(exclude, d_ids.ptr + p0, b, stream);
        CU2REC_HIP(hipMemcpyAsync(items_out + static_cast<size_t>(p0) * k, run.items.ptr, static_cast<size_t>(b) * k * sizeof(int),
                                  hipMemcpyDeviceToHost, stream));
        CU2REC_HIP(hipMemcpyAsync(scores_out + static_cast<size_t>(p0) * k, run.scores.ptr,
                                  static_cast<size_t>(b) * k * sizeof(float), hipMemcpyDeviceToHost, stream));
    }  // stream order: a batch's copies are done before the next batch overwrites the workspace
    CU2REC_HIP(hipStreamSynchronize(stream));
}

}  // namespace

// the k best non-excluded items of each listed user, best first (recommend's order and scores)
void model_topk(const DeviceModel &m, const DeviceCsr *exclude, const int *users, int n_users, int k, int *items_out,
                float *scores_out) {
    check_k("cu2rec_model_topk: k must be at least 1", k);
    require(items_out && scores_out, "cu2rec_model_topk: null output");
    const std::vector<int> ids = query_ids(users, n_users, m.rows, "cu2rec_model_topk: user id out of range (or negative n_users)");
    check_exclude(exclude, m.rows, m.cols, "cu2rec_model_topk: exclusions exceed the model's shape");
    if (ids.empty()) return;
    require(m.cols > 0, "cu2rec_model_topk: no items");
    require_device();
    select_to_host(user_items(m), exclude, ids, k, items_out, scores_out, nullptr);
}

// the k nearest other rows of the same side (include/cu2rec_amd.h: cu2rec_model_similar)
void model_similar(const DeviceModel &m, int side, int metric, const DeviceCsr *exclude, const int *ids_in, int n_ids, int k,
                   int *ids_out, float *scores_out) {
    check_k("cu2rec_model_similar: k must be at least 1", k);
    require(ids_out && scores_out, "cu2rec_model_similar: null output");
    require(side == CU2REC_SIDE_USERS || side == CU2REC_SIDE_ITEMS, "cu2rec_model_similar: side is neither users nor items");
    require(metric == CU2REC_SIM_DOT || metric == CU2REC_SIM_COSINE, "cu2rec_model_similar: metric is neither dot nor cosine");
    const bool users = side == CU2REC_SIDE_USERS;
    const int rows = users ? m.rows : m.cols;
    const std::vector<int> ids = query_ids(ids_in, n_ids, rows, "cu2rec_model_similar: id out of range (or negative n_ids)");
    check_exclude(exclude, rows, rows, "cu2rec_model_similar: exclusions exceed the side's rows");
    if (ids.empty()) return;
    require_device();
    hipStream_t stream = nullptr;
    const float *X = users ? m.P.ptr : m.Q.ptr;
    const int ld = users ? m.ld : m.ldq;
    const bool cosine = metric == CU2REC_SIM_COSINE;
    DeviceBuffer<float> unit, bad;
    if (cosine) {  // recomputed on every call: one read of the side's rows, nothing to keep in sync
        unit.allocate(static_cast<size_t>(rows) * ld);
        bad.allocate(rows);
        hipLaunchKernelGGL(unit_rows_kernel, dim3(std::min((rows + 3) / 4, 8192)), dim3(256), 0, stream, X, ld, m.n_factors, rows,
                           unit.ptr, bad.ptr);
        CU2REC_HIP(hipGetLastError());
    }
    const float *Xs = cosine ? unit.ptr : X;
    const TopkProblem pb{cosine ? kSimilarCos : kSimilarDot, Xs, ld, bad.ptr, Xs, ld, bad.ptr, rows, m.n_factors, 0.f};
    select_to_host(pb, exclude, ids, k, ids_out, scores_out, stream);
}

// the k best non-excluded users of each listed item, with cu2rec_model_scores' floats
void model_top_users(const DeviceModel &m, const DeviceCsr *exclude, const int *items, int n_items, int k, int *users_out,
                     float *scores_out) {
    check_k("cu2rec_model_top_users: k must be at least 1", k);
    require(users_out && scores_out, "cu2rec_model_top_users: null output");
    const std::vector<int> ids = query_ids(items, n_items, m.cols, "cu2rec_model_top_users: item id out of range (or negative n_items)");
    check_exclude(exclude, m.cols, m.rows, "cu2rec_model_top_users: exclusions exceed the model's shape (items x users)");
    if (ids.empty()) return;
    require(m.rows > 0, "cu2rec_model_top_users: no users");
    require_device();
    const TopkProblem pb{kItemUsers, m.Q.ptr, m.ldq, m.item_bias.ptr, m.P.ptr, m.ld, m.user_bias.ptr, m.rows, m.n_factors,
                         m.global_bias};
    select_to_host(pb, exclude, ids, k, users_out, scores_out, nullptr);
}

void model_rank_metrics(const DeviceModel &m, const DeviceCsr *exclude, const DeviceCsr *test, int k, float threshold,
                        cu2rec_rank_metrics *out, double *per_user) {
    check_k("cu2rec_model_rank_metrics: k must be at least 1", k);
    require(test && out, "cu2rec_model_rank_metrics: null argument");
    require(!std::isnan(threshold), "cu2rec_model_rank_metrics: threshold is NaN");
    require(test->rows <= m.rows, "cu2rec_model_rank_metrics: the test set has rows past the model's rows");
    check_exclude(exclude, m.rows, m.cols, "cu2rec_model_rank_metrics: exclusions exceed the model's shape");
    *out = empty_rank_metrics(k, m.rows);
    if (m.rows == 0) return;
    require(m.cols > 0, "cu2rec_model_rank_metrics: no items");
    require_device();
    hipStream_t stream = nullptr;
    const int n = test->rows;  // rows past the test set's last row have no relevant items
    std::vector<int> ids(n);
    for (int i = 0; i < n; ++i) ids[i] = i;
    DeviceBuffer<int> d_ids(n);
    std::optional<TopkRunner> run;
    if (n > 0) {
        d_ids.upload(ids.data(), n);
        run.emplace(user_items(m), k, n, exclude && exclude->nnz > 0, RankStage::bytes_per_row(m.cols));
    }
    RankStage stage(m.rows, m.cols, n > 0 ? run->batch : 1, stream);
    for (int p0 = 0; p0 < n; p0 += run->batch) {  // stream order keeps the workspace of one batch until the next needs it
        const int b = std::min(run->batch, n - p0);
        run->run(exclude, d_ids.ptr + p0, b, stream);
        stage.add(*test, threshold, run->items.ptr, k, p0, b);
    }
    stage.finish(k, out, per_user);
}

cu2rec_rank_metrics empty_rank_metrics(int k, int rows) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    return cu2rec_rank_metrics{k, 0, rows, nan, nan, nan, nan, nan};
}

RankStage::RankStage(int rows_, int cols_, int batch, hipStream_t stream_)
    : rows(rows_), cols(cols_), words((cols_ + 31) / 32), stream(stream_), d_per(static_cast<size_t>(rows_) * 5), d_sum(6),
      rel(static_cast<size_t>(batch) * ((cols_ + 31) / 32)), n_rel(batch) {
    hipLaunchKernelGGL(fill_nan_kernel, dim3(std::min<size_t>((d_per.count + 255) / 256, 4096)), dim3(256), 0, stream, d_per.ptr,
                       d_per.count);
    CU2REC_HIP(hipGetLastError());
}

void RankStage::add(const DeviceCsr &test, float threshold, const int *items, int k, int p0, int b) {
    const bool all = std::isinf(threshold) && threshold < 0;
    CU2REC_HIP(hipMemsetAsync(rel.ptr, 0, static_cast<size_t>(b) * words * sizeof(unsigned), stream));
    CU2REC_HIP(hipMemsetAsync(n_rel.ptr, 0, static_cast<size_t>(b) * sizeof(int), stream));
    hipLaunchKernelGGL(relevant_kernel, dim3(std::min(b, 4096)), dim3(256), 0, stream, test.indptr.ptr, test.indices.ptr,
                       test.data.ptr, p0, b, cols, all, threshold, words, rel.ptr, n_rel.ptr);
    hipLaunchKernelGGL(rank_metrics_kernel, dim3((b + 255) / 256), dim3(256), 0, stream, items, k, rel.ptr, words, n_rel.ptr, p0, b,
                       d_per.ptr);
    CU2REC_HIP(hipGetLastError());
}

void RankStage::finish(int k, cu2rec_rank_metrics *out, double *per_user) {
    *out = empty_rank_metrics(k, rows);
    hipLaunchKernelGGL(rank_sum_kernel, dim3(1), dim3(256), 0, stream, d_per.ptr, rows, d_sum.ptr);
    CU2REC_HIP(hipGetLastError());
    double sums[6];
    CU2REC_HIP(hipMemcpyAsync(sums, d_sum.ptr, sizeof(sums), hipMemcpyDeviceToHost, stream));
    if (per_user) CU2REC_HIP(hipMemcpyAsync(per_user, d_per.ptr, d_per.count * sizeof(double), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    const int evaluated = static_cast<int>(sums[5]);
    out->users_evaluated = evaluated;
    out->users_skipped = rows - evaluated;
    if (evaluated > 0) {
        out->precision = sums[0] / evaluated;
        out->recall = sums[1] / evaluated;
        out->ndcg = sums[2] / evaluated;
        out->map = sums[3] / evaluated;
        out->hit_rate = sums[4] / evaluated;
    }
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_model_topk(const cu2rec_model *m, const cu2rec_csr *exclude, const int *users, int n_users, int k, int *items_out,
                      float *scores_out) {
    return guarded([&] {
        require(m, "model is null");
        model_topk(unwrap(m), exclude ? &unwrap(exclude) : nullptr, users, n_users, k, items_out, scores_out);
    });
}

int cu2rec_model_rank_metrics(const cu2rec_model *m, const cu2rec_csr *exclude, const cu2rec_csr *test, int k, float threshold,
                              cu2rec_rank_metrics *out, double *per_user) {
    return guarded([&] {
        require(m, "model is null");
        model_rank_metrics(unwrap(m), exclude ? &unwrap(exclude) : nullptr, test ? &unwrap(test) : nullptr, k, threshold, out,
                           per_user);
    });
}

int cu2rec_model_similar(const cu2rec_model *m, int side, int metric, const cu2rec_csr *exclude, const int *ids, int n_ids, int k,
                         int *ids_out, float *scores_out) {
    return guarded([&] {
        require(m, "model is null");
        model_similar(unwrap(m), side, metric, exclude ? &unwrap(exclude) : nullptr, ids, n_ids, k, ids_out, scores_out);
    });
}

int cu2rec_model_top_users(const cu2rec_model *m, const cu2rec_csr *exclude, const int *items, int n_items, int k, int *users_out,
                           float *scores_out) {
    return guarded([&] {
        require(m, "model is null");
        model_top_users(unwrap(m), exclude ? &unwrap(exclude) : nullptr, items, n_items, k, users_out, scores_out);
    });
}

}  // extern "C"
