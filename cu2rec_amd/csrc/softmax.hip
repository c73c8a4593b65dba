// Softmax matrix factorization, full batch (softmax.hpp; include/cu2rec_amd.h: cu2rec_model_softmax).
//
// With lse_u = log sum_(i < I) exp(s_ui), pi_ui = exp(s_ui - lse_u) and W_u = the sum of user u's stored values, a half-step moves
// every own row against the frozen partner side:
//   users:  g_u  = sum_entries w q_i - W_u sum_(i < I) pi_ui q_i - P_reg p_u                     (no bias gradient)
//   items:  g_i  = sum_(u has i) w p_u - sum_(u < U) W_u pi_ui p_u - Q_reg q_i
//           gb_i = sum_(u has i) w     - sum_(u < U) W_u pi_ui     - item_bias_reg ib_i
// and then takes lmf.hip's AdaGrad step.  The dense kernels have lmf_dense_kernel's workgroup: 32 own rows staged once, the partner
// side walked 128 rows per step, one 32 x 32 block per wavefront scored through score_tile.hpp with the partners in the MFMA A
// operand, the staged tiles' padding columns zeroed, column f a synthesised 1; the score of a pair is the same float in all of them.
//
// ROW WEIGHTS (softmax_weights_kernel): W_u, one thread per user, the row's values added in entry order.
//
// LSE (softmax_lse_kernel): own rows are the users.  Of a step's block a lane (r, h) holds the scores of user r with 16 items: it
// takes their max m and l = sum expf(s - m) in register order; the halves h = 0 and h = 1 are merged; the wavefront keeps a running
// (m, l) over its steps, rescaled by expf(m_old - m_new) when the max moves; the four wavefronts' pairs go through LDS and are
// merged in wave order; lse = m + logf(l).  Items past I contribute nothing.  expf(x - x) is taken as 1 also where x is infinite.
//
// DENSE (softmax_dense_kernel): the coefficient of a pair, expf(s - lse_u) for the users and W_u expf(s - lse_u) for the items (W and
// lse loaded per partner, as the partner's bias is), is pushed through the second v_mfma_f32_32x32x2_f32 against [partner tile | 1]
// exactly as lmf_dense_kernel pushes sigma: G_u = sum_i pi_ui [q_i | 1], G_i = sum_u W_u pi_ui [p_u | 1].  The scores are computed
// again, not stored: they are pass 1's bits, so s - lse is at most a rounding above 0 and the accumulators need no rescaling.
// Column f of G_u is sum_i pi_ui, 1 within rounding.
//
// SPARSE (softmax_sparse_kernel): one wavefront per own row in row_wave.hpp's ENTRY map sums w [y | 1] over the row's entries, the
// four groups added in group order, and combines in place: g = (sparse - W_own G) - reg x for the users (column f: a zero),
// g = (sparse - G) - reg x for the items.
//
// Every sum's order is a function of the partner index or the entry position alone: no float atomics, bit-identical run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"
#include "objective_pass.hpp"
#include "row_wave.hpp"
#include "score_tile.hpp"
#include "softmax.hpp"

namespace cu2rec {

namespace {

constexpr int kSoftmaxStep = 4 * kTile;  // partners scored per workgroup step

// columns f .. 4 nslots - 1 of a staged [32][RS] tile become zeros (by the wavefront that staged it), as in lmf.hip
__device__ __forceinline__ void zero_padding(float4 *tile, int RS, int nslots, int f, int lane) {
    const int keep = f - 4 * (nslots - 1);  // 1 .. 4 data floats in the last slot
    if (keep < 4 && lane < kTile) {
        float4 v = tile[lane * RS + nslots - 1];
        if (keep < 2) v.y = 0.f;
        if (keep < 3) v.z = 0.f;
        v.w = 0.f;
        tile[lane * RS + nslots - 1] = v;
    }
}

// expf(x - m) for x <= m, with expf(x - x) = 1 also at x = -inf (a share without a partner) and +inf.  NaN in, NaN out.
__device__ __forceinline__ float exp_below(float x, float m) { return x == m ? 1.f : expf(x - m); }

// (m, l) <- the merge of (m, l) and (m2, l2), the first operand's term first
__device__ __forceinline__ void lse_merge(float &m, float &l, float m2, float l2) {
    const float mn = fmaxf(m, m2);
    l = l * exp_below(m, mn) + l2 * exp_below(m2, mn);
    m = mn;
}

struct SoftmaxDenseArgs {
    const float *X;
    int ldx;
    const float *xb;
    int n_own;
    const float *Y;
    int ldy;
    const float *yb;
    int n_partner;
    float global_bias;
    int f, nslots;
    const float *lse, *W;  // of the users: the own rows' (LSE: written; users' DENSE: read) or the partners' (items' DENSE)
    float *lse_out;
    float *G;  // [n_own][ldg]
    int ldg;
};

// the part every dense kernel starts with: wavefront 0 stages the own tile
__device__ __forceinline__ void stage_own(const SoftmaxDenseArgs &a, float4 *xtile, int RS, int own0, int wave, int lane) {
    if (wave == 0) {
        stage_rows(xtile, a.X, a.ldx, own0, a.n_own, 0, a.nslots, RS, lane);
        wave_sync();
        zero_padding(xtile, RS, a.nslots, a.f, lane);
    }
}

// acc = this wavefront's 32 partners from part0 against the 32 own rows; pb = the partners' biases
__device__ __forceinline__ void score_block(const SoftmaxDenseArgs &a, float4 *ytile, const float4 *xtile, int RS, int part0, int lane,
                                            int r, int h, f32x16 &acc) {
    wave_sync();  // the previous step's reads of this wavefront's tile are done
    stage_rows(ytile, a.Y, a.ldy, part0, a.n_partner, 0, a.nslots, RS, lane);
    wave_sync();
    zero_padding(ytile, RS, a.nslots, a.f, lane);
    wave_sync();
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    contract(acc, ytile, xtile, RS, a.nslots, r, h);  // A: partners, B: own rows
}

__global__ __launch_bounds__(256) void softmax_lse_kernel(SoftmaxDenseArgs a) {
    extern __shared__ float4 softmax_smem[];
    const int RS = a.nslots | 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int own0 = blockIdx.x * kTile;
    float4 *xtile = softmax_smem, *ytile = softmax_smem + (1 + wave) * kTile * RS;
    stage_own(a, xtile, RS, own0, wave, lane);
    const float base = a.global_bias + (own0 + r < a.n_own ? a.xb[own0 + r] : 0.f);  // (gb + b_own), this lane's own row r
    float m_run = -INFINITY, l_run = 0.f;
    __syncthreads();  // the own tile is staged
    for (int part0 = wave * kTile; part0 < a.n_partner; part0 += kSoftmaxStep) {
        float pb[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) pb[reg] = a.yb[min(part0 + acc_row(reg, h), a.n_partner - 1)];
        f32x16 acc;
        score_block(a, ytile, xtile, RS, part0, lane, r, h, acc);
        float m = -INFINITY, l = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            acc[reg] = (base + pb[reg]) + acc[reg];
            if (part0 + acc_row(reg, h) < a.n_partner) m = fmaxf(m, acc[reg]);
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            if (part0 + acc_row(reg, h) < a.n_partner) l = l + exp_below(acc[reg], m);
        const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
        float ms = h ? mo : m, ls = h ? lo : l;  // half 0's pair first, in both lanes
        lse_merge(ms, ls, h ? m : mo, h ? l : lo);
        lse_merge(m_run, l_run, ms, ls);
    }
    __syncthreads();  // every wavefront is done with the tiles: the pairs overlay them
    float2 *red = reinterpret_cast<float2 *>(softmax_smem);  // [4][32]
    if (h == 0) red[wave * kTile + r] = make_float2(m_run, l_run);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kTile && own0 + t < a.n_own) {
        float m = red[t].x, l = red[t].y;
        for (int w = 1; w < 4; ++w) lse_merge(m, l, red[w * kTile + t].x, red[w * kTile + t].y);
        a.lse_out[own0 + t] = m + logf(l);
    }
}

template <int T, bool Items>
__global__ __launch_bounds__(256) void softmax_dense_kernel(SoftmaxDenseArgs a) {
    extern __shared__ float4 softmax_smem[];
    const int RS = a.nslots | 1, f = a.f;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int own0 = blockIdx.x * kTile;
    float4 *xtile = softmax_smem, *ytile = softmax_smem + (1 + wave) * kTile * RS;
    const float *yf = reinterpret_cast<const float *>(ytile);
    stage_own(a, xtile, RS, own0, wave, lane);
    const int own = min(own0 + r, a.n_own - 1);
    // the score's bits are the LSE pass's on both sides: ((gb + user bias) + item bias) + dot
    const float own_b = own0 + r < a.n_own ? a.xb[own] : 0.f;  // this lane's own row r
    [[maybe_unused]] const float base = a.global_bias + own_b;
    [[maybe_unused]] float l_own = 0.f;
    if constexpr (!Items) l_own = a.lse[own];
    f32x16 G[T];
#pragma unroll
    for (int b = 0; b < T; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) G[b][i] = 0.f;
    __syncthreads();  // the own tile is staged
    for (int part0 = wave * kTile; part0 < a.n_partner; part0 += kSoftmaxStep) {
        float pb[16];
        [[maybe_unused]] float pw[16], pl[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int part = min(part0 + acc_row(reg, h), a.n_partner - 1);
            pb[reg] = a.yb[part];
            if constexpr (Items) {
                pw[reg] = a.W[part];
                pl[reg] = a.lse[part];
            }
        }
        f32x16 acc;
        score_block(a, ytile, xtile, RS, part0, lane, r, h, acc);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float c;
            if constexpr (Items) c = pw[reg] * expf((((a.global_bias + pb[reg]) + own_b) + acc[reg]) - pl[reg]);
            else c = expf(((base + pb[reg]) + acc[reg]) - l_own);
            acc[reg] = part0 + acc_row(reg, h) < a.n_partner ? c : 0.f;
        }
#pragma unroll
        for (int b = 0; b < T; ++b) {
            const int col = 32 * b + r, cc = min(col, f - 1);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                float y = yf[acc_row(reg, h) * 4 * RS + cc];
                if (b == T - 1) y = col < f ? y : (col == f ? 1.f : 0.f);  // [Y | 1 | 0 ...]
                G[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[reg], y, G[b], 0, 0, 0);  // rows: own, columns: factors
            }
        }
    }
    __syncthreads();  // every wavefront is done with the tiles: the sums overlay them
    float *red = reinterpret_cast<float *>(softmax_smem);  // [4][T][16][64]
#pragma unroll
    for (int b = 0; b < T; ++b)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) red[((wave * T + b) * 16 + reg) * 64 + lane] = G[b][reg];
    __syncthreads();
    constexpr int per_wave = T * 16 * 64;
    for (int e = threadIdx.x; e < per_wave; e += 256) {
        const float v = ((red[e] + red[per_wave + e]) + red[2 * per_wave + e]) + red[3 * per_wave + e];
        const int l = e & 63, reg = (e >> 6) & 15, b = e >> 10;
        const int row = own0 + acc_row(reg, l >> 5), col = 32 * b + (l & 31);
        if (row < a.n_own) a.G[static_cast<size_t>(row) * a.ldg + col] = v;
    }
}

__global__ __launch_bounds__(256) void softmax_weights_kernel(const int *__restrict__ indptr, const float *__restrict__ data, int rows,
                                                              float *__restrict__ W) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= rows) return;
    float w = 0.f;
    for (int e = indptr[u]; e < indptr[u + 1]; ++e) w = w + data[e];
    W[u] = w;
}

struct SoftmaxRowArgs {
    LmfProblem p;
    const float *W;  // users: the own rows'
    float *grad;     // [n_own][ldg]
    int ldg;
    bool mass;  // users: column f keeps the dense pass's sum
};

// E = ceil((f + 1) / 64) elements per lane: element i = lane + 64 k is factor i, element f the bias
template <int E, bool Items>
__global__ __launch_bounds__(kRowThreads) void softmax_sparse_kernel(SoftmaxRowArgs a) {
    __shared__ float4 lds4[kRowWaves * 4 * 16 * E];
    constexpr int FS = 64 * E;
    const LmfProblem &p = a.p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int F = p.n_factors;
    float *part = reinterpret_cast<float *>(lds4) + wave * 4 * FS;
    for (int row = blockIdx.x * kRowWaves + wave; row < p.n_own; row += gridDim.x * kRowWaves) {
        const int lo = p.indptr[row], hi = p.indptr[row + 1];
        const float *x = p.X + static_cast<size_t>(row) * p.ldx;
        float4 acc[E];
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int e0 = lo; e0 < hi; e0 += 4) {  // group g takes entries g, g + 4, ... in ascending order
            const int e = e0 + g;
            const bool on = e < hi;
            const int ec = on ? e : hi - 1;
            const int idx = p.indices[ec];
            const float w = p.data[ec];
            float4 q[E];
#pragma unroll
            for (int k = 0; k < E; ++k) q[k] = load_partner4<true>(p.Y, p.ldy, F, idx, 4 * l16 + 64 * k);
            if (on) {
#pragma unroll
                for (int k = 0; k < E; ++k) axpy4(w, q[k], acc[k]);
            }
        }
        float t[E];
        wave_sync();  // the previous row has read part
        combine_groups<E>(acc, part, part + g * FS + 4 * l16, lane, t);
        float *gr = a.grad + static_cast<size_t>(row) * a.ldg;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = lane + 64 * k;
            if (i > F) continue;
            if constexpr (Items) {
                const float xi = i < F ? x[i] : p.xb[row];
                gr[i] = (t[k] - gr[i]) - (i < F ? p.reg : p.reg_bias) * xi;
            } else {
                if (i < F) gr[i] = (t[k] - a.W[row] * gr[i]) - p.reg * x[i];
                else if (!a.mass) gr[i] = 0.f;  // no bias gradient: lmf_step adds a zero
            }
        }
    }
}

// the entries' term and the three norms, a 16-lane group per entry / row, in double; partials[block][4]
__global__ __launch_bounds__(kObjThreads) void softmax_objective_kernel(LmfProblem p, const float *__restrict__ lse, int nnz,
                                                                        double *__restrict__ partials) {
    __shared__ double red[4][kObjThreads];
    const int tid = threadIdx.x, lane16 = tid & (kObjGroup - 1);
    const int group = (blockIdx.x * kObjThreads + tid) / kObjGroup, groups = gridDim.x * (kObjThreads / kObjGroup);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = group; k < nnz; k += groups) {
        const int u = row_of_entry(p.indptr, p.n_own, k), i = p.indices[k];
        const double dot = group_dot(p.X + static_cast<size_t>(u) * p.ldx, p.Y + static_cast<size_t>(i) * p.ldy, p.n_factors, lane16);
        const double sc = ((static_cast<double>(p.global_bias) + static_cast<double>(p.xb[u])) + static_cast<double>(p.yb[i])) + dot;
        if (lane16 == 0) s[0] += static_cast<double>(p.data[k]) * (sc - static_cast<double>(lse[u]));
    }
    for (int u = group; u < p.n_own; u += groups) {
        const float *x = p.X + static_cast<size_t>(u) * p.ldx;
        const double n2 = group_dot(x, x, p.n_factors, lane16);
        if (lane16 == 0) s[1] += n2;
    }
    for (int i = group; i < p.n_partner; i += groups) {
        const float *y = p.Y + static_cast<size_t>(i) * p.ldy;
        const double n2 = group_dot(y, y, p.n_factors, lane16);
        if (lane16 == 0) {
            s[2] += n2;
            s[3] += static_cast<double>(p.yb[i]) * static_cast<double>(p.yb[i]);
        }
    }
    block_reduce(s, red);
    if (tid == 0)
        for (int j = 0; j < 4; ++j) partials[4 * blockIdx.x + j] = red[j][0];
}

size_t dense_lds(int n_factors, int T) {
    const int nslots = (n_factors + 3) / 4;
    const size_t tiles = static_cast<size_t>(5) * kTile * (nslots | 1) * sizeof(float4);  // topk's five tiles: 161,280 B at f = 252
    const size_t sums = static_cast<size_t>(4) * T * 16 * 64 * sizeof(float);  // the four partial G (LSE: 128 pairs), overlaid
    return std::max(tiles, sums);
}

SoftmaxDenseArgs dense_args(const LmfProblem &p, const SoftmaxState &sm, float *G) {
    return {p.X, p.ldx, p.xb, p.n_own, p.Y, p.ldy, p.yb, p.n_partner, p.global_bias, p.n_factors, (p.n_factors + 3) / 4,
            sm.lse.ptr, sm.W.ptr, sm.lse.ptr, G, 32 * lmf_tiles(p.n_factors)};
}

template <class Kernel>
void launch_dense(Kernel kernel, const SoftmaxDenseArgs &a, int T, hipStream_t stream) {
    const size_t lds = dense_lds(a.f, T);
    if (lds > kMaxLds) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_softmax: the score tiles need more LDS than a workgroup has");
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(kernel), kMaxLds);
    hipLaunchKernelGGL(kernel, dim3((a.n_own + kTile - 1) / kTile), dim3(256), lds, stream, a);
    CU2REC_HIP(hipGetLastError());
}

}  // namespace

void softmax_lse(SoftmaxState &sm, const LmfProblem &users, hipStream_t stream) {
    const int n = users.n_own;
    if (n <= 0) return;
    if (sm.lse.count < static_cast<size_t>(n)) {
        sm.lse.allocate(n);
        sm.W.allocate(n);
    }
    hipLaunchKernelGGL(softmax_weights_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, users.indptr, users.data, n, sm.W.ptr);
    CU2REC_HIP(hipGetLastError());
    launch_dense(&softmax_lse_kernel, dense_args(users, sm, nullptr), 1, stream);
}

void softmax_gradient(LmfState &st, const SoftmaxState &sm, const LmfProblem &p, bool users, hipStream_t stream, bool mass) {
    if (p.n_own <= 0) return;
    const int T = lmf_tiles(p.n_factors), ldg = 32 * T;
    const size_t need = static_cast<size_t>(p.n_own) * ldg;
    if (st.grad.count < need) st.grad.allocate(need);
    const SoftmaxDenseArgs d = dense_args(p, sm, st.grad.ptr);
    dispatch_1_to_8(T, "cu2rec_model_softmax: n_factors above 252 is not supported", [&](auto tiles) {
        if (users) launch_dense(&softmax_dense_kernel<tiles(), false>, d, tiles(), stream);
        else launch_dense(&softmax_dense_kernel<tiles(), true>, d, tiles(), stream);
    });
    const SoftmaxRowArgs a{p, sm.W.ptr, st.grad.ptr, ldg, mass};
    dispatch_1_to_4(p.n_factors + 1, [&](auto elems) {
        if (users) hipLaunchKernelGGL((softmax_sparse_kernel<elems(), false>), dim3(row_grid(p.n_own)), dim3(kRowThreads), 0, stream, a);
        else hipLaunchKernelGGL((softmax_sparse_kernel<elems(), true>), dim3(row_grid(p.n_own)), dim3(kRowThreads), 0, stream, a);
    });
    CU2REC_HIP(hipGetLastError());
}

void softmax_objective_sums(LmfState &st, const SoftmaxState &sm, const LmfProblem &users, int nnz, double (&out)[4], hipStream_t stream) {
    const int blocks = objective_blocks(static_cast<size_t>(std::max(nnz, std::max(users.n_own, users.n_partner))));
    if (st.partials.count < 4 * static_cast<size_t>(blocks)) st.partials.allocate(4 * static_cast<size_t>(blocks));
    hipLaunchKernelGGL(softmax_objective_kernel, dim3(blocks), dim3(kObjThreads), 0, stream, users, sm.lse.ptr, nnz, st.partials.ptr);
    CU2REC_HIP(hipGetLastError());
    sum_block_partials(st.partials, blocks, out, stream);
}

}  // namespace cu2rec
