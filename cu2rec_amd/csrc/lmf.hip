// Logistic matrix factorization, full batch (lmf.hpp; include/cu2rec_amd.h: cu2rec_model_lmf).
//
// A half-step moves every own row x (a user, or an item on the item-major view) against the frozen partner side Y:
//   g  = sum_entries w (1 - sigma(s)) y  -  sum_(every partner) sigma(s) y  -  reg x,        w = alpha r
//   gb = sum_entries w (1 - sigma(s))    -  sum_(every partner) sigma(s)    -  reg_bias xb
// and then takes an AdaGrad step.  Three kernels:
//
// DENSE (lmf_dense_kernel): the all-pairs term is G = sigma(X Y^T) [Y | 1], never forming the own x partner matrix.  A workgroup
// owns 32 own rows, staged once, and walks the partner side 128 rows per step, one 32 x 32 block per wavefront, scored through
// score_tile.hpp exactly as topk_kernel's kItemUsers does: partners in the MFMA A operand, own rows in B, so that register `reg`
// of lane (r, h) holds the score of partner acc_row(reg, h) with own row r.  After sigma that register IS the A operand
// A[i = r][k = h] of a v_mfma_f32_32x32x2_f32 whose two K values are the partners acc_row(reg, 0) and acc_row(reg, 1): sixteen
// MFMAs per 32-column block of the partner tile still in LDS add sigma . y into G[own row][column], the B operand read as scalars
// from the tile, nothing moved across lanes.  Column f of the partner tile is the constant 1 (block T - 1 then carries sum sigma,
// the bias term); it is supplied in registers, not staged: at f = 252 a 253rd column would push the five tiles past topk's LDS
// budget.  The staged tiles' columns from f on are zeroed in LDS, so the model's padding floats never enter a score.  Each
// wavefront keeps T x 16 accumulator registers over its share of the partners (steps ascending, within a step the registers
// ascending, k = 0 before k = 1); the four partial sums go through LDS and are added in wave order.  Partners past n contribute
// exact zeros (sigma is replaced by 0 there).  The Objective instantiation replaces the second product by a sum of softplus(s) in
// double per lane, then per workgroup in thread order, the workgroups' partials added in block order on the host.
//
// SPARSE (lmf_sparse_kernel): one wavefront per own row gathers the row's entries in ascending stored order in the four groups of
// 16 lanes x float4 of row_wave.hpp's ENTRY map (column f a synthesised 1), accumulates w sigma(-s) [y | 1] per group, adds the four
// groups in group order and combines g = (sparse - dense) - reg x in place of the dense sums.
//
// STEP (lmf_step_kernel): one wavefront per row, element-wise float32: a' = a + g g, x' = x + (lr g) / sqrtf(a') where a' > 0.  A
// row with any non-finite gradient value, new value or new accumulator keeps all of its bits and is counted (integer atomic).
//
// Every sum's order is a function of the partner index or the entry position alone: no float atomics, bit-identical run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"
#include "lmf.hpp"
#include "logistic.hpp"
#include "objective_pass.hpp"
#include "row_wave.hpp"
#include "score_tile.hpp"

namespace cu2rec {

namespace {

constexpr int kLmfStep = 4 * kTile;  // partners scored per workgroup step

// columns f .. 4 nslots - 1 of a staged [32][RS] tile become zeros (by the wavefront that staged it)
__device__ __forceinline__ void zero_tail(float4 *tile, int RS, int nslots, int f, int lane) {
    const int keep = f - 4 * (nslots - 1);  // 1 .. 4 data floats in the last slot
    if (keep < 4 && lane < kTile) {
        float4 v = tile[lane * RS + nslots - 1];
        if (keep < 2) v.y = 0.f;
        if (keep < 3) v.z = 0.f;
        v.w = 0.f;
        tile[lane * RS + nslots - 1] = v;
    }
}

struct LmfDenseArgs {
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
    float *G;  // [n_own][ldg]
    int ldg;
    double *partials;  // Objective: one per workgroup
};

template <int T, bool Objective>
__global__ __launch_bounds__(256) void lmf_dense_kernel(LmfDenseArgs a) {
    extern __shared__ float4 lmf_smem[];
    const int RS = a.nslots | 1, f = a.f;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int own0 = blockIdx.x * kTile;
    float4 *xtile = lmf_smem, *ytile = lmf_smem + (1 + wave) * kTile * RS;
    const float *yf = reinterpret_cast<const float *>(ytile);
    if (wave == 0) {
        stage_rows(xtile, a.X, a.ldx, own0, a.n_own, 0, a.nslots, RS, lane);
        wave_sync();
        zero_tail(xtile, RS, a.nslots, f, lane);
    }
    const bool own_ok = own0 + r < a.n_own;
    const float base = a.global_bias + (own_ok ? a.xb[own0 + r] : 0.f);  // (gb + b_own), this lane's own row r
    [[maybe_unused]] f32x16 G[T];
    [[maybe_unused]] double sp = 0.0;
    if constexpr (!Objective) {
#pragma unroll
        for (int b = 0; b < T; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) G[b][i] = 0.f;
    }
    __syncthreads();  // the own tile is staged
    for (int part0 = wave * kTile; part0 < a.n_partner; part0 += kLmfStep) {
        float pb[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) pb[reg] = a.yb[min(part0 + acc_row(reg, h), a.n_partner - 1)];
        wave_sync();  // the previous step's reads of this wavefront's tile are done
        stage_rows(ytile, a.Y, a.ldy, part0, a.n_partner, 0, a.nslots, RS, lane);
        wave_sync();
        zero_tail(ytile, RS, a.nslots, f, lane);
        wave_sync();
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        contract(acc, ytile, xtile, RS, a.nslots, r, h);  // A: partners, B: own rows
        if constexpr (Objective) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float s = (base + pb[reg]) + acc[reg];
                if (own_ok && part0 + acc_row(reg, h) < a.n_partner) sp += lmf_softplus(static_cast<double>(s));
            }
        } else {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float s = (base + pb[reg]) + acc[reg];
                acc[reg] = part0 + acc_row(reg, h) < a.n_partner ? lmf_sigmoid(s) : 0.f;
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
    }
    __syncthreads();  // every wavefront is done with the tiles: the sums overlay them
    if constexpr (Objective) {
        double *red = reinterpret_cast<double *>(lmf_smem);
        red[threadIdx.x] = sp;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int t = 0; t < 256; ++t) s += red[t];
            a.partials[blockIdx.x] = s;
        }
    } else {
        float *red = reinterpret_cast<float *>(lmf_smem);  // [4][T][16][64]
#pragma unroll
        for (int b = 0; b < T; ++b)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) red[((wave * T + b) * 16 + reg) * 64 + lane] = G[b][reg];
        __syncthreads();
        constexpr int per_wave = T * 16 * 64;
        for (int e = threadIdx.x; e < per_wave; e += 256) {
            const float v = ((red[e] + red[per_wave + e]) + red[2 * per_wave + e]) + red[3 * per_wave + e];
            const int l = e & 63, reg = (e >> 6) & 15, b = e >> 10;
            const int own = own0 + acc_row(reg, l >> 5), col = 32 * b + (l & 31);
            if (own < a.n_own) a.G[static_cast<size_t>(own) * a.ldg + col] = v;
        }
    }
}

struct LmfRowArgs {
    LmfProblem p;
    float *grad;  // [n_own][ldg]
    int ldg;
    float *a, *ab;  // step: the own side's accumulators
    int *unchanged;
};

// E = ceil((f + 1) / 64) elements per lane: element i = lane + 64 k is factor i, element f the bias
template <int E>
__global__ __launch_bounds__(kRowThreads) void lmf_sparse_kernel(LmfRowArgs a) {
    __shared__ float4 lds4[kRowWaves * 5 * 16 * E];
    constexpr int FS = 64 * E;
    const LmfProblem &p = a.p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int F = p.n_factors;
    float *pv = reinterpret_cast<float *>(lds4) + wave * 5 * FS, *part = pv + FS;
    for (int row = blockIdx.x * kRowWaves + wave; row < p.n_own; row += gridDim.x * kRowWaves) {
        const int lo = p.indptr[row], hi = p.indptr[row + 1];
        const float *x = p.X + static_cast<size_t>(row) * p.ldx;
        float xr[E];
        wave_sync();  // the previous row has read pv and part
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int c = lane + 64 * k;
            xr[k] = c < F ? x[c] : 0.f;
            pv[c] = xr[k];  // zero from F on: the synthesised 1 of column F adds an exact 0 to the dot product
        }
        wave_sync();
        const float base = p.global_bias + p.xb[row];
        float4 v[E], acc[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            v[k] = *reinterpret_cast<const float4 *>(pv + 4 * l16 + 64 * k);
            acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int e0 = lo; e0 < hi; e0 += 4) {  // group g takes entries g, g + 4, ... in ascending order
            const int e = e0 + g;
            const bool on = e < hi;
            const int ec = on ? e : hi - 1;
            const int idx = p.indices[ec];
            const float w = p.alpha * p.data[ec];
            const float b = p.yb[idx];
            float4 q[E];
#pragma unroll
            for (int k = 0; k < E; ++k) q[k] = load_partner4<true>(p.Y, p.ldy, F, idx, 4 * l16 + 64 * k);
            const float d = group_dot4<E>(q, v);
            if (on) {
                const float s = (base + b) + d;
                const float c = w * lmf_sigmoid(-s);  // w (1 - sigma(s)), without the cancellation
#pragma unroll
                for (int k = 0; k < E; ++k) axpy4(c, q[k], acc[k]);
            }
        }
        float t[E];
        combine_groups<E>(acc, part, part + g * FS + 4 * l16, lane, t);
        float *gr = a.grad + static_cast<size_t>(row) * a.ldg;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = lane + 64 * k;
            if (i > F) continue;
            const float xi = i < F ? xr[k] : p.xb[row];
            gr[i] = (t[k] - gr[i]) - (i < F ? p.reg : p.reg_bias) * xi;
        }
    }
}

template <int E>
__global__ __launch_bounds__(kRowThreads) void lmf_step_kernel(LmfRowArgs a) {
    const LmfProblem &p = a.p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int F = p.n_factors;
    for (int row = blockIdx.x * kRowWaves + wave; row < p.n_own; row += gridDim.x * kRowWaves) {
        float *x = p.X + static_cast<size_t>(row) * p.ldx, *acc = a.a + static_cast<size_t>(row) * p.ldx;
        const float *gr = a.grad + static_cast<size_t>(row) * a.ldg;
        float xn[E], an[E];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = lane + 64 * k;
            xn[k] = an[k] = 0.f;
            if (i > F) continue;
            const float g = gr[i];
            const float x0 = i < F ? x[i] : p.xb[row], a0 = i < F ? acc[i] : a.ab[row];
            an[k] = a0 + g * g;
            xn[k] = an[k] > 0.f ? x0 + (p.lr * g) / sqrtf(an[k]) : x0;
            ok = ok && isfinite(g) && isfinite(xn[k]) && isfinite(an[k]);
        }
        if (__any(!ok)) {  // the row keeps its bits
            if (lane == 0) atomicAdd(a.unchanged, 1);
            continue;
        }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = lane + 64 * k;
            if (i < F) {
                x[i] = xn[k];
                acc[i] = an[k];
            } else if (i == F) {
                p.xb[row] = xn[k];
                a.ab[row] = an[k];
            }
        }
    }
}

// the entries' term and the four norms, a 16-lane group per entry / row, in double; partials[block][5]
__global__ __launch_bounds__(kObjThreads) void lmf_objective_kernel(LmfProblem p, int nnz, double *__restrict__ partials) {
    __shared__ double red[5][kObjThreads];
    const int tid = threadIdx.x, lane16 = tid & (kObjGroup - 1);
    const int group = (blockIdx.x * kObjThreads + tid) / kObjGroup, groups = gridDim.x * (kObjThreads / kObjGroup);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = group; k < nnz; k += groups) {
        const int u = row_of_entry(p.indptr, p.n_own, k), i = p.indices[k];
        const double dot = group_dot(p.X + static_cast<size_t>(u) * p.ldx, p.Y + static_cast<size_t>(i) * p.ldy, p.n_factors, lane16);
        const double sc = ((static_cast<double>(p.global_bias) + static_cast<double>(p.xb[u])) + static_cast<double>(p.yb[i])) + dot;
        const double w = static_cast<double>(p.alpha * p.data[k]);
        if (lane16 == 0) s[0] += w * (sc - lmf_softplus(sc));
    }
    for (int u = group; u < p.n_own; u += groups) {
        const float *x = p.X + static_cast<size_t>(u) * p.ldx;
        const double n2 = group_dot(x, x, p.n_factors, lane16);
        if (lane16 == 0) {
            s[1] += n2;
            s[2] += static_cast<double>(p.xb[u]) * static_cast<double>(p.xb[u]);
        }
    }
    for (int i = group; i < p.n_partner; i += groups) {
        const float *y = p.Y + static_cast<size_t>(i) * p.ldy;
        const double n2 = group_dot(y, y, p.n_factors, lane16);
        if (lane16 == 0) {
            s[3] += n2;
            s[4] += static_cast<double>(p.yb[i]) * static_cast<double>(p.yb[i]);
        }
    }
    block_reduce(s, red);
    if (tid == 0)
        for (int j = 0; j < 5; ++j) partials[5 * blockIdx.x + j] = red[j][0];
}

size_t dense_lds(int n_factors, int T) {
    const int nslots = (n_factors + 3) / 4;
    const size_t tiles = static_cast<size_t>(5) * kTile * (nslots | 1) * sizeof(float4);  // topk's five tiles: 161,280 B at f = 252
    const size_t sums = static_cast<size_t>(4) * T * 16 * 64 * sizeof(float);  // the four partial G (Objective: 256 doubles), overlaid
    return std::max(tiles, sums);
}

LmfDenseArgs dense_args(LmfState &st, const LmfProblem &p) {
    return {p.X, p.ldx, p.xb, p.n_own, p.Y, p.ldy, p.yb, p.n_partner, p.global_bias, p.n_factors, (p.n_factors + 3) / 4,
            st.grad.ptr, 32 * lmf_tiles(p.n_factors), st.partials.ptr};
}

template <int T, bool Objective>
void launch_dense(const LmfDenseArgs &a, hipStream_t stream) {
    const size_t lds = dense_lds(a.f, T);
    if (lds > kMaxLds) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_lmf: the score tiles need more LDS than a workgroup has");
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(&lmf_dense_kernel<T, Objective>), kMaxLds);
    hipLaunchKernelGGL((lmf_dense_kernel<T, Objective>), dim3((a.n_own + kTile - 1) / kTile), dim3(256), lds, stream, a);
    CU2REC_HIP(hipGetLastError());
}

}  // namespace

void lmf_gradient(LmfState &st, const LmfProblem &p, hipStream_t stream) {
    if (p.n_own <= 0) return;
    const int T = lmf_tiles(p.n_factors), ldg = 32 * T;
    const size_t need = static_cast<size_t>(p.n_own) * ldg;
    if (st.grad.count < need) st.grad.allocate(need);
    const LmfDenseArgs d = dense_args(st, p);
    dispatch_1_to_8(T, "cu2rec_model_lmf: n_factors above 252 is not supported", [&](auto tiles) { launch_dense<tiles(), false>(d, stream); });
    const LmfRowArgs a{p, st.grad.ptr, ldg, nullptr, nullptr, nullptr};
    dispatch_1_to_4(p.n_factors + 1, [&](auto elems) {
        hipLaunchKernelGGL((lmf_sparse_kernel<elems()>), dim3(row_grid(p.n_own)), dim3(kRowThreads), 0, stream, a);
    });
    CU2REC_HIP(hipGetLastError());
}

int lmf_step(LmfState &st, const LmfProblem &p, float *acc, float *acc_bias, hipStream_t stream) {
    if (p.n_own <= 0) return 0;
    if (!st.unchanged.ptr) st.unchanged.allocate(1);
    CU2REC_HIP(hipMemsetAsync(st.unchanged.ptr, 0, sizeof(int), stream));
    const LmfRowArgs a{p, st.grad.ptr, 32 * lmf_tiles(p.n_factors), acc, acc_bias, st.unchanged.ptr};
    dispatch_1_to_4(p.n_factors + 1, [&](auto elems) {
        hipLaunchKernelGGL((lmf_step_kernel<elems()>), dim3(row_grid(p.n_own)), dim3(kRowThreads), 0, stream, a);
    });
    CU2REC_HIP(hipGetLastError());
    int n = 0;
    CU2REC_HIP(hipMemcpyAsync(&n, st.unchanged.ptr, sizeof(int), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    return n;
}

double lmf_dense_objective(LmfState &st, const LmfProblem &p, hipStream_t stream) {
    if (p.n_own <= 0 || p.n_partner <= 0) return 0.0;
    const int blocks = (p.n_own + kTile - 1) / kTile;
    if (st.partials.count < static_cast<size_t>(blocks)) st.partials.allocate(blocks);
    const LmfDenseArgs d = dense_args(st, p);
    launch_dense<1, true>(d, stream);  // no second product: nothing depends on T
    double s[1];
    sum_block_partials(st.partials, blocks, s, stream);
    return s[0];
}

void lmf_sparse_objective(LmfState &st, const LmfProblem &p, int nnz, double (&out)[5], hipStream_t stream) {
    const int blocks = objective_blocks(static_cast<size_t>(std::max(nnz, std::max(p.n_own, p.n_partner))));
    if (st.partials.count < 5 * static_cast<size_t>(blocks)) st.partials.allocate(5 * static_cast<size_t>(blocks));
    hipLaunchKernelGGL(lmf_objective_kernel, dim3(blocks), dim3(kObjThreads), 0, stream, p, nnz, st.partials.ptr);
    CU2REC_HIP(hipGetLastError());
    sum_block_partials(st.partials, blocks, out, stream);
}

}  // namespace cu2rec
