// The conjugate-gradient form of the implicit-feedback half-step (als.hpp: ials_cg_short_rows; include/cu2rec_amd.h:
// cu2rec_model_als_implicit_cg).  Takacs, Pilaszy, Tikk: Applications of the conjugate gradient method for implicit feedback
// collaborative filtering (RecSys 2011): a few CG steps per row on A x = b, warm-started from the row's current factors, with
//   A v = G0 v + sum_e w_e (q_e . v) q_e + reg v,   b = sum_e (1 + w_e) q_e
// applied as an operator -- the row's Gram is never formed.
//
// One wavefront per row, kCgWaves rows per workgroup, the workgroups grid-striding over the rows.  G0 arrives in the accumulator
// layout of als.hip and is unpacked once per half-step into a dense f x S matrix (S = f rounded up to 4); a workgroup stages it
// into LDS once up to f = 128 (64 KiB) and reads it from L2 otherwise.  After that one barrier the wavefronts never
// meet again.
//
// The two lane <-> element maps of row_wave.hpp.  OWNER: x, r, p, A p (E = ceil(f / 64) registers each); the G0 product reads
// column i of the symmetric G0 for element i, a chain over j = 0 .. f - 1.  ENTRY: the gathered partner rows, two entries per group
// in flight; the dot product is against v (kept in LDS per wavefront), and w (q . v) q is accumulated per group.  Every sum's order
// is a function of the row's length and f alone: no float atomics, nothing that depends on which wavefront or workgroup picked the
// row up.
//
// The explicit half-step (als.hpp: als_cg_short_rows; cu2rec_model_als_cg) is the AlsKind::Explicit case of the same templates: the
// system has order D = f + 1, x = [factors; bias], z_e = [q_e; 1] and
//   A v = sum_e (z_e . v) z_e + n diag(reg, ..., reg, reg_bias) v,   b = sum_e t_e z_e,   t_e = (r_e - gb) - the partner's bias.
// OWNER: E = ceil((f + 1) / 64), the bias is element f.  ENTRY: the same gather with column f a synthesised 1.0 (never loaded, also
// where f is a multiple of 4 and column f starts a float4 of its own); the per-entry scalar is (z . v), the right-hand side's
// weight t.  There is no G0: nothing is unpacked or staged, the diagonal term is formed in registers, and the kernel has no
// workgroup barrier at all.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "als.hpp"
#include "kernels.hpp"
#include "mfma_f32.hpp"
#include "row_wave.hpp"

namespace cu2rec {

namespace {

constexpr int kCgThreads = 256, kCgWaves = kCgThreads / 64;
constexpr int kCgMaxBlocks = 2048;             // rows beyond kCgWaves x this many take another trip of the grid-stride loop
constexpr int kCgLdsElems = 2;                 // the dense G0 is staged into LDS up to E = 2 elements per lane (f <= 128: 64 KiB)

struct CgArgs {
    const int *indptr, *indices;
    const float *data;
    AlsProblem p;
    const float *g0;  // dense, symmetric: [f][S] (AlsKind::Implicit only)
    int S, rows, steps;
    int *unsolved;
};

// G0 from the accumulator layout [tile pair][16][64] (tile pairs ti >= tj of the lower triangle, als.hip) to dense [f][S]; the
// upper triangle mirrors the lower one, the columns f .. S - 1 are zero
__global__ void cg_unpack_g0_kernel(const float *__restrict__ acc, float *__restrict__ dense, int f, int S) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= f * S) return;
    const int i = e / S, j = e - i * S;
    float v = 0.f;
    if (j < f) {
        const int a = max(i, j), b = min(i, j);
        const int ti = a >> 5, tj = b >> 5, r = b & 31;
        int reg, h;
        acc_reg_of_row(a & 31, reg, h);
        v = acc[(static_cast<size_t>(tri(ti) + tj) * 16 + reg) * 64 + r + 32 * h];
    }
    dense[e] = v;
}

template <int E>
__device__ __forceinline__ float owner_dot(const float (&a)[E], const float (&b)[E]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) s = fmaf(a[k], b[k], s);
    return wave_sum(s);
}

// ENTRY pass over entries [lo, hi): t = sum_e w_e (q_e . v) q_e with v read from pv; FIRST: also b = sum_e (1 + w_e) q_e.
// AlsKind::Explicit: t = sum_e (z_e . v) z_e and b = sum_e t_e z_e.  Results in the OWNER map.  part: the wavefront's [4][64 E] floats.
template <int E, bool FIRST, AlsKind K>
__device__ __forceinline__ void entry_pass(const CgArgs &a, int lo, int hi, const float *pv, float *part, float (&t)[E],
                                           float (&b)[E]) {
    const int lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    float4 v[E], acc[E], bacc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        v[k] = *reinterpret_cast<const float4 *>(pv + 4 * l16 + 64 * k);
        acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        bacc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int e0 = lo; e0 < hi; e0 += 8) {  // two entries per group in flight; each group still adds its entries in ascending order
        float4 q[2][E];
        float w[2];  // the entry's weight; AlsKind::Explicit: its right-hand side weight t (read by the first pass only)
        bool on[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = e0 + 4 * u + g;
            on[u] = e < hi;
            const int ec = on[u] ? e : hi - 1;
            const int idx = a.indices[ec];
            if constexpr (K == AlsKind::Implicit) w[u] = a.p.alpha * a.data[ec];
            else if constexpr (FIRST) w[u] = (a.data[ec] - a.p.global_bias) - a.p.xb[idx];
            else w[u] = 0.f;
#pragma unroll
            for (int k = 0; k < E; ++k) q[u][k] = load_partner4<K == AlsKind::Explicit>(a.p.X, a.p.ldx, a.p.n_factors, idx, 4 * l16 + 64 * k);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float d = group_dot4<E>(q[u], v);
            if (on[u]) {
                const float s = K == AlsKind::Implicit ? w[u] * d : d;
                [[maybe_unused]] const float bw = K == AlsKind::Implicit ? 1.f + w[u] : w[u];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    axpy4(s, q[u][k], acc[k]);
                    if constexpr (FIRST) axpy4(bw, q[u][k], bacc[k]);
                }
            }
        }
    }
    float *mine = part + g * (64 * E) + 4 * l16;
    wave_sync();  // the previous pass has read part
    combine_groups<E>(acc, part, mine, lane, t);
    if constexpr (FIRST) {
        wave_sync();
        combine_groups<E>(bacc, part, mine, lane, b);
    }
}

// A v in the OWNER map: the G0 product (element i: the chain over j of G0[j][i] v[j], G0 symmetric), + t + reg v.  v is read from
// pv (all of its 64 E floats are written, zero from f on) and, for the reg term, from the lane's own registers.
template <int E>
__device__ __forceinline__ void apply_a(const CgArgs &a, const float *G, const float *pv, const float (&t)[E], const float (&v)[E],
                                        float (&out)[E]) {
    const int lane = threadIdx.x & 63, F = a.p.n_factors, S = a.S;
    int col[E];
    float s[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        col[k] = min(lane + 64 * k, F - 1);
        s[k] = 0.f;
    }
    for (int j0 = 0; j0 < F; j0 += 4) {  // S is a multiple of 4 and pv is zero from F on: the rows j0 .. j0 + 3 < S exist in G
        const float4 vj = *reinterpret_cast<const float4 *>(pv + j0);
        const float *gj = G + j0 * S;
        const bool full = j0 + 3 < F;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            s[k] = fmaf(gj[col[k]], vj.x, s[k]);
            if (full) {
                s[k] = fmaf(gj[S + col[k]], vj.y, s[k]);
                s[k] = fmaf(gj[2 * S + col[k]], vj.z, s[k]);
                s[k] = fmaf(gj[3 * S + col[k]], vj.w, s[k]);
            } else {
                if (j0 + 1 < F) s[k] = fmaf(gj[S + col[k]], vj.y, s[k]);
                if (j0 + 2 < F) s[k] = fmaf(gj[2 * S + col[k]], vj.z, s[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) out[k] = lane + 64 * k < F ? (s[k] + t[k]) + a.p.reg * v[k] : 0.f;
}

// the explicit system's A v in the OWNER map: t + n diag(reg, ..., reg, reg_bias) v for a row of n ratings, zero from f + 1 on
template <int E>
__device__ __forceinline__ void apply_a_explicit(const CgArgs &a, int n, const float (&t)[E], const float (&v)[E], float (&out)[E]) {
    const int lane = threadIdx.x & 63, F = a.p.n_factors;
    const float nf = static_cast<float>(n);
    const float nreg = nf * a.p.reg, nreg_bias = nf * a.p.reg_bias;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int c = lane + 64 * k;
        out[k] = c <= F ? fmaf(c < F ? nreg : nreg_bias, v[k], t[k]) : 0.f;
    }
}

template <int E>
__device__ __forceinline__ void put_v(float *pv, const float (&v)[E]) {
    const int lane = threadIdx.x & 63;
    wave_sync();  // the previous pass has read pv
#pragma unroll
    for (int k = 0; k < E; ++k) pv[lane + 64 * k] = v[k];
    wave_sync();
}

template <int E, AlsKind K>
__global__ __launch_bounds__(kCgThreads) void als_cg_kernel(CgArgs a) {
    extern __shared__ float4 cg_smem[];
    constexpr int FS = 64 * E;
    constexpr bool explicit_kind = K == AlsKind::Explicit;
    constexpr bool G0_IN_LDS = !explicit_kind && E <= kCgLdsElems;
    float *lds = reinterpret_cast<float *>(cg_smem);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int F = a.p.n_factors;
    [[maybe_unused]] const int S = a.S;
    [[maybe_unused]] const float *G = a.g0;
    float *wave_lds = lds;
    if constexpr (G0_IN_LDS) {
        const int n4 = F * S / 4;
        const float4 *src = reinterpret_cast<const float4 *>(a.g0);
        for (int e = tid; e < n4; e += kCgThreads) cg_smem[e] = src[e];
        G = lds;
        wave_lds = lds + F * S;  // F S is a multiple of 4 floats: 16-byte aligned
        __syncthreads();         // the only workgroup barrier
    }
    float *pv = wave_lds + wave * 5 * FS, *part = pv + FS;
    for (int row = blockIdx.x * kCgWaves + wave; row < a.rows; row += gridDim.x * kCgWaves) {
        const int lo = a.indptr[row], hi = a.indptr[row + 1];
        float *y = a.p.Y + static_cast<size_t>(row) * a.p.ldy;
        if (hi <= lo) {  // right-hand side 0: the zero row, not counted; AlsKind::Explicit: the row keeps its values
            if constexpr (!explicit_kind) {
                for (int c = lane; c < a.p.ldy; c += 64) y[c] = 0.f;
                if (lane == 0) a.p.yb[row] = 0.f;
            }
            continue;
        }
        if (hi - lo > kAlsChunk) continue;  // the long rows are solved exactly by the chunk -> long kernels
        float x[E], r[E], p[E], ap[E], t[E], b[E];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int c = lane + 64 * k;
            x[k] = c < F ? y[c] : 0.f;
            if constexpr (explicit_kind)
                if (c == F) x[k] = a.p.yb[row];  // element f: the row's bias
            finite = finite && isfinite(x[k]);
        }
        if (__any(!finite)) {
#pragma unroll
            for (int k = 0; k < E; ++k) x[k] = 0.f;
        }
        put_v<E>(pv, x);
        entry_pass<E, true, K>(a, lo, hi, pv, part, t, b);
        if constexpr (explicit_kind) apply_a_explicit<E>(a, hi - lo, t, x, ap);
        else apply_a<E>(a, G, pv, t, x, ap);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            r[k] = b[k] - ap[k];
            p[k] = r[k];
        }
        float rho = owner_dot<E>(r, r);
        bool ok = isfinite(rho);
        for (int step = 0; ok && step < a.steps; ++step) {  // rho, d: the same bits in every lane, the exits are uniform
            if (rho == 0.f) break;
            put_v<E>(pv, p);
            entry_pass<E, false, K>(a, lo, hi, pv, part, t, b);
            if constexpr (explicit_kind) apply_a_explicit<E>(a, hi - lo, t, p, ap);
            else apply_a<E>(a, G, pv, t, p, ap);
            const float d = owner_dot<E>(p, ap);
            if (!(isfinite(d) && d >= 0.f)) {
                ok = false;
                break;
            }
            if (d == 0.f) break;
            const float alpha = rho / d;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                x[k] = fmaf(alpha, p[k], x[k]);
                r[k] = fmaf(-alpha, ap[k], r[k]);
            }
            const float rho1 = owner_dot<E>(r, r);
            if (!isfinite(rho1)) {
                ok = false;
                break;
            }
            const float beta = rho1 / rho;
#pragma unroll
            for (int k = 0; k < E; ++k) p[k] = fmaf(beta, p[k], r[k]);
            rho = rho1;
        }
        finite = true;
#pragma unroll
        for (int k = 0; k < E; ++k) finite = finite && isfinite(x[k]);
        if (!ok || __any(!finite)) {  // the row keeps its bits
            if (lane == 0) atomicAdd(a.unsolved, 1);
            continue;
        }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int c = lane + 64 * k;
            if (c < a.p.ldy) y[c] = c < F ? x[k] : 0.f;
            if constexpr (explicit_kind)
                if (c == F) a.p.yb[row] = x[k];
        }
        for (int c = lane + FS; c < a.p.ldy; c += 64) y[c] = 0.f;
        if constexpr (!explicit_kind)
            if (lane == 0) a.p.yb[row] = 0.f;
    }
}

template <int E, AlsKind K>
void launch_cg(const CgArgs &a, int grid, hipStream_t stream) {
    const size_t g_bytes = K == AlsKind::Implicit && E <= kCgLdsElems ? static_cast<size_t>(a.p.n_factors) * a.S * sizeof(float) : 0;
    const size_t bytes = g_bytes + static_cast<size_t>(kCgWaves) * 5 * 64 * E * sizeof(float);  // explicit: 20 KiB at most
    if constexpr (K == AlsKind::Implicit) ensure_max_dynamic_lds(reinterpret_cast<const void *>(&als_cg_kernel<E, K>), 160 * 1024);
    hipLaunchKernelGGL((als_cg_kernel<E, K>), dim3(grid), dim3(kCgThreads), bytes, stream, a);
    CU2REC_HIP(hipGetLastError());
}

// every row of the side, kCgWaves per workgroup; order: of the row's system, E = ceil(order / 64) elements per lane
template <AlsKind K>
void launch_cg_rows(const CgArgs &a, int order, hipStream_t stream) {
    if (a.rows <= 0) return;
    const int grid = std::min((a.rows + kCgWaves - 1) / kCgWaves, kCgMaxBlocks);
    dispatch_1_to_4(order, [&](auto elems) { launch_cg<elems(), K>(a, grid, stream); });
}

}  // namespace

void als_unpack_gram(const float *acc, float *dense, int f, int S, hipStream_t stream) {
    const int threads = 256;
    hipLaunchKernelGGL(cg_unpack_g0_kernel, dim3(static_cast<unsigned>((static_cast<size_t>(f) * S + threads - 1) / threads)), dim3(threads), 0,
                       stream, acc, dense, f, S);
    CU2REC_HIP(hipGetLastError());
}

void ials_cg_short_rows(AlsCache &c, const AlsSide &side, const AlsProblem &p, int max_rows, int cg_steps, hipStream_t stream) {
    const int F = p.n_factors, S = (F + 3) & ~3;
    if (F < 1 || F > kAlsMaxFactors) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_als_implicit_cg: n_factors above 252 is not supported");
    const size_t dense = static_cast<size_t>(F) * S;
    if (c.g0_dense.count < dense) c.g0_dense.allocate(dense);
    als_unpack_gram(c.g0.ptr, c.g0_dense.ptr, F, S, stream);
    CgArgs a{side.indptr, side.indices, side.data, p, c.g0_dense.ptr, S, std::min(side.rows, max_rows), cg_steps, c.unsolved.ptr};
    launch_cg_rows<AlsKind::Implicit>(a, F, stream);
}

void als_cg_short_rows(AlsCache &c, const AlsSide &side, const AlsProblem &p, int max_rows, int cg_steps, hipStream_t stream) {
    const int F = p.n_factors;
    if (F < 1 || F > kAlsMaxFactors) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_als_cg: n_factors above 252 is not supported");
    CgArgs a{side.indptr, side.indices, side.data, p, nullptr, 0, std::min(side.rows, max_rows), cg_steps, c.unsolved.ptr};
    launch_cg_rows<AlsKind::Explicit>(a, F + 1, stream);  // order f + 1 <= 253: E <= 4
}

}  // namespace cu2rec
