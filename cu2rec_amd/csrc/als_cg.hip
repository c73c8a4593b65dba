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
// Two lane <-> element maps.  OWNER: lane l holds elements l, l + 64, ... of x, r, p, A p (E = ceil(f / 64) registers each); the
// G0 product reads column i of the symmetric G0 for element i, a chain over j = 0 .. f - 1.  ENTRY: the wavefront is four groups
// of 16 lanes, group g takes the row's entries e = g, g + 4, ... in ascending order, lane l16 of a group holds columns
// 4 l16 + 64 k .. + 3 of the gathered partner row; the dot product against v (kept in LDS per wavefront) is reduced over the 16
// lanes by a butterfly and w (q . v) q accumulated per group; the four groups' partial sums go through LDS and are added in group
// order.  Every sum's order is a function of the row's length and f alone: no float atomics, nothing that depends on which
// wavefront or workgroup picked the row up.
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

__device__ inline int cg_tri(int i) { return i * (i + 1) / 2; }

// G0 from the accumulator layout [tile pair][16][64] (tile pairs ti >= tj of the lower triangle, als.hip) to dense [f][S]; the
// upper triangle mirrors the lower one, the columns f .. S - 1 are zero
__global__ void cg_unpack_g0_kernel(const float *__restrict__ acc, float *__restrict__ dense, int f, int S) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= f * S) return;
    const int i = e / S, j = e - i * S;
    float v = 0.f;
    if (j < f) {
        const int a = max(i, j), b = min(i, j);
        const int ti = a >> 5, tj = b >> 5, ra = a & 31, r = b & 31;
        const int h = (ra >> 2) & 1, reg = (ra & 3) + 4 * (ra >> 3);  // acc_row(reg, h) == ra
        v = acc[(static_cast<size_t>(cg_tri(ti) + tj) * 16 + reg) * 64 + r + 32 * h];
    }
    dense[e] = v;
}

// the wavefront's LDS traffic is its own: order it for the compiler and the memory model, no instruction is needed beyond that
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// sum over the wavefront, the same bits in every lane (a butterfly: both partners add the same two values)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

template <int E>
__device__ __forceinline__ float owner_dot(const float (&a)[E], const float (&b)[E]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) s = fmaf(a[k], b[k], s);
    return wave_sum(s);
}

// partner row `idx`, columns c0 .. c0 + 3 (c0 < 64 E), zero from column F on: the padding floats are never read as data.
// AlsKind::Explicit: column F is the constant 1 of z = [q; 1], synthesised here
template <AlsKind K>
__device__ __forceinline__ float4 load_q(const AlsProblem &p, int idx, int c0) {
    const int F = p.n_factors;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < F) {
        v = *reinterpret_cast<const float4 *>(p.X + static_cast<size_t>(idx) * p.ldx + c0);
        if (c0 + 1 >= F) v.y = 0.f;
        if (c0 + 2 >= F) v.z = 0.f;
        if (c0 + 3 >= F) v.w = 0.f;
    }
    if constexpr (K == AlsKind::Explicit) {
        if (c0 == F) v.x = 1.f;
        if (c0 + 1 == F) v.y = 1.f;
        if (c0 + 2 == F) v.z = 1.f;
        if (c0 + 3 == F) v.w = 1.f;
    }
    return v;
}

// ENTRY pass over entries [lo, hi): t = sum_e w_e (q_e . v) q_e with v read from pv; FIRST: also b = sum_e (1 + w_e) q_e.
// AlsKind::Explicit: t = sum_e (z_e . v) z_e and b = sum_e t_e z_e.  Results in the OWNER map.  part: the wavefront's [4][64 E] floats.
template <int E, bool FIRST, AlsKind K>
__device__ __forceinline__ void entry_pass(const CgArgs &a, int lo, int hi, const float *pv, float *part, float (&t)[E],
                                           float (&b)[E]) {
    constexpr int FS = 64 * E;
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
            for (int k = 0; k < E; ++k) q[u][k] = load_q<K>(a.p, idx, 4 * l16 + 64 * k);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float d = 0.f;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                d = fmaf(q[u][k].x, v[k].x, d);
                d = fmaf(q[u][k].y, v[k].y, d);
                d = fmaf(q[u][k].z, v[k].z, d);
                d = fmaf(q[u][k].w, v[k].w, d);
            }
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) d = d + __shfl_xor(d, m, 16);
            if (on[u]) {
                const float s = K == AlsKind::Implicit ? w[u] * d : d;
                [[maybe_unused]] const float bw = K == AlsKind::Implicit ? 1.f + w[u] : w[u];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    acc[k].x = fmaf(s, q[u][k].x, acc[k].x);
                    acc[k].y = fmaf(s, q[u][k].y, acc[k].y);
                    acc[k].z = fmaf(s, q[u][k].z, acc[k].z);
                    acc[k].w = fmaf(s, q[u][k].w, acc[k].w);
                    if constexpr (FIRST) {
                        bacc[k].x = fmaf(bw, q[u][k].x, bacc[k].x);
                        bacc[k].y = fmaf(bw, q[u][k].y, bacc[k].y);
                        bacc[k].z = fmaf(bw, q[u][k].z, bacc[k].z);
                        bacc[k].w = fmaf(bw, q[u][k].w, bacc[k].w);
                    }
                }
            }
        }
    }
    // the four groups' sums, added in group order
    wave_sync();
#pragma unroll
    for (int k = 0; k < E; ++k) *reinterpret_cast<float4 *>(part + g * FS + 4 * l16 + 64 * k) = acc[k];
    wave_sync();
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = lane + 64 * k;
        t[k] = ((part[i] + part[FS + i]) + part[2 * FS + i]) + part[3 * FS + i];
    }
    if constexpr (FIRST) {
        wave_sync();
#pragma unroll
        for (int k = 0; k < E; ++k) *reinterpret_cast<float4 *>(part + g * FS + 4 * l16 + 64 * k) = bacc[k];
        wave_sync();
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = lane + 64 * k;
            b[k] = ((part[i] + part[FS + i]) + part[2 * FS + i]) + part[3 * FS + i];
        }
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

// every row of the side, kCgWaves per workgroup; elems: the per-lane element count E of the system's order
template <AlsKind K>
void launch_cg_rows(const CgArgs &a, int elems, hipStream_t stream) {
    if (a.rows <= 0) return;
    const int grid = std::min((a.rows + kCgWaves - 1) / kCgWaves, kCgMaxBlocks);
    switch (elems) {
        case 1: launch_cg<1, K>(a, grid, stream); break;
        case 2: launch_cg<2, K>(a, grid, stream); break;
        case 3: launch_cg<3, K>(a, grid, stream); break;
        default: launch_cg<4, K>(a, grid, stream); break;
    }
}

}  // namespace

void ials_cg_short_rows(AlsCache &c, const AlsSide &side, const AlsProblem &p, int max_rows, int cg_steps, hipStream_t stream) {
    const int F = p.n_factors, S = (F + 3) & ~3;
    if (F < 1 || F > kAlsMaxFactors) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_als_implicit_cg: n_factors above 252 is not supported");
    const size_t dense = static_cast<size_t>(F) * S;
    if (c.g0_dense.count < dense) c.g0_dense.allocate(dense);
    const int threads = 256;
    hipLaunchKernelGGL(cg_unpack_g0_kernel, dim3(static_cast<unsigned>((dense + threads - 1) / threads)), dim3(threads), 0, stream,
                       c.g0.ptr, c.g0_dense.ptr, F, S);
    CU2REC_HIP(hipGetLastError());
    CgArgs a{side.indptr, side.indices, side.data, p, c.g0_dense.ptr, S, std::min(side.rows, max_rows), cg_steps, c.unsolved.ptr};
    launch_cg_rows<AlsKind::Implicit>(a, (F + 63) / 64, stream);
}

void als_cg_short_rows(AlsCache &c, const AlsSide &side, const AlsProblem &p, int max_rows, int cg_steps, hipStream_t stream) {
    const int F = p.n_factors;
    if (F < 1 || F > kAlsMaxFactors) fail(CU2REC_EUNSUPPORTED, "cu2rec_model_als_cg: n_factors above 252 is not supported");
    CgArgs a{side.indptr, side.indices, side.data, p, nullptr, 0, std::min(side.rows, max_rows), cg_steps, c.unsolved.ptr};
    launch_cg_rows<AlsKind::Explicit>(a, (F + 1 + 63) / 64, stream);  // order f + 1 <= 253: E <= 4
}

}  // namespace cu2rec
