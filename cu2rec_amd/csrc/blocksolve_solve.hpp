// ---- phase 2: the chains ----------------------------------------------------------------------------------------------
// Workgroup = one hot chain: one solver wavefront (lane = link) and four loader wavefronts.
//   solver: per block  d = P_blk q (every lane its own row against the item row, broadcast from LDS),
//           rhs -> e = M rhs (every lane its row of M against rhs, broadcast from LDS), then the item row's columns
//           (lane = column) collect sum_k w_k P_blk[k][column].  No global loads in the loop, no exchange with other
//           wavefronts; one __syncthreads() per block hands over the next LDS slot.
//   loader: streams each block's 64 user rows, factor tiles and base errors global -> registers -> LDS ring of two slots,
//           kDepth blocks in flight in the register file: a chain of n links moves n * (4f + 196) bytes through ONE
//           CU's load path, and that is what a long chain takes.
// (the plain form's copy of the decay tables in LDS: powers 0 .. 64 only -- at 63 slots a row its LDS has no room for more)
#pragma once

#include "blocksolve_device.hpp"

namespace cu2rec {
namespace bs_dev {

constexpr int kSolTabStride = kB + 1, kSolTabFloats = 4 * kSolTabStride;
constexpr int kSolTabAdel = 0, kSolTabCdel = kSolTabStride, kSolTabApow = 2 * kSolTabStride, kSolTabCpow = 3 * kSolTabStride;
constexpr int kRing = 2;   // LDS slots: the block being solved and the next one
constexpr int kDepth = 4;  // blocks a loader keeps in flight

template <int N>
struct Stage {  // one loader thread's share of a block
    f32x4 rows[N];
    f32x4 m4[3];
    float base;
    uint64_t next_val;  // the thread's schedule entry of the block this stage loads next (kDepth blocks on)
};

// LDS slot: [kB][RS] float4 user rows | three factor tiles, rows of kMS floats (column 32 of the first 64 rows: the base error)
__host__ __device__ inline int solve_slot_f4(int nslots) { return kB * (nslots | 1) + 3 * kH * kMS / 4; }

// after the ring: the item row (4 * sw + 8 float4, zero beyond the row), the partial dots and errors, four copies of rhs
// and w, the decay tables, a row of zeros
__host__ __device__ inline size_t solve_lds_bytes(int nslots, int sw) {
    return (static_cast<size_t>(kRing) * solve_slot_f4(nslots) + 4 * sw + 8 + 2 * kB + 8 * kB / 4 + (kSolTabFloats + 3) / 4 + 8 + 1) * 16;
}

// The four solver wavefronts meet twice inside a block; s_barrier would drag the loaders along (their work of an interval
// -- 25 KB of LDS writes, a few hundred cache-line requests -- would then sit on the chain's critical path), so they count
// arrivals in LDS instead.  LDS operations of a wavefront complete in order: the partial results written before the
// ds_add are visible to whoever sees the count.
__device__ __forceinline__ void solvers_meet(unsigned *meet, unsigned target, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_fetch_add(meet, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (__hip_atomic_load(meet, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Eight wavefronts: four solvers (one per SIMD) and four loaders.
//   loaders: stream the chain's blocks (64 user rows, the factor tiles, the base errors) into a ring of two LDS slots,
//            kDepth blocks in flight in their registers; every load unconditional at a clamped address.
//   solvers: all four hold the same 64 links (lane = link) and split every step of a block four ways:
//     (A) d_k = p_k . q      each wavefront a quarter of the row (SW slots), partial sums through LDS            -- meet
//     (B) e = M rhs          each wavefront 16 columns of M (rhs is cheap and computed four times), partials     -- meet
//     (C) q <- a^n q + sum_k w_k p_k   each wavefront its quarter of the row: lane = (slot, group of 8 links), the
//                            eight groups summed across lanes (DPP row rotate, permlane16/32 swaps)              -- barrier
//            (the barrier is the one per block all eight wavefronts share: it hands the ring slot back to the loaders)
//   One wavefront doing all of it issued ~500 instructions per block and took 1.35 us of the block's 1.8 us; the
//   loaders alone sustain a block per 0.42 us (measured by ablation, profiles/README.md).
// SW: float4 slots per row quarter (4 * SW >= nslots).
template <int SW>
__device__ __forceinline__ void solve_chain(const SgdArgs &a, const BsIteration &it, float4 *bs_smem, const BsChainDesc &cd) {
    const int begin = cd.begin, len = cd.len;
    if (len <= 0) return;  // workgroup uniform
    const int nblk = (len + kB - 1) / kB;
    const int g0 = cd.blk0;
    const int nslots = a.nslots, RS = nslots | 1;  // odd row stride (in float4): conflict-free ds_read_b128 down a column
    const int S4 = solve_slot_f4(nslots);
    const bool long_chain = nblk > kDepth;
    const int n_intervals = long_chain ? (nblk + kDepth - 1) / kDepth * kDepth : kDepth;  // both roles: 3 barriers each
    float4 *smem = bs_smem;
    const int tid = threadIdx.x;

    if (tid >= 256) {
        // ------------------------------------------------------------------------------------------ loader
        __builtin_amdgcn_s_setprio(2);
        constexpr int NLT = SW;  // float4 per loader thread and block: slots tp, tp + 4, ...
        const int lt = tid - 256, tr = lt >> 2, tp = lt & 3;
        auto load_val = [&](int t) -> uint64_t { return it.vals[begin + min(kB * t + tr, len - 1)]; };
        // every load is unconditional (clamped addresses): a branch or a predicated load inside the ring would make the
        // compiler's s_waitcnt pass fall back to vmcnt(0) and serialise the ring
        auto issue_rows = [&](Stage<NLT> &s, int t, uint64_t val) {  // the schedule and the user rows: nothing phase 1 writes
            s.next_val = load_val(t + kDepth);
            const f32x4 *row = reinterpret_cast<const f32x4 *>(a.P + static_cast<size_t>(static_cast<uint32_t>(val >> 32)) * a.ldp);
#pragma unroll
            for (int i = 0; i < NLT; ++i) s.rows[i] = row[min(tp + 4 * i, nslots - 1)];
        };
        auto issue_rec = [&](Stage<NLT> &s, int t) {  // phase 1's record of the block
            const float *rec = it.Mbuf + static_cast<size_t>(g0 + min(t, nblk - 1)) * kBsRecFloats;
            const f32x4 *mg = reinterpret_cast<const f32x4 *>(rec);
#pragma unroll
            for (int q = 0; q < 3; ++q) s.m4[q] = mg[q * 256 + lt];
            s.base = rec[kBsFactorFloats + (lt & 63)];
        };
        auto issue = [&](Stage<NLT> &s, int t, uint64_t val) {
            issue_rows(s, t, val);
            issue_rec(s, t);
        };
        auto commit = [&](const Stage<NLT> &s, int t) {  // block t -> ring slot t % kRing; links beyond the chain: zero rows
            f32x4 *sl = reinterpret_cast<f32x4 *>(smem + (t % kRing) * S4);
            const bool rv = kB * t + tr < len;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NLT; ++i) {
                const int slot = tp + 4 * i;
                if (slot < nslots) sl[tr * RS + slot] = rv ? s.rows[i] : z;
            }
            f32x4 *mt = sl + kB * RS;  // three tiles of 32 rows x 8 float4, rows kMS floats apart
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int item = q * 256 + lt;  // float4 number inside the block's factor
                mt[(item >> 3) * (kMS / 4) + (item & 7)] = s.m4[q];
            }
            if (lt < kB) reinterpret_cast<float *>(mt)[lt * kMS + kH] = kB * t + lt < len ? s.base : 0.f;
        };
        Stage<NLT> st[kDepth];
        if (long_chain) {
            uint64_t v[kDepth];
#pragma unroll
            for (int t = 0; t < kDepth; ++t) v[t] = load_val(t);
#pragma unroll
            for (int t = 0; t < kDepth; ++t) issue(st[t], t, v[t]);
            commit(st[0], 0);
            issue(st[0], kDepth, st[0].next_val);
            __syncthreads();
            for (int m0 = 0; m0 < n_intervals; m0 += kDepth) {
#pragma unroll
                for (int u = 0; u < kDepth; ++u) {
                    const int m = m0 + u;
                    Stage<NLT> &s = st[(u + 1) % kDepth];
                    commit(s, m + 1);
                    issue(s, m + 1 + kDepth, s.next_val);
                    __syncthreads();
                }
            }
        } else {  // everything the chain needs is requested at once
            uint64_t v[kDepth];
#pragma unroll
            for (int t = 0; t < kDepth; ++t) v[t] = load_val(min(t, nblk - 1));
#pragma unroll
            for (int t = 0; t < kDepth; ++t)
                if (t < nblk) issue(st[t], t, v[t]);
            commit(st[0], 0);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kDepth; ++u) {
                if (u + 1 < kDepth && u + 1 < nblk) commit(st[(u + 1) % kDepth], u + 1);
                __syncthreads();
            }
        }
        return;
    }

    // ---------------------------------------------------------------------------------------------- solvers
    __builtin_amdgcn_s_setprio(3);  // the chain is the critical path of the iteration; whatever shares the CU is not
    const int w = tid >> 6, k = tid & 63;  // wavefront = quarter, lane = link
    constexpr int NP = (SW + 7) / 8;       // passes of 8 slots over this wavefront's quarter of the item row
    float4 *qrow = smem + kRing * S4;                              // [4 * SW + 8]: the item row, zero beyond it
    float4 *dpart = qrow + 4 * SW + 8;                             // [kB]: link k's four partial dot products
    float4 *epart = dpart + kB;                                    // [kB]: link k's four partial errors
    float *rbuf = reinterpret_cast<float *>(epart + kB) + w * kB;  // [4][kB]: rhs, one copy per wavefront
    float *wbuf = reinterpret_cast<float *>(epart + kB) + (4 + w) * kB;  // [4][kB]: w, one copy per wavefront
    float *tab = reinterpret_cast<float *>(epart + kB) + 8 * kB;   // [kSolTabFloats]
    float4 *zrow = reinterpret_cast<float4 *>(tab) + (kSolTabFloats + 3) / 4;  // [8] zeros
    unsigned *meet = reinterpret_cast<unsigned *>(zrow + 8);                    // [1] arrivals at the solvers' meeting points
    if (w == 0) {
        for (int i = k; i < kSolTabFloats; i += 64) tab[i] = it.tables[(i / kSolTabStride) * kBsTableStride + i % kSolTabStride];
        if (k < 8) zrow[k] = zero4();
        if (k == 0) *meet = 0u;
    }
    unsigned met = 0;
    const int y = cd.item;
    const int sl = k & 7, kg = k >> 3;  // (C): lane (slot sl of the pass, links 8 kg .. 8 kg + 7)
    f32x4 q4[NP];                       // this wavefront's quarter of the item row, slot w SW + 8 p + sl (every kg holds it)
    const f32x4 *qsrc = reinterpret_cast<const f32x4 *>(a.Q + static_cast<size_t>(y) * a.ldq);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int sq = 8 * p + sl, slot = w * SW + sq;
        const f32x4 v = qsrc[min(slot, nslots - 1)];
        q4[p] = sq < SW && slot < nslots ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        if (kg == 0 && sq < SW) *reinterpret_cast<f32x4 *>(qrow + slot) = q4[p];
    }
    float b = a.item_bias[y];
    const float lr = a.h.lr;
    const int kr = k & 31;
    const bool upper = k >= kH;
    __syncthreads();  // block 0 is in the ring
    for (int m = 0; m < n_intervals; ++m) {
        const bool live = m < nblk;  // workgroup uniform
        const int n = min(kB, len - kB * m);
        const float4 *tile = smem + (m % kRing) * S4;
        const float *Mt = reinterpret_cast<const float *>(tile + kB * RS);
        float base = 0.f, adel_k = 0.f, cdel_k = 0.f, apr = 0.f, cpr = 0.f, adel_n = 0.f, cdel_n = 0.f;
        f32x4 mq[4];
        if (live) {
            // this lane's 16 columns of its row of M: links 0-31 [M11 row | 0], links 32-63 [M21 row | M22 row]
            const float4 *mrow = w < 2 ? reinterpret_cast<const float4 *>(Mt + ((upper ? kH : 0) + kr) * kMS + 16 * w)
                                       : (upper ? reinterpret_cast<const float4 *>(Mt + (2 * kH + kr) * kMS + 16 * (w - 2)) : zrow);
#pragma unroll
            for (int t = 0; t < 4; ++t) mq[t] = lds4(mrow + t);
            base = Mt[k * kMS + kH];
            const int back = max(n - 1 - k, 0);
            adel_k = tab[kSolTabAdel + k], cdel_k = tab[kSolTabCdel + k];
            apr = tab[kSolTabApow + back], cpr = tab[kSolTabCpow + back];
            adel_n = tab[kSolTabAdel + n], cdel_n = tab[kSolTabCdel + n];
            // (A) this wavefront's quarter of every link's row against the item row; slots beyond the row multiply the
            // item row's zero padding
            const float4 *prow = tile + k * RS;
            f32x4 pv[SW], qv[SW];
#pragma unroll
            for (int i = 0; i < SW; ++i) {
                pv[i] = lds4(prow + min(w * SW + i, nslots - 1));
                qv[i] = lds4(qrow + w * SW + i);
            }
            f32x2 dacc[2] = {dup2(0.f), dup2(0.f)};
#pragma unroll
            for (int i = 0; i < SW; ++i) {
                dacc[0] = fma2(lo2(pv[i]), lo2(qv[i]), dacc[0]);
                dacc[1] = fma2(hi2(pv[i]), hi2(qv[i]), dacc[1]);
            }
            const f32x2 ds = dacc[0] + dacc[1];
            reinterpret_cast<float *>(dpart)[4 * k + w] = ds.x + ds.y;
        }
        met += 4;
        solvers_meet(meet, met, k);
        if (live) {
            // (B) e = M rhs: 16 columns each
            const f32x4 d4 = lds4(dpart + k);
            const float d = (d4.x + d4.y) + (d4.z + d4.w);
            const float rhs = k < n ? (base - (b - cdel_k * b)) - (d - adel_k * d) : 0.f;
            rbuf[k] = rhs;
            __builtin_amdgcn_wave_barrier();
            const float4 *rv = reinterpret_cast<const float4 *>(rbuf) + 4 * w;
            f32x2 eacc[2] = {dup2(0.f), dup2(0.f)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 r4 = lds4(rv + t);
                eacc[0] = fma2(lo2(mq[t]), lo2(r4), eacc[0]);
                eacc[1] = fma2(hi2(mq[t]), hi2(r4), eacc[1]);
            }
            const f32x2 es = eacc[0] + eacc[1];
            reinterpret_cast<float *>(epart)[4 * k + w] = es.x + es.y;
        }
        met += 4;
        solvers_meet(meet, met, k);
        if (live) {
            const f32x4 e4 = lds4(epart + k);
            const float e = (e4.x + e4.y) + (e4.z + e4.w);
            if (w == 0) {  // the block's errors, four to a lane, for phase 3
                const float e0 = k < n ? e : 0.f;
                const f32x4 e4v = {e0, dpp_move<0x55>(e0), dpp_move<0xAA>(e0), dpp_move<0xFF>(e0)};  // quad lanes 0..3
                if ((k & 3) == 0) {
                    float *dst = it.ebuf + static_cast<size_t>(g0 + m) * kB + k;
                    *reinterpret_cast<f32x4 *>(dst) = e4v;
                }
            }
            // (C) the state the block leaves behind; its start state goes to phase 3
            wbuf[k] = k < n ? lr * apr * e : 0.f;
            const float bs = row_sum16(k < n ? lr * cpr * e : 0.f);
            b = (b - cdel_n * b) + ((lane_value(bs, 0) + lane_value(bs, 16)) + (lane_value(bs, 32) + lane_value(bs, 48)));
            __builtin_amdgcn_wave_barrier();
            float *qdst = it.qstart + static_cast<size_t>(g0 + m) * a.ldq;
            const float4 *wv = reinterpret_cast<const float4 *>(wbuf) + 2 * kg;
#pragma unroll
            for (int p = 0; p < NP; ++p) {  // lane (slot, group): sum over the group's 8 links of w_k P[k][slot]
                const int sq = 8 * p + sl, slot = w * SW + sq;
                const bool ok = sq < SW && slot < nslots;
                if (ok && kg == 0) *reinterpret_cast<f32x4 *>(qdst + 4 * slot) = q4[p];
                const float4 *colp = tile + (8 * kg) * RS + min(slot, nslots - 1);
                f32x4 tb[8], wb[2];
#pragma unroll
                for (int i = 0; i < 8; ++i) tb[i] = lds4(colp + i * RS);
                wb[0] = lds4(wv), wb[1] = lds4(wv + 1);
                f32x2 ulo = dup2(0.f), uhi = dup2(0.f);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const f32x2 ww = dup2(wb[i >> 2][i & 3]);
                    ulo = fma2(ww, lo2(tb[i]), ulo);
                    uhi = fma2(ww, hi2(tb[i]), uhi);
                }
                float u[4] = {ulo.x, ulo.y, uhi.x, uhi.y};
#pragma unroll
                for (int c = 0; c < 4; ++c) {  // the eight groups: lanes l ^ 8, l ^ 16, l ^ 32
                    u[c] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(u[c]), 0x128, 0xf, 0xf, false));  // row_ror:8
                    u[c] = half_sum(row_pair_sum(u[c]));
                }
                const f32x4 qo = q4[p];
                q4[p] = ok ? f32x4{(qo.x - adel_n * qo.x) + u[0], (qo.y - adel_n * qo.y) + u[1], (qo.z - adel_n * qo.z) + u[2],
                                   (qo.w - adel_n * qo.w) + u[3]}
                           : f32x4{0.f, 0.f, 0.f, 0.f};
                if (kg == 0 && sq < SW) *reinterpret_cast<f32x4 *>(qrow + slot) = q4[p];
            }
        }
        __syncthreads();
    }
    {
        if (kg == 0) {
            f32x4 *qdst = reinterpret_cast<f32x4 *>(a.Q + static_cast<size_t>(y) * a.ldq);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int sq = 8 * p + sl, slot = w * SW + sq;
                if (sq < SW && slot < nslots) qdst[slot] = q4[p];
            }
        }
        if (tid == 0) a.item_bias[y] = b;
    }
}

}  // namespace bs_dev
}  // namespace cu2rec
