// ---- phase 2, the longest chains: the look-ahead form ---------------------------------------------------------------------------
// The plain form (blocksolve_solve.hpp) is a ring of three dependent mat-vecs per block, (A) d = P q -> (B) e = M rhs -> (C) q <- a^n q + P^T w, split
// four ways with two meeting points: 1.4-1.6 us per block, and the hottest chain (31 blocks on the ML-20M shape) is more than half
// of an iteration.  With the cross block N_i = lr L[block i][block i - 1] from phase 1 (gram_cross_block) the errors obey
//     e_i = M_i (pre_i - N_i e_(i-1)),     pre_i[k] = base_i[k] - c^(k+64) b_(i-1) - a^(k+64) (p_(i,k) . q_(i-1))
// (tests/test_blocksolve_algebra.py, lookahead_chain): the only DEPENDENT work per block is two 64 x 64 mat-vecs, done by ONE
// wavefront with no partner to meet; the item row follows one block behind -- q_(i+1) from e_i, then (p . q_(i+1)) for block
// i + 2 -- on other wavefronts, with two blocks' time to do it in.  Eight wavefronts, fixed roles, NO workgroup barrier after the
// prologue; every hand-over is a counter in LDS that only its producer writes (LDS operations of a wavefront complete in order:
// whoever sees the count sees the data written before it):
//   wavefront 0   chain   e_i: record i (M_i, N_i, base) LDS -> registers, t0 = N_i e_(i-1), waits for g_i, e_i = M_i (pre_i - t0),
//                         publishes e_i and w_i = lr a^(n-1-k) e_i[k]; carries the item bias
//   wavefronts 1-2 state  q_(i+1) = a^n q_i + sum_k w_i[k] p_(i,k): every other pass of 8 slots each, lane = (slot, group of 8 links);
//                         q_i goes to phase 3 (qstart)
//   wavefront 3   dots    g_i[k] = p_(i,k) . q_(max(i-1, 0)): lane = link
//   wavefronts 4-7 loaders  block i (i = w mod 4): its 64 user rows memory -> registers -> P ring (three slots), then its record
//                         memory -> registers -> record ring (two slots).  One block at a time per wavefront, waiting with its data
//                         in registers for the slot: no load is in flight across a wait, so the compiler's s_waitcnt
//                         bookkeeping has nothing to get wrong; four wavefronts cover the latency.
// NSM: float4 slots per row the instantiation has registers for (nslots <= NSM <= 31: the rings fit the 160 KB of LDS).
#pragma once

#include "blocksolve_device.hpp"

namespace cu2rec {
namespace bs_dev {

constexpr int kLaPRing = 3, kLaRRing = 2, kLaDepth = 2;
constexpr int kLaNS4 = 17;                                  // float4 per row of the cross block in LDS (odd: conflict-free row reads)
constexpr int kLaRec4 = 3 * kH * kMS / 4 + kB * kLaNS4;     // a record in LDS: three factor tiles (base errors in column 32), the cross block
constexpr int kLaQ4 = 32;                                   // float4 per item-row buffer
constexpr int kLaMaxSlots = 29;
__host__ __device__ inline bool la_supported(int nslots) { return nslots >= 1 && nslots <= kLaMaxSlots; }
__host__ __device__ inline size_t la_lds_bytes(int nslots) {
    return (static_cast<size_t>(kLaPRing) * kB * (nslots | 1) + kLaRRing * kLaRec4 + 2 * kLaQ4 + 7 * kB / 4 + (kBsTableFloats + 3) / 4 + 4 + 64) * 16;
}

enum { kSyC0 = 0, kSyC1 = 1, kSyE = 2, kSyG = 3, kSyLdP = 4, kSyLdR = 8, kSyR = 12, kSyAbort = 13 };  // (C0 | C1, LdP[4], LdR[4]: read together)

// Waits until reached() says the counters are there; bounded: gives up after 2 s (or as soon as another wait of the workgroup has) and sets
// the workgroup's abort flag and the status word to 2 -- a wait inside one workgroup: the fork / join topology had no part in it
// (check_faults, device_runtime.cpp).  The store is unconditional (a load in front of it costs the loader's hot loop its wait-count schedule): a
// join that gave up earlier in the same call (1) is then reported as this wait.
template <class Reached>
__device__ __forceinline__ void la_wait_until(unsigned *sy, const BsIteration &it, Reached reached) {
    unsigned polls = 0;
    unsigned long long t0 = 0;
    while (!reached()) {
        __builtin_amdgcn_s_sleep(1);
        if ((++polls & 1023u) == 0) {
            if (t0 == 0) t0 = wall_clock64();
            if (__hip_atomic_load(sy + kSyAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u || wall_clock64() - t0 > it.wait_ticks) {
                __hip_atomic_store(sy + kSyAbort, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((threadIdx.x & 63) == 0) __hip_atomic_store(it.status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    asm volatile("" ::: "memory");  // nothing behind the wait is read in front of it
}
// ... until sy[word] >= target
__device__ __forceinline__ void la_wait(unsigned *sy, int word, unsigned target, const BsIteration &it) {
    la_wait_until(sy, it, [=] __device__ { return __hip_atomic_load(sy + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= target; });
}
// ... until all four counters sy[word .. word + 3] (16-byte aligned) have reached target: ONE LDS read per poll
__device__ __forceinline__ void la_wait4(unsigned *sy, int word, unsigned target, const BsIteration &it) {
    la_wait_until(sy, it, [=] __device__ {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        // (an LDS pointer by type: through a generic volatile pointer this was a FLAT load that waited for every global store in flight)
        const u32x4 v = __builtin_nontemporal_load((const __attribute__((address_space(3))) u32x4 *)(sy + word));
        asm volatile("" ::: "memory");
        return min(min(v.x, v.y), min(v.z, v.w)) >= target;
    });
}
// ... until both sy[word] and sy[word + 1] (8-byte aligned) have
__device__ __forceinline__ void la_wait2(unsigned *sy, int word, unsigned target, const BsIteration &it) {
    la_wait_until(sy, it, [=] __device__ {
        const u32x2 v = __builtin_nontemporal_load((const __attribute__((address_space(3))) u32x2 *)(sy + word));
        asm volatile("" ::: "memory");
        return min(v.x, v.y) >= target;
    });
}
__device__ __forceinline__ void la_post(unsigned *sy, int word, unsigned value) {
    asm volatile("" ::: "memory");  // everything written so far is issued in front of the count
    if ((threadIdx.x & 63) == 0) __hip_atomic_store(sy + word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int NSM>
__device__ __forceinline__ void chain_lookahead(const SgdArgs &a, const BsIteration &it, float4 *smem, const BsChainDesc &cd) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nslots = a.nslots, RS = nslots | 1;
    const int begin = cd.begin, len = cd.len, nblk = (len + kB - 1) / kB, g0 = cd.blk0, y = cd.item;
    float4 *pring = smem;                                        // [kLaPRing][kB][RS]
    float4 *rring = pring + kLaPRing * kB * RS;                  // [kLaRRing][kLaRec4]
    float4 *qbuf = rring + kLaRRing * kLaRec4;                   // [2][kLaQ4] the item row in front of block i: buffer i & 1, zero beyond the row
    float *wbuf = reinterpret_cast<float *>(qbuf + 2 * kLaQ4);   // [2][kB] w_i
    float *ebl = wbuf + 2 * kB;                                  // [2][kB] e_i
    float *tbuf = ebl + 2 * kB;                                  // [kB]    the chain wavefront's own right-hand side
    float *gbuf = tbuf + kB;                                     // [2][kB] g_i
    float *tab = gbuf + 2 * kB;                                  // [kBsTableFloats]
    unsigned *sy = reinterpret_cast<unsigned *>(tab + ((kBsTableFloats + 3) & ~3));  // [16] the counters
    f32x4 *sink = reinterpret_cast<f32x4 *>(sy + 16);                               // [64] where the loaders' surplus lanes store
    const float lr = a.h.lr;

    if (wave >= 4) {
        // ---------------------------------------------------------------------------------------------------------- loaders
        // wavefront 4 + w: quarter w of every block's row image (float4 numbers 64 (w NQ + j) + lane, j < NQ) and its share of the
        // block's record (w 0, 1: the factor tiles, w 0 the base errors too; w 2, 3: the cross block), kLaDepth blocks in flight in
        // registers.  Every load and store is unconditional (clamped addresses, a sink in LDS for the surplus lanes): a branch
        // around a load makes the compiler wait for everything in flight.
        const int w = wave - 4;
        __builtin_amdgcn_s_setprio(2);
        constexpr int NQ = (NSM + 3) / 4;
        const int idx0 = w * kB * NQ + lane;
        const int row0 = idx0 / nslots, slot0 = idx0 - row0 * nslots;
        const int drow = kB / nslots, dslot = kB - drow * nslots;
        auto load_val = [&](int i) -> uint64_t { return it.vals[begin + min(kB * i + lane, len - 1)]; };
        struct LaStage {
            f32x4 v[NQ], r[8];
            uint64_t next_val;
        };
        auto issue = [&](LaStage &st, int i, uint64_t val) {  // block i (clamped: past the chain's end the last block again, never committed)
            const int ic = min(i, nblk - 1);
            st.next_val = load_val(min(i + kLaDepth, nblk - 1));
            const int x = static_cast<int>(val >> 32);
            int row = row0, slot = slot0;
#pragma unroll
            for (int j = 0; j < NQ; ++j) {  // past the block's image (float4 number >= 64 nslots): the last row again
                const int xr = __shfl(x, min(row, kB - 1));
                st.v[j] = reinterpret_cast<const f32x4 *>(a.P + static_cast<size_t>(xr) * a.ldp)[slot];
                slot += dslot, row += drow;
                if (slot >= nslots) slot -= nslots, ++row;
            }
            // the record: 768 float4 of factor tiles + 16 of base errors (Mbuf), 1,024 of the cross block (Nbuf; block 0 has none:
            // block 1's, never used)
            const f32x4 *src = w < 2 ? reinterpret_cast<const f32x4 *>(it.Mbuf + static_cast<size_t>(g0 + ic) * kBsRecFloats) + 384 * w
                                     : reinterpret_cast<const f32x4 *>(it.Nbuf + static_cast<size_t>(g0 + max(ic, 1)) * kBsCrossFloats) + 512 * (w - 2);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int at = w < 2 && j >= 6 ? 768 - 384 * w + (lane & 15) : lane + 64 * j;  // (w < 2: six tiles' pieces, then the base errors)
                st.r[j] = src[at];
            }
        };
        auto commit = [&](const LaStage &st, int i) {
            if (i >= kLaPRing) {  // the slot's last reader: the state wavefronts, block i - 3
                la_wait2(sy, kSyC0, static_cast<unsigned>(i - kLaPRing + 1), it);
            }
            {
                f32x4 *tile = reinterpret_cast<f32x4 *>(pring + (i % kLaPRing) * kB * RS);
                int row = row0, slot = slot0;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < NQ; ++j) {  // past the image: this lane's float4 of the sink
                    f32x4 *dst = row < kB ? tile + row * RS + slot : sink + lane;
                    *dst = kB * i + row < len ? st.v[j] : z;
                    slot += dslot, row += drow;
                    if (slot >= nslots) slot -= nslots, ++row;
                }
            }
            la_post(sy, kSyLdP + w, static_cast<unsigned>(i + 1));
            if (i >= kLaRRing) la_wait(sy, kSyR, static_cast<unsigned>(i - kLaRRing + 1), it);  // the chain wavefront has taken record i - 2
            f32x4 *rr = reinterpret_cast<f32x4 *>(rring + (i % kLaRRing) * kLaRec4);
            if (w < 2) {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int idx = 384 * w + lane + 64 * j;  // tile idx >> 8, row (idx >> 3) & 31, float4 idx & 7
                    rr[((idx >> 8) * kH + ((idx >> 3) & 31)) * (kMS / 4) + (idx & 7)] = st.r[j];
                }
                if (w == 0 && lane < 16) {  // float4 number 768 + lane: the base errors of links 4 lane .. 4 lane + 3, column 32 of their rows
                    float *col = reinterpret_cast<float *>(rr) + (4 * lane) * kMS + kH;
#pragma unroll
                    for (int e = 0; e < 4; ++e) col[e * kMS] = st.r[6][e];
                }
            } else {
                f32x4 *nl = rr + 3 * kH * kMS / 4;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int idx = 512 * (w - 2) + lane + 64 * j;
                    nl[(idx >> 4) * kLaNS4 + (idx & 15)] = st.r[j];
                }
            }
            la_post(sy, kSyLdR + w, static_cast<unsigned>(i + 1));
        };
        static_assert(kLaDepth == 2, "two stages: four wavefronts x two blocks x 15 KB in flight");
        LaStage st[kLaDepth];
        {
            uint64_t v0[kLaDepth];
#pragma unroll
            for (int t = 0; t < kLaDepth; ++t) v0[t] = load_val(min(t, nblk - 1));
#pragma unroll
            for (int t = 0; t < kLaDepth; ++t) issue(st[t], t, v0[t]);
        }
        __syncthreads();  // the prologue's one barrier: counters and tables are set
        for (int m0 = 0; m0 < nblk; m0 += kLaDepth) {
#pragma unroll
            for (int u = 0; u < kLaDepth; ++u) {
                const int i = m0 + u;
                if (i < nblk) commit(st[u], i);  // wavefront uniform
                issue(st[u], i + kLaDepth, st[u].next_val);
            }
        }
        return;
    }

    if (wave == 3) {
        // ------------------------------------------------------------------------------------------------------------- dots
        __syncthreads();
        __builtin_amdgcn_s_setprio(2);
        for (int i = 0; i < nblk; ++i) {
            const int src = max(i - 1, 0);
            la_wait4(sy, kSyLdP, static_cast<unsigned>(i + 1), it);
            if (src > 0) la_wait2(sy, kSyC0, static_cast<unsigned>(src), it);
            const float4 *prow = pring + (i % kLaPRing) * kB * RS + lane * RS;
            const float4 *qv = qbuf + (src & 1) * kLaQ4;
            // two halves, every read of a half in flight before its first product: one LDS latency per half, not one per slot
            constexpr int NH2 = (NSM + 1) / 2;
            f32x2 acc[4] = {dup2(0.f), dup2(0.f), dup2(0.f), dup2(0.f)};
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                f32x4 pv[NH2], qq[NH2];
#pragma unroll
                for (int j = 0; j < NH2; ++j) {
                    pv[j] = lds4(prow + min(hh * NH2 + j, nslots - 1));
                    qq[j] = lds4(qv + min(hh * NH2 + j, kLaQ4 - 1));  // (the item row's buffer is zero beyond the row)
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NH2; ++j) {
                    if (hh * NH2 + j < NSM) {
                        acc[2 * (j & 1)] = fma2(lo2(pv[j]), lo2(qq[j]), acc[2 * (j & 1)]);
                        acc[2 * (j & 1) + 1] = fma2(hi2(pv[j]), hi2(qq[j]), acc[2 * (j & 1) + 1]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            acc[0] += acc[2];
            acc[1] += acc[3];
            const f32x2 ds = acc[0] + acc[1];
            gbuf[(i & 1) * kB + lane] = ds.x + ds.y;
            la_post(sy, kSyG, static_cast<unsigned>(i + 1));
        }
        return;
    }

    if (wave >= 1) {
        // ------------------------------------------------------------------------------------------------------------ state
        const int c = wave - 1;
        constexpr int NP = (NSM + 7) / 8, NPW = (NP + 1) / 2;  // passes of 8 slots; this wavefront: passes c, c + 2, ...
        const int sl = lane & 7, kg = lane >> 3;
        f32x4 q4[NPW];
        const f32x4 *qsrc = reinterpret_cast<const f32x4 *>(a.Q + static_cast<size_t>(y) * a.ldq);
#pragma unroll
        for (int pp = 0; pp < NPW; ++pp) {
            const int slot = 8 * (2 * pp + c) + sl;
            const f32x4 v = qsrc[min(slot, nslots - 1)];
            q4[pp] = slot < nslots ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            if (kg < 2 && slot < kLaQ4) *reinterpret_cast<f32x4 *>(qbuf + kg * kLaQ4 + slot) = kg == 0 ? q4[pp] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        __builtin_amdgcn_s_setprio(2);
        for (int i = 0; i < nblk; ++i) {
            const int n = min(kB, len - kB * i);
            const float adel_n = tab[kTabAdel + n];
            la_wait(sy, kSyE, static_cast<unsigned>(i + 1), it);
            const float4 *tile = pring + (i % kLaPRing) * kB * RS;
            const float4 *wv = reinterpret_cast<const float4 *>(wbuf + (i & 1) * kB) + 2 * kg;
            float *qdst = it.qstart + static_cast<size_t>(g0 + i) * a.ldq;
            const f32x4 wb0 = lds4(wv), wb1 = lds4(wv + 1);
            f32x4 tb[NPW][8];  // every read of the block in flight before the first product
#pragma unroll
            for (int pp = 0; pp < NPW; ++pp) {
                const float4 *colp = tile + (8 * kg) * RS + min(8 * (2 * pp + c) + sl, nslots - 1);
#pragma unroll
                for (int r = 0; r < 8; ++r) tb[pp][r] = lds4(colp + r * RS);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pp = 0; pp < NPW; ++pp) {
                const int slot = 8 * (2 * pp + c) + sl;
                const bool ok = slot < nslots;
                // the row in front of block i: phase 3's
                if (ok && kg == 0) *reinterpret_cast<f32x4 *>(qdst + 4 * slot) = q4[pp];
                f32x2 ulo = dup2(0.f), uhi = dup2(0.f);
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const f32x2 ww = dup2(r < 4 ? wb0[r & 3] : wb1[r & 3]);
                    ulo = fma2(ww, lo2(tb[pp][r]), ulo);
                    uhi = fma2(ww, hi2(tb[pp][r]), uhi);
                }
                float u[4] = {ulo.x, ulo.y, uhi.x, uhi.y};
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // the eight groups: lanes l ^ 8, l ^ 16, l ^ 32
                    u[e] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(u[e]), 0x128, 0xf, 0xf, false));  // row_ror:8
                    u[e] = half_sum(row_pair_sum(u[e]));
                }
                const f32x4 qo = q4[pp];
                q4[pp] = ok ? f32x4{(qo.x - adel_n * qo.x) + u[0], (qo.y - adel_n * qo.y) + u[1], (qo.z - adel_n * qo.z) + u[2],
                                    (qo.w - adel_n * qo.w) + u[3]}
                            : f32x4{0.f, 0.f, 0.f, 0.f};
                if (ok && kg == 0) *reinterpret_cast<f32x4 *>(qbuf + ((i + 1) & 1) * kLaQ4 + slot) = q4[pp];
            }
            la_post(sy, kSyC0 + c, static_cast<unsigned>(i + 1));
        }
        if (kg == 0) {
            f32x4 *qd = reinterpret_cast<f32x4 *>(a.Q + static_cast<size_t>(y) * a.ldq);
#pragma unroll
            for (int pp = 0; pp < NPW; ++pp) {
                const int slot = 8 * (2 * pp + c) + sl;
                if (slot < nslots) qd[slot] = q4[pp];
            }
        }
        return;
    }

    // ------------------------------------------------------------------------------------------------------------------ chain
    const int k = lane;
    for (int i = k; i < kBsTableFloats; i += 64) tab[i] = it.tables[i];
    if (k < 16) sy[k] = 0u;
    float b_cur = a.item_bias[y], b_prev = b_cur;
    asm volatile("" ::"v"(b_cur));
    __syncthreads();
    __builtin_amdgcn_s_setprio(3);
    const int kr = k & 31;
    const bool upper = k >= kH;
    // record i in registers one block ahead: this lane's row of M (links 0-31: [M11 row | 0], links 32-63: [M21 row | M22 row]), its
    // row of the cross block, its base error -- read while the other wavefronts work on the item row, not on the dependent path
    f32x4 m4[16], n4[16];
    float base;
    auto take_record = [&](int i) {
        la_wait4(sy, kSyLdR, static_cast<unsigned>(i + 1), it);
        const float4 *rr = rring + (i % kLaRRing) * kLaRec4;
        const float *Mt = reinterpret_cast<const float *>(rr);
        const float4 *mlo = reinterpret_cast<const float4 *>(Mt + ((upper ? kH : 0) + kr) * kMS);
        const float4 *mhi = reinterpret_cast<const float4 *>(Mt + (2 * kH + kr) * kMS);
        const float4 *nrow = rr + 3 * kH * kMS / 4 + k * kLaNS4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            m4[j] = lds4(mlo + j);
            const f32x4 hi = lds4(mhi + j);
            m4[8 + j] = upper ? hi : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) n4[j] = lds4(nrow + j);
        base = Mt[k * kMS + kH];
        la_post(sy, kSyR, static_cast<unsigned>(i + 1));  // (the slot's reads are issued: LDS serves a wavefront in order)
    };
    take_record(0);
    for (int i = 0; i < nblk; ++i) {
        const int n = min(kB, len - kB * i);
        // t0 = N_i e_(i-1): this lane's row of the cross block against the errors of the block before (all 16 broadcast reads in
        // flight before the first product)
        f32x2 tacc[2] = {dup2(0.f), dup2(0.f)};
        if (i > 0) {
            const float4 *ev = reinterpret_cast<const float4 *>(ebl + ((i - 1) & 1) * kB);
            f32x4 e4[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) e4[j] = lds4(ev + j);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                tacc[0] = fma2(lo2(n4[j]), lo2(e4[j]), tacc[0]);
                tacc[1] = fma2(hi2(n4[j]), hi2(e4[j]), tacc[1]);
            }
        }
        const f32x2 ts = tacc[0] + tacc[1];
        const float t0 = ts.x + ts.y;
        // pre_i from the state in front of block max(i - 1, 0)
        const int kd = i > 0 ? k + kB : k;
        const float adel_k = tab[kTabAdel + kd], cdel_k = tab[kTabCdel + kd];
        const float bsrc = i > 0 ? b_prev : b_cur;
        la_wait(sy, kSyG, static_cast<unsigned>(i + 1), it);
        const float gd = gbuf[(i & 1) * kB + k];
        const float pre = k < n ? (base - (bsrc - cdel_k * bsrc)) - (gd - adel_k * gd) : 0.f;
        tbuf[k] = pre - t0;
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        f32x2 eacc[2] = {dup2(0.f), dup2(0.f)};
        {
            const float4 *tv = reinterpret_cast<const float4 *>(tbuf);
            f32x4 t4[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) t4[j] = lds4(tv + j);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                eacc[0] = fma2(lo2(m4[j]), lo2(t4[j]), eacc[0]);
                eacc[1] = fma2(hi2(m4[j]), hi2(t4[j]), eacc[1]);
            }
        }
        const f32x2 es = eacc[0] + eacc[1];
        const float e = k < n ? es.x + es.y : 0.f;
        const int back = max(n - 1 - k, 0);
        ebl[(i & 1) * kB + k] = e;
        wbuf[(i & 1) * kB + k] = k < n ? lr * tab[kTabApow + back] * e : 0.f;
        la_post(sy, kSyE, static_cast<unsigned>(i + 1));
        it.ebuf[static_cast<size_t>(g0 + i) * kB + k] = e;
        if (i + 1 < nblk) take_record(i + 1);  // wavefront uniform
        // the item bias behind block i
        const float bs = row_sum16(k < n ? lr * tab[kTabCpow + back] * e : 0.f);
        const float cdel_n = tab[kTabCdel + n];
        const float b_next = (b_cur - cdel_n * b_cur) + ((lane_value(bs, 0) + lane_value(bs, 16)) + (lane_value(bs, 32) + lane_value(bs, 48)));
        b_prev = b_cur;
        b_cur = b_next;
    }
    if (k == 0) a.item_bias[y] = b_cur;
}

}  // namespace bs_dev
}  // namespace cu2rec
