// ---- hot chains: a compute wave and two memory waves per block --------------------------------------------------
// The chain is latency bound: per update a ~17-deep dependent chain (slot dot, cross-row add, butterfly, error,
// item-row update).  Everything that is NOT on that chain -- fetching the next users' rows, updating and storing
// the user's row, the user bias -- is moved to a second wavefront of the same workgroup, which talks to the first
// one through LDS, double buffered per tile of 8 updates, with ONE __syncthreads() per tile as the only
// synchronisation (no flags, no spinning: every wave of the block executes the same number of barriers).
//   wave 0 ("A"):      the block's two chains, one per half-wave: reads the tile's user rows / ratings / biases from
//                      LDS, computes the error, publishes the item row as it was BEFORE the update and the error,
//                      updates the item row and bias in registers.
//   waves 1, 2 ("B"):  the same two chains, each wave half of every tile: load tile k+2's rows from global memory
//                      (entries three tiles ahead), apply tile k-1's user-row and user-bias updates from what A
//                      published and store them, publish tile k+1.
// W = lanes per chain: 32 (one slot per lane, 65 <= ld <= 128) or 16 (ld <= 64); wave 0 computes 64 / W chains,
// waves 1 and 2 move their memory
#pragma once

#include "sgd_device.hpp"

namespace cu2rec {
namespace {  // (ordered.hip's own: the one translation unit that includes this)

using namespace dev;

constexpr int kWide = 32;  // lanes per chain in the wide layout (one float4 slot per lane, 65 <= ld <= 128)

typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));

// Wide layout only: adds the two 16-lane rows of a half-wavefront, s_l + s_{l+16} of the canonical order.
__device__ __forceinline__ float cross_row_sum(float v) {
    // rows (r0, r1) -> both operands hold (r0 | r0) and (r1 | r1): the sum is r0 + r1 in every lane of both rows
    const uint2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

// Shape of the two-wave form for a row of S float4 slots per lane:
//   W      lanes per chain: 32 with S == 1 (65 <= ld <= 128: one slot per lane, s_l + s_{l+16} by v_permlane16_swap),
//          16 otherwise (the 16-lane layout of the other kernels, S slots per lane)
//   tile   updates between two barriers; part = the share of each of the two memory waves
//   chains chains per hot block, limited by the 64 KB of static LDS a block may declare
template <int W, int S>
struct DuoShape {
    static_assert(W == kGroup || S == 1, "the 32-lane layout holds exactly one slot per lane");
    static constexpr int kTile = S == 1 ? 8 : 4;
    static constexpr int kPart = kTile / 2;
    static constexpr int kChains = W == kWide ? 2 : (S <= 3 ? 4 : (S <= 6 ? 2 : 1));
};

template <int S>
struct WideRow {  // a lane's share of a factor row: slots lane, lane + W, ...
    float4 v[S];
};

template <int W, int S>
struct DuoLds {
    static constexpr int T = DuoShape<W, S>::kTile;
    float4 p[2][T][S][W];     // user rows of the tile, as loaded
    float4 qold[2][T][S][W];  // item row before each update of the tile (written by A)
    float rating[2][T], ub[2][T], err[2][T];
    int user[2][T];
};

template <int W, int S>
struct DuoTileRegs {  // one memory wave's share of a tile
    WideRow<S> rows[DuoShape<W, S>::kPart];
    uint64_t val;  // lanes 0..part-1: entry (user << 32 | rating bits)
    float ub;      // lanes 0..part-1: user bias
};

template <int W, int S>
__device__ __forceinline__ WideRow<S> load_wide_row(const float *__restrict__ base, size_t row, int ld, int nslots, int lane) {
    const float4 *p = reinterpret_cast<const float4 *>(base + row * static_cast<size_t>(ld));
    WideRow<S> r;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int slot = lane + W * s;
        const float4 v = p[min(slot, nslots - 1)];  // branch free: out-of-row lanes re-read the last slot and drop it
        const bool ok = slot < nslots;
        r.v[s] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
    }
    return r;
}

template <int W, int S>
__device__ __forceinline__ void store_wide_row(float *__restrict__ base, size_t row, int ld, int nslots, int lane,
                                               const WideRow<S> &r) {
    float4 *p = reinterpret_cast<float4 *>(base + row * static_cast<size_t>(ld));
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int slot = lane + W * s;
        if (slot < nslots) p[slot] = r.v[s];
    }
}

// this wave's entries of the tile starting at tile_start, one per lane 0..part-1 (mirrored on the other lanes)
template <int W, int S>
__device__ __forceinline__ uint64_t duo_load_vals(const uint64_t *__restrict__ vals, int tile_start, int end, int part,
                                                  int lane) {
    constexpr int kPart = DuoShape<W, S>::kPart;
    return vals[min(tile_start + kPart * part + (lane & (kPart - 1)), end - 1)];  // past the chain: its last entry, never used
}

template <int W, int S>
__device__ __forceinline__ void duo_load_rows(DuoTileRegs<W, S> &r, const SgdArgs &a, uint64_t val, int lane) {
    r.val = val;
    const int my_user = static_cast<int>(val >> 32);
    r.ub = a.user_bias[my_user];
#pragma unroll
    for (int t = 0; t < DuoShape<W, S>::kPart; ++t) {
        const int x = __shfl(my_user, t, W);
        r.rows[t] = load_wide_row<W, S>(a.P, static_cast<size_t>(x), a.ldp, a.nslots, lane);
    }
}

template <int W, int S>
__device__ __forceinline__ void duo_publish(DuoLds<W, S> &l, int buf, const DuoTileRegs<W, S> &r, int part, int lane) {
    constexpr int kPart = DuoShape<W, S>::kPart;
#pragma unroll
    for (int t = 0; t < kPart; ++t)
#pragma unroll
        for (int s = 0; s < S; ++s) l.p[buf][kPart * part + t][s][lane] = r.rows[t].v[s];
    if (lane < kPart) {
        const int e = kPart * part + lane;
        l.rating[buf][e] = __uint_as_float(static_cast<uint32_t>(r.val));
        l.ub[buf][e] = r.ub;
        l.user[buf][e] = static_cast<int>(r.val >> 32);
    }
}

// B: the user side of this wave's share of a finished tile (mf_sequential.cu:133-135,140 with the item row as it
// was at that update)
template <int W, int S>
__device__ __forceinline__ void duo_update_users(DuoLds<W, S> &l, int buf, int n_valid, const SgdArgs &a, int part, int lane) {
    constexpr int kPart = DuoShape<W, S>::kPart;
#pragma unroll
    for (int t = 0; t < kPart; ++t) {
        const int e = kPart * part + t;
        if (e < n_valid) {
            const float err = l.err[buf][e];
            WideRow<S> pn;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float4 po = l.p[buf][e][s][lane], qo = l.qold[buf][e][s][lane];
                pn.v[s].x = step(po.x, qo.x, err, a.h.lr, a.h.p_reg);
                pn.v[s].y = step(po.y, qo.y, err, a.h.lr, a.h.p_reg);
                pn.v[s].z = step(po.z, qo.z, err, a.h.lr, a.h.p_reg);
                pn.v[s].w = step(po.w, qo.w, err, a.h.lr, a.h.p_reg);
            }
            store_wide_row<W, S>(a.P, static_cast<size_t>(l.user[buf][e]), a.ldp, a.nslots, lane, pn);
        }
    }
    const int mine = kPart * part + lane;
    if (lane < kPart && mine < n_valid) {
        const float ub = l.ub[buf][mine], err = l.err[buf][mine];
        a.user_bias[l.user[buf][mine]] = ub + a.h.lr * (err - a.h.ub_reg * ub);
    }
}

// A: the dependent chain of one update (same operations, same order as predict<J> + rank1_update<J>'s item half); the
// user's row, rating and bias arrive in registers.
template <int W, int S>
__device__ __forceinline__ void duo_step_a(DuoLds<W, S> &l, int buf, int t, const WideRow<S> &po, float rating, float ub,
                                           const SgdArgs &a, WideRow<S> &q, float &ib, int lane) {
    float acc = slot_dot(q.v[0], po.v[0]);
#pragma unroll
    for (int s = 1; s < S; ++s) acc = acc + slot_dot(q.v[s], po.v[s]);
    const float dot = W == kWide ? row_sum16(cross_row_sum(acc)) : row_sum16(acc);  // canonical order either way
    const float err = rating - (((a.global_bias + ub) + ib) + dot);
#pragma unroll
    for (int s = 0; s < S; ++s) l.qold[buf][t][s][lane] = q.v[s];
    if (lane == 0) l.err[buf][t] = err;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const float4 qo = q.v[s];
        q.v[s].x = step(qo.x, po.v[s].x, err, a.h.lr, a.h.q_reg);
        q.v[s].y = step(qo.y, po.v[s].y, err, a.h.lr, a.h.q_reg);
        q.v[s].z = step(qo.z, po.v[s].z, err, a.h.lr, a.h.q_reg);
        q.v[s].w = step(qo.w, po.v[s].w, err, a.h.lr, a.h.q_reg);
    }
    ib = ib + a.h.lr * (err - a.h.ib_reg * ib);
}

template <int W, int S>
__device__ __forceinline__ void duo_compute(DuoLds<W, S> &l, int buf, int n_valid, const SgdArgs &a, WideRow<S> &q,
                                            float &ib, int lane) {
    constexpr int T = DuoShape<W, S>::kTile;
    if (n_valid == T) {
        // full tile: fetch everything its updates need from LDS up front (one latency per tile, not per update);
        // the scheduling barrier keeps the compiler from sinking the reads back next to their uses
        WideRow<S> po[T];
        float rating[T], ub[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int s = 0; s < S; ++s) po[t].v[s] = l.p[buf][t][s][lane];
            rating[t] = l.rating[buf][t];
            ub[t] = l.ub[buf][t];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < T; ++t) duo_step_a<W, S>(l, buf, t, po[t], rating[t], ub[t], a, q, ib, lane);
    } else {
        for (int t = 0; t < n_valid; ++t) {
            WideRow<S> po;
#pragma unroll
            for (int s = 0; s < S; ++s) po.v[s] = l.p[buf][t][s][lane];
            duo_step_a<W, S>(l, buf, t, po, l.rating[buf][t], l.ub[buf][t], a, q, ib, lane);
        }
    }
}

// One hot block: up to 64 / W chains; wave 0 computes (W lanes per chain), waves 1 and 2 each move half of every
// tile's memory traffic, wave 3 only keeps the barriers company.  ranges[r], r <= n_hot: where the chain of rank r begins in this
// iteration's sorted values (chain_ranges_kernel has looked them up behind the sort).
template <int W, int S>
__device__ __forceinline__ void run_hot_block_duo(const SgdArgs &a, const uint64_t *__restrict__ vals, int n_hot,
                                                  const int *__restrict__ item_of_rank, int rank_lo,
                                                  const int *__restrict__ ranges) {
    constexpr int kChains = DuoShape<W, S>::kChains, kTile = DuoShape<W, S>::kTile;
    __shared__ DuoLds<W, S> lds[kChains];
    __shared__ int s_range[kChains][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (W - 1);
    const bool role_a = wave == 0, role_b = wave == 1 || wave == 2;
    const int part = wave - 1;                       // memory waves: which half of the tile
    const int group = (threadIdx.x & 63) / W;        // lane group inside the wave
    const bool has_chain = group < kChains;          // blocks of fat rows use only some of the groups
    const int c = has_chain ? group : 0;
    const int r = rank_lo + blockIdx.x * kChains + c;  // ranks below rank_lo belong to somebody else (block-solve mode)
    if (role_a && has_chain) {
        int begin = 0, end = 0;
        if (r < n_hot) {
            begin = ranges[r];
            end = ranges[r + 1];
        }
        if (lane == 0) {
            s_range[c][0] = begin;
            s_range[c][1] = end;
        }
    }
    __syncthreads();
    const int begin = s_range[c][0], end = s_range[c][1], len = end - begin;
    int longest = 0;
#pragma unroll
    for (int i = 0; i < kChains; ++i) longest = max(longest, s_range[i][1] - s_range[i][0]);
    const int n_tiles = (longest + kTile - 1) / kTile;  // block uniform: every wave runs the same barriers
    if (n_tiles == 0) return;
    const bool alive = len > 0 && has_chain && (role_a || role_b);
    DuoLds<W, S> &l = lds[c];
    const int y = alive ? item_of_rank[r] : 0;
    WideRow<S> q;
#pragma unroll
    for (int s = 0; s < S; ++s) q.v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    float ib = 0.f;
    // A memory wave keeps two register tiles and alternates their roles each phase (no copies: a copy would wait for
    // the loads just issued): at the start of phase k, r0 / r1 (by parity of k) holds its share of tile k+1 -- loads
    // issued a whole phase ago -- and the other one receives tile k+2.
    DuoTileRegs<W, S> r0, r1;
    uint64_t v_next = 0;  // this wave's entries of tile k+2 at the start of phase k
    if (alive && role_b) {
        const uint64_t v0 = duo_load_vals<W, S>(vals, begin, end, part, lane);
        const uint64_t v1 = duo_load_vals<W, S>(vals, begin + kTile, end, part, lane);
        v_next = duo_load_vals<W, S>(vals, begin + 2 * kTile, end, part, lane);
        duo_load_rows<W, S>(r1, a, v0, lane);
        duo_load_rows<W, S>(r0, a, v1, lane);
        duo_publish<W, S>(l, 0, r1, part, lane);
    } else if (alive) {
        q = load_wide_row<W, S>(a.Q, static_cast<size_t>(y), a.ldq, a.nslots, lane);
        ib = a.item_bias[y];
    }
    __syncthreads();
    auto b_phase = [&](int k, DuoTileRegs<W, S> &ready, DuoTileRegs<W, S> &loading) {
        const uint64_t v_after = duo_load_vals<W, S>(vals, begin + (k + 3) * kTile, end, part, lane);
        duo_load_rows<W, S>(loading, a, v_next, lane);  // tile k + 2
        if (k >= 1) duo_update_users<W, S>(l, (k - 1) & 1, min(max(len - (k - 1) * kTile, 0), kTile), a, part, lane);
        duo_publish<W, S>(l, (k + 1) & 1, ready, part, lane);  // tile k + 1, after the reads of that buffer just above
        v_next = v_after;
    };
    auto a_phase = [&](int k) { duo_compute<W, S>(l, k & 1, min(max(len - k * kTile, 0), kTile), a, q, ib, lane); };
    for (int k = 0; k < n_tiles; k += 2) {
        if (alive) {
            if (role_b) b_phase(k, r0, r1); else a_phase(k);
        }
        __syncthreads();
        if (k + 1 < n_tiles) {  // block uniform
            if (alive) {
                if (role_b) b_phase(k + 1, r1, r0); else a_phase(k + 1);
            }
            __syncthreads();
        }
    }
    if (alive) {
        if (role_b) {
            duo_update_users<W, S>(l, (n_tiles - 1) & 1, min(max(len - (n_tiles - 1) * kTile, 0), kTile), a, part, lane);
        } else {
            store_wide_row<W, S>(a.Q, static_cast<size_t>(y), a.ldq, a.nslots, lane, q);
            if (lane == 0) a.item_bias[y] = ib;
        }
    }
}

}  // namespace
}  // namespace cu2rec
