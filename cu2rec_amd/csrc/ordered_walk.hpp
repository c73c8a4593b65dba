// ---- the walk: one 16-lane group per chain of an unpopular item ------------------------------------------------------
// What sgd_ordered_kernel's regular blocks (ordered.hip) run: chain_step, one update with the item row in registers, and
// walk_group, the chain that starts at one sorted position.
#pragma once

#include "sgd_device.hpp"

namespace cu2rec {
namespace {  // (ordered.hip's own: the one translation unit that includes this)

using namespace dev;

// ---- one update inside a chain: the user's row comes in, the item row / bias stay in registers -------------
template <int J>
__device__ __forceinline__ float chain_step(const SgdArgs &a, Row<J> &p, Row<J> &q, float ub, float &ib, float rating) {
    const float err = rating - predict<J>(p, q, ub, ib, a.global_bias);  // sgd.cu:45
    rank1_update<J>(p, q, err, a.h);                                      // mf_sequential.cu:129-137
    ib = ib + a.h.lr * (err - a.h.ib_reg * ib);                           // :141
    return ub + a.h.lr * (err - a.h.ub_reg * ub);                         // :140 (new user bias)
}

// A 16-lane group owns ONE sorted position and runs the chain that starts there (rank >= n_hot; longer chains have the
// two-wave form).  A chain is a string of dependent updates on the item row, but nothing else about it depends on values:
// three dependent round trips bring everything in -- (1) the 16 keys around the position and the 16 schedule entries
// behind it, (2) the item's id and the first four users' rows, (3) the item row -- and the users' rows stay four links
// ahead from there (a walk that asks for a row only when it needs it pays the memory latency per link).  Loads past the
// end of the chain re-read its last row (a cache hit) instead of being predicated.
template <int J>
__device__ __forceinline__ void walk_group(const SgdArgs &a, const uint32_t *__restrict__ keys, const uint64_t *__restrict__ vals,
                                           int n_active, const int *__restrict__ item_of_rank, int n_hot, int start) {
    constexpr int D = 4;  // user rows a walking group keeps in flight
    const int lane = threadIdx.x & (kGroup - 1);
    const int gshift = threadIdx.x & 48;  // this group's lanes in the wavefront
    if (start >= n_active) return;
    const int kpos = start - 1 + lane;  // lane 0: the position in front, lane 1: this one, lanes 2..15: the next 14
    const uint32_t key_l = keys[min(max(kpos, 0), n_active - 1)];
    const uint64_t val0 = vals[min(start + lane, n_active - 1)];
    const uint32_t key = __shfl(key_l, gshift + 1), prev = __shfl(key_l, gshift);
    if (static_cast<int>(key) < n_hot) return;               // a hot chain: the other role runs it
    if (start > 0 && prev == key) return;                    // the chain began at an earlier position
    const bool same0 = lane >= 2 && kpos < n_active && key_l == key;
    const uint32_t m0 = (static_cast<uint32_t>(__ballot(same0) >> gshift) & 0xffffu) >> 2;  // bit i: keys[start + 1 + i] == key
    int len = __ffs(static_cast<int>(~m0));  // 1 + leading run of equal keys: 1..15
    bool more = len == 15;
    auto link = [&](uint64_t mv, int i, int nw) -> uint64_t {
        const int src = gshift + min(i, nw - 1);
        const uint32_t lo = __shfl(static_cast<uint32_t>(mv), src), hi = __shfl(static_cast<uint32_t>(mv >> 32), src);
        return static_cast<uint64_t>(hi) << 32 | lo;
    };
    Row<J> cur[D], nxt[D];
    float cub[D], nub[D];
    auto prime = [&](uint64_t mv, int nw) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int x = static_cast<int>(link(mv, d, nw) >> 32);
            cur[d] = load_row<J>(a.P, static_cast<size_t>(x), a.ldp, a.nslots, lane);
            cub[d] = a.user_bias[x];
        }
    };
    prime(val0, len);
    const int y = item_of_rank[key];  // (a position below n_active: the key is the item's rank, no sentinel bit)
    while (more) {  // the chain's length: the group looks at 16 more keys at a time
        const int pos = start + len + lane;
        const bool same = pos < n_active && keys[pos] == key;
        const uint32_t m = static_cast<uint32_t>(__ballot(same) >> gshift) & 0xffffu;
        const int run = __ffs(static_cast<int>(~m)) - 1;  // 0..16
        len += run;
        more = run == kGroup;
    }
    Row<J> q = load_row<J>(a.Q, static_cast<size_t>(y), a.ldq, a.nslots, lane);
    float ib = a.item_bias[y];
    for (int wb = 0; wb < len; wb += kGroup) {
        const int nw = min(kGroup, len - wb);
        uint64_t myval = val0;
        if (wb > 0) {
            myval = vals[start + wb + min(lane, nw - 1)];
            prime(myval, nw);
        }
        for (int b0 = 0; b0 < nw; b0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int x = static_cast<int>(link(myval, b0 + D + d, nw) >> 32);
                nxt[d] = load_row<J>(a.P, static_cast<size_t>(x), a.ldp, a.nslots, lane);
                nub[d] = a.user_bias[x];
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (b0 + d < nw) {
                    const uint64_t val = link(myval, b0 + d, nw);
                    const int x = static_cast<int>(val >> 32);
                    const float new_ub = chain_step<J>(a, cur[d], q, cub[d], ib, __uint_as_float(static_cast<uint32_t>(val)));
                    store_row<J>(a.P, static_cast<size_t>(x), a.ldp, a.nslots, lane, cur[d]);
                    if (lane == 0) a.user_bias[x] = new_ub;
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                cur[d] = nxt[d];
                cub[d] = nub[d];
            }
        }
    }
    store_row<J>(a.Q, static_cast<size_t>(y), a.ldq, a.nslots, lane, q);
    if (lane == 0) a.item_bias[y] = ib;
}

}  // namespace
}  // namespace cu2rec
