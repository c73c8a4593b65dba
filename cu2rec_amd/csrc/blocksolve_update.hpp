// ---- phase 3: the user side of every hot block ---------------------------------------------------------------------
// One wavefront per (block, 64 columns), lane = column.  The wavefront holds its 64 x 64 piece of the block's user rows in registers
// (one 256-byte row segment per load instruction, user id and error of link k broadcast from lane k) and walks down the links with
// the reference's own recurrence (mf_sequential.cu:133-134), the item row as link k saw it carried in one register:
//     p_k <- p_k + lr (e_k q - P_reg p_k),   q <- q + lr (e_k p_k - Q_reg q)        (p_k on the right: the old value)
// 64 dependent steps of a few VALU instructions (~0.4 us), no LDS, no staging.  (Rounds 2-3 built the rows "as link k saw them"
// as a triangular 64 x 64 product on the MFMA pipe: 48 fp32 MFMA instructions and ~200 LDS reads per 32 columns, 3 us of a wavefront's
// 9 -- and the kernel's duration IS one wavefront's latency, every block's workgroup being resident at once.)
#pragma once

#include "blocksolve_device.hpp"

namespace cu2rec {
namespace bs_dev {

constexpr int kUpdMaxWaves = (4 * kBsMaxSlots + 63) / 64;

__device__ __forceinline__ void update_block(const SgdArgs &a, const BsIteration &it, int g) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const BsBlockDesc bd = it.blocks[g];
    if (bd.n_valid == 0) return;  // workgroup uniform
    const bool mine = lane < bd.n_valid;  // lane l: link l
    // links past the end of a short block: the last link's row (finite, loaded, never stored) with e = 0
    const uint64_t val = it.vals[bd.pos0 + min(lane, bd.n_valid - 1)];
    const int x = static_cast<int>(val >> 32);
    const float lr = a.h.lr;
    const int ncols = 4 * a.nslots;
    const int col = 64 * wave + lane, colc = min(col, ncols - 1);
    const float qs = it.qstart[static_cast<size_t>(g) * a.ldq + colc];
    const float e_all = it.ebuf[static_cast<size_t>(g) * kB + lane];
    const float e = mine ? e_all : 0.f;
    float p[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) {
        const int xk = __builtin_amdgcn_readlane(x, k);
        p[k] = a.P[static_cast<size_t>(xk) * a.ldp + colc];
    }
    float q = qs;
    const float p_reg = a.h.p_reg, q_reg = a.h.q_reg;
#pragma unroll
    for (int k = 0; k < kB; ++k) {
        const float ek = lane_value(e, k);
        const float pk = p[k];
        p[k] = pk + lr * (ek * q - p_reg * pk);  // mf_sequential.cu:133-134
        q = q + lr * (ek * pk - q_reg * q);
    }
    // (the stores in a sequence of their own behind the walk: interleaved with it -- what the compiler makes of the two unrolled loops --
    // every step's wait for its row also waited for stores issued before it, 5 us per wavefront)
#pragma unroll
    for (int k = 0; k < kB; ++k) asm volatile("" : "+v"(p[k]));  // (the values exist HERE: no sinking of the walk into the stores)
    __builtin_amdgcn_sched_barrier(0);
    if (col < ncols) {
#pragma unroll
        for (int k = 0; k < kB; ++k) {
            if (k < bd.n_valid) a.P[static_cast<size_t>(__builtin_amdgcn_readlane(x, k)) * a.ldp + col] = p[k];  // wavefront uniform
        }
    }
    if (wave == 0 && mine) {
        const float ub = a.user_bias[x];
        a.user_bias[x] = ub + lr * (e - a.h.ub_reg * ub);  // mf_sequential.cu:140
    }
}

// The join with the side stream: one thread of an extra workgroup in the LAST launch of the iteration on the main stream (phase 3).
// It ends when the signal kernel queued behind this iteration's side kernel has run -- i.e. that kernel is complete, its rows in
// memory -- so that the next iteration's phase 1, queued behind this launch, needs no event (a wait on one costs the stream 2.5 us
// per iteration).  (The side kernel's workgroups counting THEMSELVES through, each behind an agent-scope release of its rows, was
// tried in round 4: 9350 L2 write-backs per launch, the side kernel took 292 us instead of 46.)
// This wait guards DATA -- the next phase 1 reads rows the side kernel and phase 3 write -- so it gives up only when the GPU must be
// taken for wedged: 15 x the bound of the other waits, 30 s by default; then the status word is set to 1 and the call reports it.  A word
// that another wait has set already (a ring wait's 2) ends the wait too, and is left as it is: the first cause is the one reported.
__device__ __forceinline__ void await_iteration_end(const BsIteration &it) {
    const unsigned long long t0 = wall_clock64();
    unsigned polls = 0;
    while (it.side_seq && ld_agent(it.side_seq) < it.side_target) {
        __builtin_amdgcn_s_sleep(8);
        if ((++polls & 63u) == 0) {
            if (ld_agent(it.status) != 0u) break;
            if (wall_clock64() - t0 > 15ull * it.wait_ticks) {
                __hip_atomic_store(it.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
}

}  // namespace bs_dev
}  // namespace cu2rec
