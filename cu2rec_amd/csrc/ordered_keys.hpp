// ---- reading a sorted window's keys: where the popular items' chains begin ------------------------------------------
// What chain_ranges_kernel (ordered.hip) runs, behind the sort on the schedule stream.  (The sampling tile that WRITES the keys is the
// body of schedule_keys_tile_kernel in ordered.hip: as a function of its own in here it compiled to different code.)
#pragma once

#include "sgd_device.hpp"

namespace cu2rec {
namespace {  // (ordered.hip's own: the one translation unit that includes this)

using namespace dev;

// first position in keys[0, n) whose key is >= target
__device__ __forceinline__ int lower_bound_key(const uint32_t *__restrict__ keys, int n, uint32_t target) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Where the chains of the n_ranks most popular items begin in every iteration of a sorted batch: ranges[b][r] = first sorted
// position of iteration b whose popularity rank is >= r (r = 0 .. n_ranks).  Runs behind the sort on the schedule stream, so
// that a two-wave block finds its chains with two loads instead of two binary searches of ~17 dependent loads each at the
// head of every iteration (6-10 us of its ~50: the searches were the first thing the iteration's longest chains did).
__device__ __forceinline__ void find_chain_ranges(const uint32_t *__restrict__ keys, int n_active, int n_ranks,
                                                  int *__restrict__ ranges, size_t stride) {
    const int b = blockIdx.x;
    const uint32_t *kb = keys + static_cast<size_t>(b) * stride;
    for (int r = threadIdx.x; r <= n_ranks; r += kBlock)
        ranges[static_cast<size_t>(b) * (n_ranks + 1) + r] = lower_bound_key(kb, n_active, static_cast<uint32_t>(r));
}

}  // namespace
}  // namespace cu2rec
