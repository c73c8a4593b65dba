// Ordered SGD: the sequential semantics of mf_sequential.cu:102-143 at GPU speed, deterministic and
// bit-identical to the CPU oracle (TREE16 dot order), with no races.
//
// Why it is possible: the sampler is counter based, so WHICH rating user x trains on at iteration i is a
// pure function of (seed, x, i) -- known before any value is computed.  Inside one iteration every user
// appears exactly once, so two updates conflict only through a shared ITEM row, and the sequential order
// matters only among the users that sampled the same item.  Hence, per iteration:
//     for every item in parallel:  apply the updates of the users that sampled it, in ascending user order
// is exactly the sequential result.  An iteration becomes a set of independent "item chains".
//
// Pipeline for a window of B iterations (B <= OrderedSchedule::max_batch), steps 1-3 on the schedule stream beside the
// iterations of the window before:
//   1. schedule_keys_tile_kernel  for every (iteration b, user x): draw the rating, emit
//        key = popularity_rank(item)                          (users without ratings: the one bit above all ranks)
//        val = user << 32 | rating bits
//      at [b * n_rows + x] (64 users x 64 iterations per workgroup, a user's rating row read once for all its samples)
//   2. a stable radix sort of the (key, val) pairs by key, every iteration a segment of n_rows pairs of its own (rocPRIM's
//      segmented_radix_sort_pairs; stability keeps users ascending inside a chain).  Afterwards iteration b occupies
//      [b * n_rows, b * n_rows + n_active), the users without ratings behind it; chains are runs of equal keys, and because
//      the key IS the item's popularity rank, the longest chains come first.
//   3. chain_ranges_kernel  for every iteration, the first sorted position of every rank r <= n_range_ranks: where the
//      chains of the popular items begin and end.  The two-wave blocks, the sweeper and the block-solve mode's plan
//      (bs_plan_kernel, blocksolve.hip, queued behind it) all read this one table.
//   4. sgd_ordered_kernel, one launch per iteration (the kernel boundary carries the P-row dependency from
//      iteration b to b+1).  The item row and item bias stay in registers for a whole chain (read and written once
//      per chain, not once per update).  Two block roles:
//        hot blocks      the chains of the 256 most popular items.  Their length (thousands of dependent updates) IS
//                        the iteration's critical path, so a block splits each chain over wavefronts: a compute wave
//                        runs only the dependent arithmetic, two memory waves prefetch the users' rows, publish them
//                        through LDS and apply / store the user-side updates (run_hot_block_duo).
//        regular blocks  a 16-lane group owns one sorted position of the iteration's tail and runs the chain that STARTS
//                        there, the users' rows fetched four links ahead (walk_group).
// The arithmetic of one update is the same device code as the Hogwild kernel (sgd_device.hpp).
//
// This file: the __global__ entry points (the sampling tile whole: schedule_keys_tile_kernel), launch_chain / launch_chains, the
// sort's configuration and class OrderedSchedule.  What the other kernels run is in three headers that do not include each other,
// over sgd_device.hpp:
//   ordered_keys.hpp  chain_ranges_kernel: lower_bound_key, find_chain_ranges
//   ordered_duo.hpp   sgd_ordered_kernel's hot blocks: DuoShape, the duo_* steps of the two roles, run_hot_block_duo
//   ordered_walk.hpp  sgd_ordered_kernel's regular blocks: chain_step, walk_group
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstring>  // (rocPRIM's headers call memset without including it)
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "hip_check.hpp"
#include "item_rates.hpp"
#include "kernels.hpp"
#include "ordered.hpp"
#include "ordered_duo.hpp"
#include "ordered_keys.hpp"
#include "ordered_walk.hpp"
#include "sampler.hpp"

namespace cu2rec {

namespace {

using namespace dev;

// The segmented sort of a batch's schedule (one segment per iteration, run()) is rocPRIM's with a block of 1,024 threads instead of
// its 256: ONE workgroup sorts a segment of n_rows pairs, and with the default block the kernel sat on its 64 CUs for 6.6 ms of
// every 15 on the Netflix shape (480,189 pairs a segment) -- a quarter of the chip that the throughput-bound phases of that shape
// then lack (iterations beside it 306 instead of 238 us).  Four times the threads: a quarter of the time.
constexpr unsigned kSegBlock = 1024;
constexpr unsigned kSegItems = 8;
using SegSortConfig = rocprim::segmented_radix_sort_config<8, rocprim::kernel_config<kSegBlock, kSegItems>,
                                                           rocprim::WarpSortConfig<8, 4, 256, 64, 16, 8, 256>, true>;

constexpr int kHotChains = 256;  // most popular items: their chains run in the two-wave form (run_hot_block_duo)

// Keys and values of a window, 64 users x up to 64 iterations per workgroup, with the users' RATING ROWS read once instead of one
// random access per sample (two cache lines -- indices, data -- for every (user, iteration): 2.0 GB per batch of 64 iterations on
// the ML-20M shape, which the iterations running beside it paid for: tools/schedule_interference.py).  Here a wavefront
// takes 16 users one after the other: lane b draws iteration b's sample, the row comes in with coalesced loads (256 ratings
// per round: most users' whole row), the lanes pick their ratings out of the registers (ds_bpermute); rows of more than
// kRowRounds rounds fall back to two gathers per sample.  The tile leaves through LDS, so that every store is a run of 64
// consecutive users of one iteration.
constexpr int kRowRounds = 8;       // x 256 ratings: rows up to 2,048 ratings are read whole
constexpr int kTileStride = 65;     // LDS words per iteration of the tile (64 users + 1: lanes write columns)

__global__ __launch_bounds__(256) void schedule_keys_tile_kernel(const int *__restrict__ indptr, const int *__restrict__ indices,
                                                                 const float *__restrict__ data, const int *__restrict__ item_rank,
                                                                 int n_rows, int n_batch, uint32_t sentinel, uint64_t seed,
                                                                 uint64_t iter0, int user_offset, uint32_t *__restrict__ keys,
                                                                 uint64_t *__restrict__ vals) {
    __shared__ uint32_t t_key[64 * kTileStride];
    __shared__ uint32_t t_rat[64 * kTileStride];  // the rating's bits; the user (the value's upper half) is known at the store
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x0 = static_cast<int>(blockIdx.x) * 64;
    const int b = lane;  // this lane's iteration
    // the 16 users' row bounds: lane l < 17 holds indptr[x0 + 16 wave + l]
    const int xi = min(x0 + 16 * wave + min(lane, 16), n_rows);
    const int bound = indptr[xi];
    // four users at a time: their first 256 ratings (most rows whole) are requested together, the samples drawn while the loads
    // fly, and their four item ranks looked up together -- a wavefront walking its 16 users one load round trip after the other
    // kept the kernel (a chip-filling grid beside the iterations) on the CUs 1.6 times as long
    for (int u0 = 0; u0 < 16; u0 += 4) {
        int low[4], high[4], y_i[4], y[4], vi[4][4];
        uint32_t r[4], vr[4][4];
        bool live[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + 16 * wave + u0 + j;
            low[j] = __shfl(bound, u0 + j);
            high[j] = __shfl(bound, u0 + j + 1);
            live[j] = x < n_rows && low[j] != high[j];  // wavefront uniform
            const int last = max(high[j] - 1, low[j]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = live[j] ? min(low[j] + 64 * k + lane, last) : 0;
                vi[j][k] = indices[e];
                vr[j][k] = __float_as_uint(data[e]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + 16 * wave + u0 + j;
            y_i[j] = live[j] && b < n_batch ? sampler_index(seed, static_cast<uint64_t>(user_offset + x), iter0 + b, low[j], high[j]) : low[j];
            y[j] = 0;
            r[j] = 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!live[j]) continue;  // wavefront uniform
            if (high[j] - low[j] <= 256 * kRowRounds) {
                for (int base = low[j]; base < high[j]; base += 256) {
                    if (base > low[j]) {  // (rows above 256 ratings: the further rounds one after the other)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int e = min(base + 64 * k + lane, high[j] - 1);
                            vi[j][k] = indices[e];
                            vr[j][k] = __float_as_uint(data[e]);
                        }
                    }
                    const int pos = y_i[j] - base, src = pos & 63, kk = pos >> 6;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int yi = __shfl(vi[j][k], src);
                        const uint32_t ri = __shfl(vr[j][k], src);
                        if (kk == k && pos >= 0) y[j] = yi, r[j] = ri;
                    }
                }
            } else {
                y[j] = indices[y_i[j]];
                r[j] = __float_as_uint(data[y_i[j]]);
            }
        }
        int rank[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rank[j] = item_rank[y[j]];  // (item 0 for users without ratings: unused)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t key = live[j] ? static_cast<uint32_t>(rank[j]) : sentinel;
            t_key[b * kTileStride + 16 * wave + u0 + j] = key;
            t_rat[b * kTileStride + 16 * wave + u0 + j] = live[j] ? r[j] : 0u;
        }
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x < n_rows) {
        for (int bb = wave; bb < n_batch; bb += 4) {
            const uint32_t key = t_key[bb * kTileStride + lane];
            const size_t idx = static_cast<size_t>(bb) * n_rows + x;
            keys[idx] = key;
            vals[idx] = (key & sentinel) ? 0ull : (static_cast<uint64_t>(static_cast<uint32_t>(x)) << 32) | t_rat[bb * kTileStride + lane];
        }
    }
}

// ranges[b][r], r = 0 .. n_ranks: where the chains of the most popular items begin in every iteration of a sorted batch (ordered_keys.hpp)
__global__ __launch_bounds__(kBlock) void chain_ranges_kernel(const uint32_t *__restrict__ keys, int n_active, int n_ranks,
                                                              int *__restrict__ ranges, size_t stride) {
    find_chain_ranges(keys, n_active, n_ranks, ranges, stride);
}

// One launch = one iteration.  Two roles, chosen per block:
//  * blocks [0, hot_blocks): the chains of popularity ranks r < n_hot, DuoShape::kChains per block, in the two-wave
//    form (ordered_duo.hpp).  These are the long chains (thousands of updates on the most rated items), i.e. the critical path.
//  * the other blocks: walk_group (ordered_walk.hpp), one sorted position per 16-lane group.
template <int J>
__global__ __launch_bounds__(kBlock) void sgd_ordered_kernel(SgdArgs a, const uint32_t *__restrict__ keys,
                                                             const uint64_t *__restrict__ vals, int n_active,
                                                             const int *__restrict__ item_of_rank, int n_hot,
                                                             int hot_blocks, int rank_lo, const int *__restrict__ ranges,
                                                             int walk_lo, int walk_blocks) {
    // above the schedule's kernels (priority 0), which run BESIDE the iterations: where a wavefront of theirs shares a SIMD with one
    // of an iteration's, the iteration's goes first (a kernel ends with its slowest workgroup: profiles/r05_handwritten_sort_experiment.txt)
    __builtin_amdgcn_s_setprio(1);
    if (static_cast<int>(blockIdx.x) < hot_blocks) {
        // two-wave form for every row width: 32 lanes x 1 slot when 65 <= ld <= 128, else 16 lanes x J slots
        run_hot_block_duo<(J == 2 ? kWide : kGroup), (J == 2 ? 1 : J)>(a, vals, n_hot, item_of_rank, rank_lo, ranges);
        return;
    }
    // The walk: one 16-lane group per sorted position of [walk_lo, n_active) -- the tail of the sorted iteration, where the chains of
    // the unpopular items are (OrderedSchedule::walk_bound: the host knows how long that tail is, give or take a few hundred positions;
    // the positions in front of it belong to two-wave chains and used to cost a workgroup each just to find that out: 84 % of the walk's
    // workgroups on the Netflix shape).  One extra workgroup sweeps whatever walked chains an iteration has in FRONT of walk_lo.
    const int wb = static_cast<int>(blockIdx.x) - hot_blocks;
    if (wb < walk_blocks) {
        walk_group<J>(a, keys, vals, n_active, item_of_rank, n_hot, walk_lo + (wb * kBlock + static_cast<int>(threadIdx.x)) / kGroup);
        return;
    }
    const int sweep_lo = ranges[n_hot];  // first sorted position whose rank is >= n_hot (chain_ranges_kernel)
    for (int p = sweep_lo + static_cast<int>(threadIdx.x) / kGroup; p < walk_lo; p += kGroupsPerBlock)
        walk_group<J>(a, keys, vals, n_active, item_of_rank, n_hot, p);
}

// One iteration's chains of ranks >= rank_lo: the two-wave chains of ranks [rank_lo, n_hot) and the walk of the rest, one launch.
// ranges: the iteration's row of the chain-range table, ranks 0 .. n_hot at least.
template <int J>
void launch_chain(const SgdArgs &a, const uint32_t *keys, const uint64_t *vals, int n_active, const int *item_of_rank, int n_hot,
                  hipStream_t stream, int rank_lo, const int *ranges, hipEvent_t stop, int walk_bound) {
    const int chains_per_block = DuoShape<(J == 2 ? kWide : kGroup), (J == 2 ? 1 : J)>::kChains;
    const int hot_blocks = (std::max(n_hot - rank_lo, 0) + chains_per_block - 1) / chains_per_block;
    // the walk covers the last walk_bound positions (whole workgroups); one more workgroup sweeps what an iteration may have in front
    // of them (see the kernel)
    const int walk_lo = walk_bound < n_active ? ((n_active - walk_bound) / kGroupsPerBlock) * kGroupsPerBlock : 0;
    const int walk_blocks = (n_active - walk_lo + kGroupsPerBlock - 1) / kGroupsPerBlock;
    const int blocks = hot_blocks + walk_blocks + (walk_lo > 0 ? 1 : 0);
    if (blocks == 0) return;
    if (stop)  // the event rides on the kernel's completion signal (see launch_gram, blocksolve.hip)
        hipExtLaunchKernelGGL(sgd_ordered_kernel<J>, dim3(blocks), dim3(kBlock), 0, stream, nullptr, stop, 0, a, keys, vals, n_active,
                              item_of_rank, n_hot, hot_blocks, rank_lo, ranges, walk_lo, walk_blocks);
    else
        hipLaunchKernelGGL(sgd_ordered_kernel<J>, dim3(blocks), dim3(kBlock), 0, stream, a, keys, vals, n_active,
                           item_of_rank, n_hot, hot_blocks, rank_lo, ranges, walk_lo, walk_blocks);
}

void launch_chains(const SgdArgs &a, const uint32_t *kb, const uint64_t *vb, int n_active, const int *item_of_rank, int n_hot,
                   hipStream_t stream, int rank_lo, const int *ranges, hipEvent_t stop, int walk_bound) {
    dispatch_row_width(a.nslots, [&](auto j) {
        launch_chain<j()>(a, kb, vb, n_active, item_of_rank, n_hot, stream, rank_lo, ranges, stop, walk_bound);
    });
}

int bits_for(int n) {  // bits needed to represent values in [0, n)
    int b = 1;
    while ((1ll << b) < n) ++b;
    return b;
}

}  // namespace

// The one-off host pass over the CSR: users with ratings (n_active), item popularity rank (item_rank, item_of_rank) and the prefix
// sums of the expected updates per iteration by rank (rank_rate_prefix).  Returns those expected updates by rank.
std::vector<double> OrderedSchedule::rank_items(const int *d_indptr, const int *d_indices) {
    std::vector<int> indptr(static_cast<size_t>(n_rows) + 1), indices(static_cast<size_t>(std::max(nnz, 1)));
    CU2REC_HIP(hipMemcpy(indptr.data(), d_indptr, indptr.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (nnz) CU2REC_HIP(hipMemcpy(indices.data(), d_indices, static_cast<size_t>(nnz) * sizeof(int), hipMemcpyDeviceToHost));
    n_active = 0;
    for (int u = 0; u < n_rows; ++u) n_active += indptr[u + 1] > indptr[u];
    // popularity = expected updates per iteration: every user draws one of its ratings uniformly (sgd.cu:36-37), so an
    // item collects sum over its raters of 1 / degree; descending, ties by item id.  Ranks only order the chains
    // (longest first) and pick the hot ones; results do not depend on them.
    std::vector<double> rate(n_cols);
    std::vector<int> order(n_cols), rank(n_cols);
    for (int u = 0; u < n_rows; ++u) require(indptr[u] <= indptr[u + 1] && indptr[u + 1] <= nnz, "ordered schedule: bad indptr");
    item_update_rates(indptr.data(), indices.data(), n_rows, n_cols, rate.data());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int l, int r) { return rate[l] > rate[r]; });
    for (int r = 0; r < n_cols; ++r) rank[order[r]] = r;
    item_rank.allocate(n_cols);
    item_rank.upload(rank.data(), n_cols);
    item_of_rank.allocate(n_cols);
    item_of_rank.upload(order.data(), n_cols);
    std::vector<double> rank_rate(n_cols);  // expected updates per iteration by popularity rank
    for (int r = 0; r < n_cols; ++r) rank_rate[r] = rate[order[r]];
    rank_rate_prefix.assign(static_cast<size_t>(n_cols) + 1, 0.0);
    for (int r = 0; r < n_cols; ++r) rank_rate_prefix[r + 1] = rank_rate_prefix[r] + rank_rate[r];
    return rank_rate;
}

OrderedSchedule::OrderedSchedule(const int *d_indptr, const int *d_indices, int n_rows_, int n_cols_, int nnz_)
    : n_rows(n_rows_), n_cols(n_cols_), nnz(nnz_) {
    require(d_indptr && n_rows >= 0 && n_cols > 0 && nnz >= 0, "ordered schedule: bad argument");
    require_device();
    const std::vector<double> rank_rate = rank_items(d_indptr, d_indices);
    // a key is the item's popularity rank in item_bits bits; the bit above them is the sentinel of the users without ratings
    item_bits = bits_for(n_cols);
    // Window length: 2^min(6, 30 - item_bits) iterations -- 64 up to 2^24 items, halved with every bit of a larger catalogue -- and
    // halved further while a window holds more than 2^27 pairs (a pair takes 24 bytes of each slot: the sort's two key and two value
    // buffers).  A rule kept for its numbers: window length decides speed on large catalogues (tests/test_gpu_size_edges.py pins them).
    int b_bits = std::min(6, 31 - item_bits - 1);
    require(b_bits >= 0, "ordered schedule: too many items for 32-bit keys");
    max_batch = 1 << b_bits;
    while (max_batch > 1 && static_cast<size_t>(max_batch) * n_rows > (size_t(1) << 27)) max_batch >>= 1;
    const size_t cap = static_cast<size_t>(max_batch) * std::max(n_rows, 1);
    for (int slot = 0; slot < 2; ++slot)
        for (int i = 0; i < 2; ++i) {
            keys[slot][i].allocate(cap);
            vals[slot][i].allocate(cap);
        }
    temp_bytes = 0;
    {
        // every iteration of a batch is a segment of n_rows pairs of the sort
        std::vector<int> offs(static_cast<size_t>(max_batch) + 1);
        for (int b = 0; b <= max_batch; ++b) offs[b] = static_cast<int>(static_cast<size_t>(b) * n_rows);
        seg_offsets.allocate(offs.size());
        seg_offsets.upload(offs.data(), offs.size());
        CU2REC_HIP(rocprim::segmented_radix_sort_pairs<SegSortConfig>(nullptr, temp_bytes, keys[0][0].ptr, keys[0][1].ptr, vals[0][0].ptr,
                                                                       vals[0][1].ptr, static_cast<unsigned>(cap), static_cast<unsigned>(max_batch),
                                                                       seg_offsets.ptr, seg_offsets.ptr + 1, 0u, 32u, nullptr));
    }
    temp.allocate(temp_bytes + 16);
    const int n_hot_bs = blocksolve_hot_items(rank_rate, n_active, (1 << item_bits) - 1);
    if (n_hot_bs > 0)
        bs.reset(new BlockSolve(n_hot_bs, rank_rate, rank_rate_prefix[static_cast<size_t>(n_hot_bs)], n_active, max_batch, item_of_rank.ptr));
    // beside the block solves: chains expected to be at least 12 links long run in the ordered mode's two-wave form
    n_duo_bs = n_hot_bs;
    while (n_duo_bs < n_cols && n_duo_bs < 4096 && rank_rate[n_duo_bs] >= 12.0) ++n_duo_bs;
    n_duo_bs = std::min(n_duo_bs, (1 << item_bits) - 1);
    // The chain-range table covers every rank whose chain anyone looks up: with M = (1 << item_bits) - 1, the ordered mode's
    // n_hot = min(min(n_cols, kHotChains), M) (run()) is at most min(max(min(n_cols, kHotChains), ...), M) = n_range_ranks, and
    // n_duo_bs and n_hot_bs are each at most M and at most the maximum below, so block-solve mode's max(n_duo_bs, n_hot_bs) is too.
    n_range_ranks = std::max(std::max(std::min(n_cols, kHotChains), n_duo_bs), n_hot_bs);
    n_range_ranks = std::min(n_range_ranks, (1 << item_bits) - 1);
    for (int slot = 0; slot < 2; ++slot) chain_ranges[slot].allocate(static_cast<size_t>(max_batch) * (n_range_ranks + 1));
    {
        // The next batch's schedule is built beside the iterations that consume this batch's, on a stream of the lowest priority
        // (measured: no different from the default priority -- what its kernels cost the iterations is DESIGN.md section 4)
        int lo = 0, hi = 0;
        CU2REC_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        CU2REC_HIP(hipStreamCreateWithPriority(&sched, hipStreamNonBlocking, lo));
    }
    for (int slot = 0; slot < 2; ++slot) {
        CU2REC_HIP(hipEventCreateWithFlags(&ev_ready[slot], hipEventDisableTiming));
        CU2REC_HIP(hipEventCreateWithFlags(&ev_consumed[slot], hipEventDisableTiming));
    }
    CU2REC_HIP(hipEventCreateWithFlags(&ev_last, hipEventDisableTiming));
}

OrderedSchedule::~OrderedSchedule() {
    // queued work may still read the buffers this object owns
    if (have_last) (void)hipEventSynchronize(ev_last);
    if (sched) (void)hipStreamSynchronize(sched);
    if (sched) (void)hipStreamDestroy(sched);
    for (int slot = 0; slot < 2; ++slot) {
        if (ev_ready[slot]) (void)hipEventDestroy(ev_ready[slot]);
        if (ev_consumed[slot]) (void)hipEventDestroy(ev_consumed[slot]);
    }
    if (ev_last) (void)hipEventDestroy(ev_last);
}

// How many sorted positions the walk behind popularity rank n_hot has to cover in one iteration, as an upper bound that holds in all but
// astronomically rare iterations: a user lands behind rank n_hot with probability 1 - (its ratings of the n_hot most popular items) / (its
// ratings), independently; the count's mean is n_active - rank_rate_prefix[n_hot] and its variance at most that mean.  Mean + 8 sigma + 64.
// The launch covers exactly that many positions at the END of the sorted iteration (where the unpopular items' chains are); whatever an
// iteration has beyond it is swept by one extra workgroup (sgd_ordered_kernel), so the bound is about speed, never about results.
int OrderedSchedule::walk_bound(int n_hot) const {
#ifdef CU2REC_TEST_HOOKS  // (fault-path tests: a bound far too small, so that the sweeper does nearly all of the walk)
    if (const char *env = std::getenv("CU2REC_BS_DBG"))
        if (std::atoi(env) & 256) return 16;
#endif
    const int r = std::min(std::max(n_hot, 0), n_cols);
    const double mean = std::max(0.0, static_cast<double>(n_active) - rank_rate_prefix[static_cast<size_t>(r)]);
    const double bound = mean + 8.0 * std::sqrt(mean) + 64.0;
    return bound >= static_cast<double>(n_active) ? n_active : static_cast<int>(bound);
}

// Which slot's window holds iteration `it` of this (seed, user offset, indptr address, mode), or -1.  Windows are keyed on exactly
// those: with `speculate` (owned cu2rec_csr objects only) the CSR arrays are IMMUTABLE for the object's lifetime, which is what lets a
// window outlive the call that scheduled it.
int OrderedSchedule::slot_holding(const SgdArgs &a, uint64_t it, bool blocksolve) const {
    for (int slot = 0; slot < 2; ++slot) {
        const Window &w = win[slot];
        if (w.valid && w.seed == a.seed && w.user_offset == a.user_offset && w.indptr == a.indptr && w.blocksolve == blocksolve &&
            it >= w.iter_begin && it < w.iter_begin + static_cast<uint64_t>(w.nb))
            return slot;
    }
    return -1;
}

// Sample + sort + chain ranges (+ plan) of the window [first_iter, first_iter + nb) into a slot, on the schedule stream: nothing in it
// depends on the model.  The key is the item's popularity rank, and every iteration of the window is sorted as a segment of its own
// (stable, so users stay ascending inside a chain); iteration b of the window occupies [b * n_rows, b * n_rows + n_active) of the
// sorted arrays.
void OrderedSchedule::schedule_window(const SgdArgs &a, int slot, uint64_t first_iter, int nb, bool blocksolve) {
    win[slot].valid = false;
    // (the window is published only when everything below has been queued -- a launch that throws leaves none behind)
    const size_t n = static_cast<size_t>(nb) * n_rows;
    if (slot_used[slot]) CU2REC_HIP(hipStreamWaitEvent(sched, ev_consumed[slot], 0));  // its last window has been run
    hipLaunchKernelGGL(schedule_keys_tile_kernel, dim3((n_rows + 63) / 64), dim3(256), 0, sched, a.indptr, a.indices, a.data,
                       item_rank.ptr, n_rows, nb, 1u << item_bits, a.seed, first_iter, a.user_offset, keys[slot][0].ptr, vals[slot][0].ptr);
    CU2REC_HIP(hipGetLastError());
    size_t bytes = temp_bytes;
    CU2REC_HIP(rocprim::segmented_radix_sort_pairs<SegSortConfig>(temp.ptr, bytes, keys[slot][0].ptr, keys[slot][1].ptr, vals[slot][0].ptr,
                                                                   vals[slot][1].ptr, static_cast<unsigned>(n), static_cast<unsigned>(nb),
                                                                   seg_offsets.ptr, seg_offsets.ptr + 1, 0u,
                                                                   static_cast<unsigned>(item_bits + 1), sched));
    Window w{true, a.seed, first_iter, nb, a.user_offset, a.indptr, blocksolve, keys[slot][1].ptr, vals[slot][1].ptr};
    hipLaunchKernelGGL(chain_ranges_kernel, dim3(nb), dim3(kBlock), 0, sched, w.sk, n_active, n_range_ranks, chain_ranges[slot].ptr,
                       static_cast<size_t>(n_rows));
    CU2REC_HIP(hipGetLastError());
    if (blocksolve) bs->plan(slot, chain_ranges[slot].ptr, n_range_ranks + 1, nb, sched);  // (reads the table just queued)
    CU2REC_HIP(hipEventRecord(ev_ready[slot], sched));
    slot_used[slot] = true;
    win[slot] = w;
}

// No window holds the call's next iteration (first call, another seed / offset / mode, a jump in the iteration number): a window for
// what the call needs is scheduled into slot 0 now, and the call's next iteration waits for it.
void OrderedSchedule::restart(const SgdArgs &a, uint64_t first_iter, int nb, bool blocksolve, hipStream_t stream) {
    // the CSR / model pointers the schedule reads must be final: whatever the caller queued on `stream` so far
    CU2REC_HIP(hipEventRecord(ev_consumed[1], stream));
    CU2REC_HIP(hipStreamWaitEvent(sched, ev_consumed[1], 0));
    slot_used[1] = true;  // (that record also stands for "slot 1 free": nothing of it is queued behind this point)
    win[1].valid = false;
    schedule_window(a, 0, first_iter, nb, blocksolve);
}

void OrderedSchedule::run(SgdArgs a, uint64_t iter0, int n_iters, hipStream_t stream, bool blocksolve) {
    if (n_active == 0) return;
    if (blocksolve && !bs) blocksolve = false;  // nothing to solve block-wise: the ordered walk, bit for bit
    // A decay factor a = 1 - lr Q_reg or c = 1 - lr item_bias_reg at or below zero has no logarithm: the cross-tile terms
    // exp2(d * log2 a) would be NaN (0 * -inf at d = 0).  The sequential update is still defined there: the ordered walk, bit for bit.
    // (In double, as the decay tables are.)
    if (blocksolve && (1.0 - static_cast<double>(a.h.lr) * static_cast<double>(a.h.q_reg) <= 0.0 ||
                       1.0 - static_cast<double>(a.h.lr) * static_cast<double>(a.h.ib_reg) <= 0.0))
        blocksolve = false;
    // The workspace (key / value buffers, block records, events) exists once: a call on another stream than the last one
    // starts behind that call's end.
    if (have_last && last_stream != stream) CU2REC_HIP(hipStreamWaitEvent(stream, ev_last, 0));
    if (blocksolve) bs->begin(a, stream);  // (before any window work)
    // ranks [0, n_hot) get a dedicated group each with deep prefetch; keep r + 1 below the sentinel bit
    const int n_hot = std::min(std::min(n_cols, kHotChains), (1 << item_bits) - 1);
    // positions the walk covers per iteration (its tail of the sorted order): behind the two-wave chains of either mode
    const int n_hot_bs = blocksolve_items(), n_side = std::max(n_duo_bs, n_hot_bs);
    const int walk_bound_plain = walk_bound(n_hot), walk_bound_bs = walk_bound(n_side);
    const size_t seg = static_cast<size_t>(n_rows);  // an iteration's stride in the sorted arrays
    // (raw pointers: the arrays behind them are the caller's and may change between calls -- no window outlives the call, whether
    // it returns or throws)
    struct DropWindows {
        OrderedSchedule *s;
        ~DropWindows() { if (!s->speculate) s->win[0].valid = s->win[1].valid = false; }
    } drop_windows{this};
    // the iteration being launched, and (block-solve mode) the launch of its other chains beside the hot ones
    const uint32_t *kb = nullptr;
    const uint64_t *vb = nullptr;
    const int *ranges = nullptr;
    const BlockSolve::SideChains side_chains = [&](hipStream_t side, hipEvent_t stop) {
        launch_chains(a, kb, vb, n_active, item_of_rank.ptr, n_side, side, n_hot_bs, ranges, stop, walk_bound_bs);
    };
    int done = 0;
    while (done < n_iters) {
        // A call usually continues where the last one stopped (cu2rec_train's segments, a bench's steps, a sharded run's periods): its
        // iterations are then already scheduled -- in the window the earlier calls have been running out of, or in the one that was
        // scheduled ahead beside them.  Otherwise the schedule restarts with a window for what this call still needs.
        const uint64_t it_first = iter0 + static_cast<uint64_t>(done);
        int slot = slot_holding(a, it_first, blocksolve);
        if (slot < 0) {
            restart(a, it_first, std::min(max_batch, n_iters - done), blocksolve, stream);
            slot = 0;
        }
        const int off = static_cast<int>(it_first - win[slot].iter_begin);  // the window's iterations [off, off + nb) are this batch
        const int nb = std::min(n_iters - done, win[slot].nb - off);
        // The window BEHIND this one is scheduled beside this batch's iterations unless it exists already: as far as this call goes
        // on, or -- for the calls to come (`speculate`) -- a whole max_batch.  It is queued (on its own stream) BEHIND this batch's
        // first iterations in host order: queueing it costs the host tens of microseconds, and at the start of a call the device is
        // idle -- with the schedule queued first, the call's first phase 1 started ~100 us after the call did (kernel traces, round 4).
        const uint64_t next_begin = win[slot].iter_begin + static_cast<uint64_t>(win[slot].nb);
        const long long call_beyond = static_cast<long long>(iter0 + static_cast<uint64_t>(n_iters)) - static_cast<long long>(next_begin);
        const int next_nb = speculate ? max_batch : static_cast<int>(std::min<long long>(max_batch, call_beyond));
        const int ahead = slot_holding(a, next_begin, blocksolve);  // (never `slot`: next_begin is the first iteration behind its window)
        bool next_due = next_nb > 0 && !(ahead >= 0 && win[ahead].iter_begin == next_begin);
        CU2REC_HIP(hipStreamWaitEvent(stream, ev_ready[slot], 0));
        const uint32_t *sk = win[slot].sk + static_cast<size_t>(off) * seg;   // (the batch's first iteration inside the window)
        const uint64_t *sv = win[slot].sv + static_cast<size_t>(off) * seg;
        a.iters = 1;
        for (int b = 0; b < nb; ++b) {
            if (next_due && b == std::min(2, nb - 1) && b > 0) {  // (two iterations are queued: the device has work)
                next_due = false;
                schedule_window(a, slot ^ 1, next_begin, next_nb, blocksolve);
            }
            a.iter0 = iter0 + done + b;
            kb = sk + static_cast<size_t>(b) * seg;
            vb = sv + static_cast<size_t>(b) * seg;
            ranges = chain_ranges[slot].ptr + static_cast<size_t>(off + b) * (n_range_ranks + 1);
            if (blocksolve) bs->iteration(a, slot, off + b, kb, vb, b == nb - 1, stream, side_chains);
            else launch_chains(a, kb, vb, n_active, item_of_rank.ptr, n_hot, stream, 0, ranges, nullptr, walk_bound_plain);
        }
        if (next_due) schedule_window(a, slot ^ 1, next_begin, next_nb, blocksolve);  // (a batch of one iteration)
        CU2REC_HIP(hipGetLastError());
        if (blocksolve) bs->join(stream);  // the batch's slot is free once both streams are through with it
        CU2REC_HIP(hipEventRecord(ev_consumed[slot], stream));
        done += nb;
    }
    if (blocksolve) bs->end(stream);
    CU2REC_HIP(hipEventRecord(ev_last, stream));
    last_stream = stream;
    have_last = true;
}

}  // namespace cu2rec
