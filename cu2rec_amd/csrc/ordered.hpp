// Workspace + driver of the ordered (sequential-semantics, deterministic) SGD mode; see ordered.hip.
#pragma once

#include <memory>
#include <vector>

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hip_check.hpp"
#include "blocksolve.hpp"
#include "kernels.hpp"

namespace cu2rec {

struct OrderedSchedule {
    // d_indptr / d_indices: the device CSR the schedule will be used with (read once, on the host, to rank the
    // items by popularity and count the users that have ratings).
    OrderedSchedule(const int *d_indptr, const int *d_indices, int n_rows, int n_cols, int nnz);
    // Runs iterations [iter0, iter0 + n_iters) of `a` (pointers, hyper-parameters, seed, user_offset filled in).
    // blocksolve: the chains of the hot items are solved block-wise (blocksolve.hip) instead of walked link by link:
    // the same sequential semantics up to float rounding, not bit for bit.
    void run(SgdArgs a, uint64_t iter0, int n_iters, hipStream_t stream, bool blocksolve = false);

    int n_rows, n_cols, nnz;
    int n_active = 0;   // users with at least one rating = updates per iteration
    int item_bits = 0;  // a sorted key is the item's popularity rank, below 1 << item_bits; users without ratings carry that one bit instead
    int max_batch = 1;  // iterations per window (sampled + sorted in one pass)
    DeviceBuffer<int> item_rank, item_of_rank;
    // Two schedule slots: the sample stream is value independent, so batch j + 1 is sampled and sorted on a stream of
    // its own while batch j's iterations run.  Per slot: the radix sort's two key / value buffers.
    DeviceBuffer<uint32_t> keys[2][2];
    DeviceBuffer<uint64_t> vals[2][2];
    hipStream_t sched = nullptr;
    hipEvent_t ev_ready[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
    bool slot_used[2] = {false, false};
    // Schedule the next call's first batch ahead (it reads the CSR arrays after run() has returned): only where the
    // schedule lives and dies with the CSR it reads, i.e. the owned-object layer (cu2rec_csr), whose arrays are IMMUTABLE for the
    // object's lifetime -- windows are keyed on (seed, user offset, indptr address, mode), not on the arrays' contents; off for raw
    // pointers, whose windows never outlive the call.
    bool speculate = false;
    // A scheduled WINDOW of iterations per slot: [iter_begin, iter_begin + nb) of one (seed, user offset, CSR, mode).  A call runs the
    // iterations it asks for out of whichever window holds them, at whatever offset -- so calls shorter than a window (a bench's
    // 20 steps, a driver's periods) share one schedule of max_batch iterations instead of paying for a schedule each.
    struct Window {
        bool valid = false;
        uint64_t seed = 0, iter_begin = 0;
        int nb = 0, user_offset = 0;
        const int *indptr = nullptr;
        bool blocksolve = false;
        const uint32_t *sk = nullptr;
        const uint64_t *sv = nullptr;
    } win[2];
    DeviceBuffer<unsigned char> temp;
    DeviceBuffer<int> seg_offsets;  // [max_batch + 1] b * n_rows: the iterations of a batch as segments of the sort
    size_t temp_bytes = 0;
    // block-solve mode (blocksolve.hip): items are ranked by their expected updates per iteration (sum over raters of 1 / degree); the
    // block-wise solved ones are ranks [0, bs->n_hot); no BlockSolve when no item qualifies (the mode is then the ordered walk)
    std::unique_ptr<BlockSolve> bs;
    int blocksolve_items() const { return bs ? bs->n_hot : 0; }
    int n_duo_bs = 0;  // block-solve mode: ranks [bs->n_hot, n_duo_bs) run in the two-wave form beside the block solves
    // per schedule slot: [iteration of the window][rank 0 .. n_range_ranks] first sorted position of the chains of the most
    // popular items (chain_ranges_kernel, behind the sort).  The ONE table of where chains begin: the two-wave blocks, the walk's
    // sweeper and the block-solve plan (BlockSolve::plan) read it
    DeviceBuffer<int> chain_ranges[2];
    int n_range_ranks = 0;
    // rank_rate_prefix[r] = expected updates per iteration of the r most popular items together (host; [n_cols + 1]): what the walk
    // behind rank r has to cover is n_active minus that, give or take its square root (walk_bound)
    std::vector<double> rank_rate_prefix;
    int walk_bound(int n_hot) const;
    // one stream at a time per schedule: a call on another stream than the last one first waits for that call's end
    hipEvent_t ev_last = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    ~OrderedSchedule();
    // CONSTRUCTOR ONLY (it allocates and fills what the constructor's other steps size their buffers by): the one-off host pass over
    // the CSR that sets n_active, item_rank / item_of_rank and rank_rate_prefix; returns the rates by rank
    std::vector<double> rank_items(const int *d_indptr, const int *d_indices);
    // the pieces of run(): which slot's window holds iteration `it` of this (seed, user offset, indptr, mode), or -1; queueing a
    // window into a slot on `sched`; starting over in slot 0 when no window holds what the call needs
    int slot_holding(const SgdArgs &a, uint64_t it, bool blocksolve) const;
    void schedule_window(const SgdArgs &a, int slot, uint64_t first_iter, int nb, bool blocksolve);
    void restart(const SgdArgs &a, uint64_t first_iter, int nb, bool blocksolve, hipStream_t stream);
};

}  // namespace cu2rec
