// Launch interface of the block-solve SGD mode (CU2REC_SGD_BLOCKSOLVE): sequential semantics
// (mf_sequential.cu:102-143) with the long item chains solved block-wise; see blocksolve.hip (entry points, launches) and the
// phase headers it includes (blocksolve_gram.hpp, blocksolve_solve.hpp, blocksolve_lookahead.hpp, blocksolve_update.hpp).
#pragma once

#include <functional>
#include <vector>

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hip_check.hpp"
#include "kernels.hpp"

namespace cu2rec {

constexpr int kBsLinks = 64;                        // updates ("links") of a chain per block
constexpr int kBsTableStride = 2 * kBsLinks + 1;    // tables: 1 - a^k, 1 - c^k, a^k, c^k for k = 0..2 kBsLinks (a block and its look-ahead)
constexpr int kBsTableFloats = 4 * kBsTableStride;
constexpr int kBsFactorFloats = 3 * 32 * 32;        // inverse factor of a block: tiles M11, M21, M22 (32 x 32 each, row major)
constexpr int kBsRecFloats = kBsFactorFloats + kBsLinks;  // a block's record from phase 1: the factor, then r - gb - ub per link
constexpr int kBsCrossFloats = kBsLinks * kBsLinks;  // look-ahead chains: the 64 x 64 block of lr L that couples a block (rows) to the one before it (columns)
constexpr int kBsMaxSlots = 63;                     // float4 slots per row the solver has LDS for (n_factors <= 252)

struct BsBlockDesc {  // up to 64 consecutive links of one hot chain
    int pos0;      // sorted position of the first link
    int n_valid;   // links in the block (the last block of a chain may be partial); 0 = unused table entry
    int chain;     // popularity rank of the item
    int m;         // block number inside the chain
};

struct BsChainDesc {  // the updates of one iteration that hit one hot item, users ascending
    int begin, len;  // sorted positions [begin, begin + len)
    int blk0;        // index of the chain's first block
    int item;
};

// One iteration's view of the sorted schedule (ordered.hip) and of the scratch buffers; all device pointers.
struct BsIteration {
    const uint32_t *keys;     // [n_active] sorted keys of this iteration
    const uint64_t *vals;     // [n_active] user << 32 | rating bits
    int n_active;
    int n_hot;                // popularity ranks [0, n_hot) are solved block-wise, the others walked link by link
    const BsChainDesc *chains;  // [n_hot]
    const BsBlockDesc *blocks;  // [max_blocks]
    const int *item_of_rank;
    const float *tables;      // [kBsTableFloats]
    float log2a, log2c;       // log2(1 - lr * Q_reg), log2(1 - lr * item_bias_reg)
    float *Mbuf;              // [max_blocks][kBsRecFloats]  (I + lr L)^-1 of each block | r - gb - ub of its links
    float *ebuf;              // [max_blocks][kBsLinks]      error of each hot link
    float *qstart;            // [max_blocks][ldq]           item row at the start of each block
    int max_blocks;
    // workgroups phase 3 is LAUNCHED with (<= max_blocks; phase 1 keeps the full grid: blocksolve.hip): what an iteration is expected to have, mean + 8 sigma of the hot links
    // (BlockSolve's constructor); the block table is dense and the workgroups stride through it, so a busier iteration is still
    // done completely
    int launch_blocks;
    // Look-ahead chains (blocksolve_lookahead.hpp, "the look-ahead form"): popularity ranks [0, la_ranks) -- the long chains, whose length IS the
    // iteration's critical path.  Phase 1 also builds the block of lr L that couples each of their blocks to the one before it
    // (la_grid more workgroups in its launch), and phase 2 runs them with the item row OFF the dependent path.
    int la_ranks;
    int la_cap;               // ... whose blocks all lie below la_cap (Nbuf has room for that many; a chain beyond it runs in the plain form)
    int la_grid;              // workgroups of phase 1's launch that build the cross blocks
    float *Nbuf;              // [la_cap][kBsCrossFloats]
    unsigned *status;                 // [1] set by a wait that gave up (bounded spins); the host reports it
    // Fork and join of the side stream without events (BlockSolve::iteration): phase 1's workgroups count themselves through and phase 2's
    // count themselves in -- ONE wavefront queued in front of the side kernel (bs_gate_kernel) ends when both counts have reached
    // what the host has launched so far (timing only, no data behind it); a signal kernel behind the side kernel stores the
    // iteration's number, and one extra workgroup of phase 3's launch waits for it (data: the next phase 1 reads rows the side kernel
    // writes).
    unsigned long long *solve_started;   // [1]  phase-2 workgroups started, over all iterations so far
    const unsigned long long *side_seq;  // (or null) the word the signal kernel sets ...
    unsigned long long side_target;      // ... and the number the extra workgroup of phase 3's launch waits for
    unsigned long long *gram_done;       // [32 x 16]  phase-1 workgroups through (32 shards, 128 bytes apart), over all iterations so far (or null)
    unsigned long long wait_ticks;    // bound of the device-side waits (CU2REC_BS_WAIT_S, 2 s), 100 MHz ticks
};

// minimum expected updates per iteration of an item for block-wise treatment (process-wide; schedules created later)
// rate > 0 sets it, rate < 0 returns to automatic (scaled with the set), 0 queries; returns the explicit value in force before
// the call or -1 for automatic
float blocksolve_min_rate(float rate);
// chains EXPECTED to be at least this many blocks of 64 links long run phase 2 in the look-ahead form (default 24: the top chains; 0: none;
// schedules created later); blocks < 0 only queries
int blocksolve_lookahead_blocks(int blocks);
// popularity ranks [0, n) that are solved block-wise, n <= rank_limit (rate: expected updates per iteration of the items by rank)
int blocksolve_hot_items(const std::vector<double> &rate, int n_active, int rank_limit);

// The host side of the block-solve mode for one ordered schedule (ordered.hip), which samples and sorts the iterations: the buffers of the
// three phases, the plan of every scheduled iteration, the side stream the other items' chains run on, and the launch sequence.
class BlockSolve {
public:
    // ranks [0, n_hot) are solved block-wise; hot_rate = rate[0] + ... + rate[n_hot - 1]
    BlockSolve(int n_hot, const std::vector<double> &rate, double hot_rate, int n_active, int max_batch, const int *item_of_rank);
    ~BlockSolve();
    BlockSolve(const BlockSolve &) = delete;
    BlockSolve &operator=(const BlockSolve &) = delete;
    // schedule slot `slot` now holds nb sorted iterations: queues their chain and block tables on `sched`, behind the kernel that fills
    // chain_ranges -- [nb][range_stride], range_stride > n_hot: where the chain of every rank r <= n_hot begins (OrderedSchedule::chain_ranges)
    void plan(int slot, const int *chain_ranges, int range_stride, int nb, hipStream_t sched);
    // A call's start: decay tables, scratch, the side stream (behind everything queued on `stream` so far) and the fork / join topology.
    void begin(const SgdArgs &a, hipStream_t stream);
    // One iteration (a.iter0): the plan of iteration `b` of slot `slot`, its sorted keys and values.  `side` launches the other items'
    // chains on the stream it is given, with `stop` (or null) riding on their completion.  last: the last iteration of the batch.
    using SideChains = std::function<void(hipStream_t side, hipEvent_t stop)>;
    void iteration(const SgdArgs &a, int slot, int b, const uint32_t *keys, const uint64_t *vals, bool last, hipStream_t stream,
                   const SideChains &side);
    void join(hipStream_t stream);  // the batch's end: `stream` waits for the side stream
    void end(hipStream_t stream);   // the call's end: refreshes the host copy of the status word

    const int n_hot;

private:
    int n_active, max_batch;
    const int *item_of_rank;
    int max_blocks;     // blocks of 64 links (kBsLinks) per iteration, upper bound
    int launch_blocks;  // workgroups phase 3 is launched with (BsIteration::launch_blocks)
    int la_ranks = 0;   // ranks [0, la_ranks): phase 2 in the look-ahead form; their blocks lie below la_cap
    int la_cap = 0;
    // per schedule slot, per iteration: the plan (bs_plan_kernel)
    DeviceBuffer<BsChainDesc> chains[2];
    DeviceBuffer<BsBlockDesc> blocks[2];
    DeviceBuffer<float> tables, Mbuf, ebuf, qstart, Nbuf;  // Nbuf: [la_cap][kBsCrossFloats] the cross blocks of the look-ahead chains
    int qstart_ld = 0;
    SgdHyper tables_for{};  // hyper-parameters the decay tables were computed from
    bool tables_valid = false;
    // Fork and join without events (blocksolve.hip, "the launch topology"): what phase 1's and phase 2's workgroups count, what the host
    // has launched so far, and the number of the last iteration whose side kernel is complete (the signal kernel's word)
    DeviceBuffer<unsigned long long> solve_started, gram_done, side_seq;
    unsigned long long gram_done_target = 0, started_total = 0, side_seq_host = 0;
    hipStream_t upd = nullptr;
    hipEvent_t ev_call = nullptr, ev_upd = nullptr, ev_gram = nullptr;
    BsIteration it{};       // the call's launch arguments; iteration() sets the fields of one iteration
    bool device_join = false;
    bool upd_pending = false;  // (event join) a side kernel of this batch has not been waited for yet
    unsigned *host_status = nullptr;
};

}  // namespace cu2rec
