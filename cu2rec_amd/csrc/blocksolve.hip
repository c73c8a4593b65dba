// Block-solve SGD (CU2REC_SGD_BLOCKSOLVE): the sequential semantics of mf_sequential.cu:102-143 at Hogwild-class
// speed.  Same schedule as the ordered mode (ordered.hip: counter-based sample stream -> per-iteration item chains,
// users ascending inside a chain), but a long chain is no longer walked one dependent update at a time.
//
// A chain is a sequence of affine rank-1 maps on the item's state (q, b).  For a block of B = 64 consecutive links with
// user rows p_k, a = 1 - lr*Q_reg, c = 1 - lr*item_bias_reg (tests/test_blocksolve_algebra.py pins these formulas):
//     (I + lr L) e = rhs,   L_kj  = c^(k-1-j) + a^(k-1-j) (p_k . p_j)  for j < k           unit lower triangular
//                           rhs_k = (r_k - gb - ub_k) - c^k b0 - a^k (p_k . q0)
//     q_end = a^B q0 + lr sum_j a^(B-1-j) e_j p_j,   b_end likewise
//     p_k'  = p_k + lr (e_k q^(k) - P_reg p_k),   q^(k) = a^k q0 + lr sum_{j<k} a^(k-1-j) e_j p_j
// Inside one iteration every user occurs once, so the user rows -- and with them L -- do not depend on any chain's
// progress.  Per iteration:
//   phase 1  bs_gram_kernel    every block of every hot chain in parallel, one wavefront each: the Gram matrix of the
//                              block's 64 user rows on the matrix cores (v_mfma_f32_32x32x2_f32: exact f32), scaled into
//                              lr*L, and its inverse factor M = (I + lr L)^-1 (two 32x32 triangular inversions on the
//                              vector unit, the off-diagonal tile as two more matrix products) -- so that e = M rhs
//   phase 2  bs_solve_kernel   one workgroup per hot chain walks its blocks, lane = link, four solver wavefronts splitting
//                              each step (a mat-vec with the block's rows, a mat-vec with M, a transposed mat-vec) -- the only
//                              sequential part; four more wavefronts stream the blocks' rows and factors global -> registers
//                              -> LDS, four blocks ahead; the leading (longest) chains in the look-ahead form, whose dependent
//                              path per block is two 64 x 64 mat-vecs on one wavefront (chain_lookahead)
//   phase 3  bs_update_kernel  every block in parallel: one wavefront per 64 columns walks down the block's links with the
//                              reference's own recurrence, the item row as each link saw it in a register; user rows and biases
//   beside   the other chains  in the ordered mode's own kernel (ordered.hip: two-wave form for chains of a dozen links
//                              and more, windowed walk for the rest) on a second stream: other items, other users
// Results equal the sequential ones up to float rounding (not bit for bit: the sums are associated differently).
//
// This file: the __global__ entry points, their launches, the fork / join topology and class BlockSolve.  What the kernels run is in
// one header per phase, each readable without the others, over one shared header:
//   blocksolve_device.hpp     geometry, table offsets, vector types, lane exchanges, chain_is_lookahead
//   blocksolve_gram.hpp       phase 1: gram_block, gram_cross_block, gram_lds_bytes
//   blocksolve_solve.hpp      phase 2, plain form: solve_chain<SW>, solve_lds_bytes
//   blocksolve_lookahead.hpp  phase 2, look-ahead form: chain_lookahead<NSM>, the bounded waits, la_lds_bytes
//   blocksolve_update.hpp     phase 3: update_block, await_iteration_end
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "blocksolve.hpp"
#include "blocksolve_device.hpp"
#include "blocksolve_gram.hpp"
#include "blocksolve_lookahead.hpp"
#include "blocksolve_solve.hpp"
#include "blocksolve_update.hpp"
#include "hip_check.hpp"

namespace cu2rec {

namespace {

using namespace bs_dev;

// ---- decay tables: x * a^k is applied as x - adel[k] * x so that the rounding of a^k (one ulp of 1.0, the same sign
// every block) cannot bias a hot item's decay rate; the deltas are computed in double from the float hyper-parameters
__global__ void bs_tables_kernel(SgdHyper h, float *__restrict__ t) {
    const int k = threadIdx.x;
    if (k > 2 * kB) return;
    const double a = 1.0 - static_cast<double>(h.lr) * static_cast<double>(h.q_reg);
    const double c = 1.0 - static_cast<double>(h.lr) * static_cast<double>(h.ib_reg);
    double ak = 1.0, ck = 1.0;
    for (int i = 0; i < k; ++i) {
        ak *= a;
        ck *= c;
    }
    t[kTabAdel + k] = static_cast<float>(1.0 - ak);
    t[kTabCdel + k] = static_cast<float>(1.0 - ck);
    t[kTabApow + k] = static_cast<float>(ak);
    t[kTabCpow + k] = static_cast<float>(ck);
}

// ---- plan: one workgroup per iteration of the batch --------------------------------------------------------------
// chain_ranges: the window's table of where the chains begin (chain_ranges_kernel, ordered.hip, queued in front of this kernel on the
// same stream): iteration b's chain of rank r is [cb[r], cb[r + 1]) with cb = chain_ranges + b * range_stride, range_stride > n_hot
__global__ __launch_bounds__(256) void bs_plan_kernel(const int *__restrict__ chain_ranges, int range_stride, int n_hot, int max_blocks,
                                                      const int *__restrict__ item_of_rank, BsChainDesc *__restrict__ chains,
                                                      BsBlockDesc *__restrict__ blocks) {
    __shared__ int s_part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int *cb = chain_ranges + static_cast<size_t>(b) * range_stride;
    BsChainDesc *cd = chains + static_cast<size_t>(b) * max(n_hot, 1);
    BsBlockDesc *bd = blocks + static_cast<size_t>(b) * max_blocks;
    // blocks per chain -> exclusive prefix; thread t owns the chains [t * per, (t + 1) * per)
    const int per = (n_hot + 255) / 256;
    const int r0 = min(tid * per, n_hot), r1 = min(r0 + per, n_hot);
    int mine = 0;
    for (int r = r0; r < r1; ++r) mine += (cb[r + 1] - cb[r] + kB - 1) / kB;
    s_part[tid] = mine;
    __syncthreads();
    __shared__ int s_total;
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = s_part[t];
            s_part[t] = run;
            run += v;
        }
        s_total = run;
    }
    __syncthreads();
    int off = s_part[tid];
    for (int r = r0; r < r1; ++r) {
        const int begin = cb[r], len = cb[r + 1] - begin;
        cd[r] = BsChainDesc{begin, len, off, item_of_rank[r]};
        const int nb = (len + kB - 1) / kB;
        for (int m = 0; m < nb; ++m) bd[off + m] = BsBlockDesc{begin + kB * m, min(kB, len - kB * m), r, m};
        off += nb;
    }
    for (int g = s_total + tid; g < max_blocks; g += 256) bd[g] = BsBlockDesc{0, 0, 0, 0};
}

__global__ __launch_bounds__(256, 4) void bs_gram_kernel(SgdArgs a, BsIteration it) {
    extern __shared__ float4 bs_smem[];
    const int g = static_cast<int>(blockIdx.x) - it.la_grid;  // (the first la_grid workgroups of the launch: the cross blocks)
    __builtin_amdgcn_s_setprio(2);  // (above the walk beside us and the schedule's kernels: this launch is on the iteration's critical path)
    // (every workgroup counts itself through, used or not: the side stream's gate waits for the whole grid)
    struct Through {
        unsigned long long *count;
        __device__ ~Through() {
            // 32 shards, 128 bytes apart: two thousand atomics on ONE word took longer than phase 1 itself
            if (count && threadIdx.x == 0)
                __hip_atomic_fetch_add(count + 16 * (blockIdx.x & 31), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } through_count{it.gram_done};
    if (g < 0) {
        // the cross blocks of the look-ahead chains, whose blocks are the first of the table; dispatched first: they have nothing to
        // wait for and end long before the inversions do
        const BsChainDesc last = it.chains[it.la_ranks - 1];
        const int la_end = min(last.blk0 + (last.len + kB - 1) / kB, it.la_cap);
        for (int gb = g + it.la_grid; gb < la_end; gb += it.la_grid) gram_cross_block(a, it, gb, bs_smem);
        return;
    }
    // (one workgroup per slot of the block table, max_blocks of them -- the worst case; most find their descriptor empty and leave.  Launching
    // only as many as an iteration is expected to fill needs a way to do the rest when an iteration has more: as a stride loop around
    // gram_block it cost this kernel 55 spilled registers, as an out-of-line function a scratch frame -- 92 instead of 79 us per
    // iteration on the ML-20M shape either way (round 6, profiles/r06_launch_bounds.txt).  Phase 3 and the walk, whose kernels have the
    // registers to spare, do stride: bs_update_kernel, sgd_ordered_kernel.
    // An EXACT grid needs no "rest": round 8 had the plan kernel write every iteration's block counts, copied them to pinned memory in
    // front of the window's "ready" event and QUERIED that event (no wait) at launch -- about 600 workgroups instead of 2,277.  This
    // kernel's average did not move, 18.54 against 18.51 / 18.62 us for the parent's two runs (the surplus workgroups are not on its
    // critical path), the benchmark step by 0.7 us with repeats 1.0 us apart: removed by the round's rule, profiles/r08_phase1_ab.txt.)
    gram_block(a, it, g, bs_smem);
}

// One workgroup per hot chain: the look-ahead form for the leading chains (rows of at most kLaMaxSlots slots), the plain form for the rest.
template <int SW>
__global__ __launch_bounds__(512) void bs_solve_kernel(SgdArgs a, BsIteration it) {
    extern __shared__ float4 bs_smem[];
    if (it.gram_done && threadIdx.x == 0)  // (the side stream's gate lets the side kernel go once the chains hold their CUs)
        __hip_atomic_fetch_add(it.solve_started, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int chain = blockIdx.x;
    const BsChainDesc cd = it.chains[chain];
    if constexpr (SW <= 8) {
        if (chain_is_lookahead(it, chain, cd)) {  // workgroup uniform
            chain_lookahead<(4 * SW < kLaMaxSlots ? 4 * SW : kLaMaxSlots)>(a, it, bs_smem, cd);
            return;
        }
    }
    solve_chain<SW>(a, it, bs_smem, cd);
}

// One workgroup per block.
__global__ __launch_bounds__(64 * kUpdMaxWaves) void bs_update_kernel(SgdArgs a, BsIteration it) {
    const int g = blockIdx.x;
    __builtin_amdgcn_s_setprio(2);
    if (g == it.launch_blocks) {  // the extra workgroup of the launch (side_seq set)
        if (threadIdx.x == 0) await_iteration_end(it);
        return;
    }
    // (launch_blocks workgroups stride through the dense block table -- only phase 3 strides, phase 1 keeps the full grid of max_blocks
    // workgroups; update_block keeps nothing in LDS)
    for (int blk = g; blk < it.max_blocks; blk += it.launch_blocks) {
        if (it.blocks[blk].n_valid == 0) break;  // workgroup uniform
        update_block(a, it, blk);
    }
}

template <int SW>
void launch_solve_sw(const SgdArgs &a, const BsIteration &it, hipStream_t stream) {
    size_t lds = solve_lds_bytes(a.nslots, SW);
    if (it.la_ranks > 0) lds = std::max(lds, la_lds_bytes(a.nslots));
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(bs_solve_kernel<SW>));
    hipLaunchKernelGGL((bs_solve_kernel<SW>), dim3(it.n_hot), dim3(512), lds, stream, a, it);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        fail(CU2REC_EHIP, std::string("bs_solve_kernel launch failed: ") + hipGetErrorString(err) + " (SW " + std::to_string(SW) +
                              ", chains " + std::to_string(it.n_hot) + ", LDS " + std::to_string(lds) + " bytes)");
}

}  // namespace

// ---- the launch topology of an iteration's fork / join, per device (DeviceRuntime::topology): decided on first use, revisable -------
// kTopologyDevice: gate kernel + device-side join (cross-stream spin waits: they need kernels of the two streams RUNNING SIDE BY SIDE);
// kTopologyEvents: events both ways (works wherever HIP works; 5.4 + 2.5-3.3 us per iteration on the main stream).  What decides:
//   1. CU2REC_BS_GATE in the environment (0: events, anything else: device) -- a force, never revised;
//   2. a counter pass of rocprofv3 (--pmc exports ROCPROF_COUNTER_COLLECTION: kernels are serialised across streams): events;
//   3. otherwise a two-stream handshake PROBE on the very streams the iterations will use (probe_streams below): a wait kernel queued
//      FIRST on one stream, satisfied by a signal kernel queued behind it on the other, bounded by 10 ms -- both directions.  Streams
//      that share a hardware queue (GPU_MAX_HW_QUEUES=1), a tool that serialises dispatches, a tenant holding the CUs: the waiter times
//      out, and the process uses events for good;
//   4. a join that gives up mid-run (check_faults, device_runtime.cpp) switches the device to events for every later call, and says so in its
//      error.  A wait inside a phase-2 workgroup that gives up (la_wait*: status 2, not 1) leaves the topology as it is.
namespace {
__global__ void bs_probe_wait_kernel(const unsigned *word, unsigned *result, unsigned long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    unsigned seen = 0;
    for (;;) {
        if (ld_agent(word) != 0u) {
            seen = 1;
            break;
        }
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > ticks) break;
    }
    __hip_atomic_store(result, seen ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void bs_probe_signal_kernel(unsigned *word) {
    if (threadIdx.x == 0) __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Do kernels of `waiter` and `signaller` run side by side?  The waiter is queued FIRST: if the two streams are served one after the
// other it can only time out (10 ms), and the signal kernel runs behind it.  Every wave reaches its exit: the wait is bounded.
bool probe_streams(hipStream_t waiter, hipStream_t signaller, unsigned *scratch) {
    CU2REC_HIP(hipMemsetAsync(scratch, 0, 64 * sizeof(unsigned), waiter));
    CU2REC_HIP(hipStreamSynchronize(waiter));
    CU2REC_HIP(hipStreamSynchronize(signaller));
    hipLaunchKernelGGL(bs_probe_wait_kernel, dim3(1), dim3(64), 0, waiter, scratch, scratch + 32, 1000000ull);  // 10 ms of the 100 MHz clock
    hipLaunchKernelGGL(bs_probe_signal_kernel, dim3(1), dim3(64), 0, signaller, scratch);
    CU2REC_HIP(hipGetLastError());
    CU2REC_HIP(hipStreamSynchronize(waiter));
    CU2REC_HIP(hipStreamSynchronize(signaller));
    unsigned result = 0;
    CU2REC_HIP(hipMemcpy(&result, scratch + 32, sizeof(unsigned), hipMemcpyDeviceToHost));
    return result == 1u;
}

// the topology of the current device (the caller holds device_runtime_mutex()).  The probe runs once per device, on its first block-solve
// call, under that mutex: check_faults and other devices' first launches wait for it (two bounded waits of 10 ms and the stream
// synchronisations around them).
int topology(DeviceRuntime &r, hipStream_t stream, hipStream_t side) {
    if (r.topology >= 0) return r.topology;
    if (const char *env = std::getenv("CU2REC_BS_GATE")) {
        r.topology = std::atoi(env) != 0 ? DeviceRuntime::kTopologyDevice : DeviceRuntime::kTopologyEvents;
        r.topology_forced = true;
        r.topology_why = std::string("CU2REC_BS_GATE=") + env;
        return r.topology;
    }
    if (const char *pmc = std::getenv("ROCPROF_COUNTER_COLLECTION"))
        if (*pmc && std::string(pmc) != "0" && std::string(pmc) != "False" && std::string(pmc) != "false") {
            r.topology = DeviceRuntime::kTopologyEvents;
            r.topology_why = "a rocprofv3 counter pass (ROCPROF_COUNTER_COLLECTION) serialises kernels across streams";
            return r.topology;
        }
    const bool forward = probe_streams(stream, side, r.probe);
    const bool backward = forward && probe_streams(side, stream, r.probe);
    if (forward && backward) {
        r.topology = DeviceRuntime::kTopologyDevice;
        r.topology_why = "two-stream handshake probe passed in both directions";
    } else {
        r.topology = DeviceRuntime::kTopologyEvents;
        r.topology_why = std::string("two-stream handshake probe: a wait kernel on the ") + (forward ? "side" : "main") +
                         " stream was not reached by the other stream's signal kernel within 10 ms (the streams do not run side by side here)";
    }
    return r.topology;
}

unsigned long long wait_ticks() {  // CU2REC_BS_WAIT_S (seconds, default 2): the bound of the device-side waits, in ticks of the 100 MHz clock
    static const unsigned long long ticks = [] {
        double sec = 2.0;
        if (const char *env = std::getenv("CU2REC_BS_WAIT_S")) sec = std::max(0.001, std::atof(env));
        return static_cast<unsigned long long>(sec * 1e8);
    }();
    return ticks;
}

#ifdef CU2REC_TEST_HOOKS  // fault-path tests only (build/test/libcu2rec_amd_hooks.so): 16 the signal is never sent, 32 the gate can never
                          // open, 512 phase 3 launched with 3 workgroups (ordered.hip reads 256 itself)
int dbg() {
    static const int bits = std::getenv("CU2REC_BS_DBG") ? std::atoi(std::getenv("CU2REC_BS_DBG")) : 0;
    return bits;
}
#else
constexpr int dbg() { return 0; }
#endif

// A gate that gives up just ENDS (the side kernel then starts a little early: a matter of timing, no data hangs on it): it must not
// set the status word -- that would declare the model state undefined for a delay that harms nothing.
__global__ void bs_gate_kernel(const unsigned long long *count, unsigned long long target, const unsigned long long *started,
                               unsigned long long started_target, unsigned long long wait_ticks) {
    // lanes 0-31: one shard of phase 1's count each; lane 32: phase 2's workgroups that hold their CU
    const int lane = threadIdx.x;
    const unsigned long long t0 = wall_clock64();
    unsigned polls = 0;
    for (;;) {
        unsigned long long v = lane < 32 ? ld_agent(count + 16 * lane) : 0ull;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);  // (lanes 32-63 sum zeros)
        const unsigned long long sum = __shfl(v, 0);
        const unsigned long long st = ld_agent(started);
        if (sum >= target && st >= started_target) break;
        __builtin_amdgcn_s_sleep(16);
        if ((++polls & 63u) == 0 && wall_clock64() - t0 > wait_ticks) break;
    }
}

// one thread that stores `value` to `word`: queued behind a kernel, it announces that kernel's completion
__global__ void bs_signal_kernel(unsigned long long *word, unsigned long long value) {
    if (threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Phase 1.  `stop`: an event completed by the kernel's own completion signal (hipExtLaunchKernelGGL) -- a hipEventRecord behind the
// launch is a marker packet of its own and held the NEXT launch of the stream back by 6-7 us (kernel traces, round 3)
void launch_gram(const SgdArgs &a, const BsIteration &it, hipStream_t stream, hipEvent_t stop) {
    const size_t gram_lds = gram_lds_bytes(a.nslots, it.la_ranks > 0);
    ensure_max_dynamic_lds(reinterpret_cast<const void *>(bs_gram_kernel));
    const int grid = it.max_blocks + (it.la_ranks > 0 ? it.la_grid : 0);
    if (stop) hipExtLaunchKernelGGL(bs_gram_kernel, dim3(grid), dim3(256), static_cast<uint32_t>(gram_lds), stream, nullptr, stop, 0, a, it);
    else hipLaunchKernelGGL(bs_gram_kernel, dim3(grid), dim3(256), gram_lds, stream, a, it);
    CU2REC_HIP(hipGetLastError());
}

// Phase 2: one workgroup per hot chain
void launch_solve(const SgdArgs &a, const BsIteration &it, hipStream_t stream) {
    const int sw = (a.nslots + 3) / 4;
    if (sw <= 1) launch_solve_sw<1>(a, it, stream);
    else if (sw <= 2) launch_solve_sw<2>(a, it, stream);
    else if (sw <= 4) launch_solve_sw<4>(a, it, stream);
    else if (sw <= 7) launch_solve_sw<7>(a, it, stream);
    else if (sw <= 8) launch_solve_sw<8>(a, it, stream);
    else if (sw <= 12) launch_solve_sw<12>(a, it, stream);
    else if (sw <= 16) launch_solve_sw<16>(a, it, stream);
    else fail(CU2REC_EUNSUPPORTED, "block-solve mode is compiled for n_factors <= 252");
}

// Phase 3: launch_blocks workgroups, and one more that waits for the side kernel when side_seq is set
void launch_update(const SgdArgs &a, const BsIteration &it, hipStream_t stream) {
    const int nwaves = (4 * a.nslots + 63) / 64;
    hipLaunchKernelGGL(bs_update_kernel, dim3(it.launch_blocks + (it.side_seq ? 1 : 0)), dim3(64 * nwaves), 0, stream, a, it);
    CU2REC_HIP(hipGetLastError());
}

std::atomic<int> g_lookahead{-1};  // -1: not yet initialised from the environment
// explicit threshold (> 0), or <= 0: automatic (240 per 131,072 rating users, scaled with the set); -2 = not yet initialised
// from the environment
std::atomic<float> g_min_rate{-2.f};
constexpr float kDefaultRate = 240.f;

float min_rate_state() {
    float cur = g_min_rate.load();
    if (cur == -2.f) {  // first use: CU2REC_BLOCKSOLVE_RATE overrides the automatic threshold
        float init = -1.f;
        if (const char *env = std::getenv("CU2REC_BLOCKSOLVE_RATE")) init = std::max(0.01f, static_cast<float>(std::atof(env)));
        g_min_rate.compare_exchange_strong(cur, init);
        cur = g_min_rate.load();
    }
    return cur;
}
}  // namespace

int blocksolve_lookahead_blocks(int blocks) {
    int prev = g_lookahead.load();
    if (prev < 0) {
        const char *env = std::getenv("CU2REC_BLOCKSOLVE_LOOKAHEAD");
        const int init = env ? std::max(0, std::atoi(env)) : 24;  // the top chains only: DESIGN.md section 4, "The look-ahead form"
        g_lookahead.compare_exchange_strong(prev, init);
        prev = g_lookahead.load();
    }
    if (blocks >= 0) g_lookahead.store(blocks);
    return prev;
}

// rate > 0: explicit threshold; rate < 0: back to automatic; rate == 0: query.  Returns what was in force before the call:
// the explicit value, or -1 for automatic -- so that f(f(x)) restores either state.
float blocksolve_min_rate(float rate) {
    const float prev = min_rate_state();
    if (rate > 0.f) g_min_rate.store(rate);
    else if (rate < 0.f) g_min_rate.store(-1.f);
    return prev > 0.f ? prev : -1.f;
}

int blocksolve_hot_items(const std::vector<double> &rate, int n_active, int rank_limit) {
    // the threshold: what the caller set, else scaled with the set -- down (a long chain costs the same whatever the set,
    // the launch overhead it has to beat does not shrink with it; 1/1 .. 1/8 of the ML-20M shape,
    // profiles/r02_shard_size_probe_blocksolve.log) and up (Netflix shape, 480,189 users: 290 us per iteration at 800
    // against 353 at 240 -- the chains of several hundred hot items do not fit the CUs at once)
    const float state = min_rate_state();
    float min_rate = state > 0.f ? state : kDefaultRate;
    const int n_cols = static_cast<int>(rate.size());
    if (state <= 0.f) {
        min_rate = std::max(30.f, min_rate * static_cast<float>(n_active) / 131072.f);
        // a small set (one GPU's shard of a strong-scaling run): with the hottest item between 150 and 350 expected updates per
        // iteration a threshold of 60 still pays a little (an eighth of the ML-20M shape, hottest item 247: 32.5 us per iteration
        // against 35.3 walking everything; thresholds 40 / 60 / 90 / 130 / 180: 32.6 / 32.5 / 33.7 / 37.5 / 41.4, round 5); below
        // that no chain is long enough to pay for three launches per iteration and the mode IS the ordered walk (ML-1M shape)
        // Only for SMALL sets (at most a quarter of 131,072 users: where the rule was measured).  A large set with flat popularity --
        // many users, hottest item under 350 -- keeps the scaled threshold: there "every item above 60" would be hundreds of
        // 512-thread solve workgroups the side stream's gate has to see started (the regime that did not fit the CUs on the
        // Netflix shape), and nothing was measured there.
        if (n_cols > 0 && n_active <= 131072 / 4 && rate[0] < 350.0) min_rate = rate[0] >= 150.0 ? 60.f : std::numeric_limits<float>::infinity();
    }
    int n = 0;
    while (n < n_cols && rate[n] >= min_rate) ++n;
    return std::min(n, rank_limit);
}

BlockSolve::BlockSolve(int n_hot_, const std::vector<double> &rate, double hot_rate, int n_active_, int max_batch_, const int *item_of_rank_)
    : n_hot(n_hot_), n_active(n_active_), max_batch(max_batch_), item_of_rank(item_of_rank_) {
    max_blocks = n_active / kBsLinks + n_hot + 1;
    // Blocks of 64 links an iteration's hot chains are expected to fill, as a bound that holds in all but astronomically rare iterations
    // (the hot links' count: mean hot_rate, variance at most the mean; one partial block per chain): what phase 3 is launched with.  Its
    // workgroups stride through the dense block table, so an iteration beyond the bound is still done completely.
    const double bound = (hot_rate + 8.0 * std::sqrt(hot_rate) + 64.0) / kBsLinks + n_hot + 1;
    launch_blocks = std::max(1, bound >= static_cast<double>(max_blocks) ? max_blocks : static_cast<int>(bound));
    if (dbg() & 512) launch_blocks = std::min(3, max_blocks);  // (a launch far too small: every workgroup strides over many blocks)
    // the look-ahead form of phase 2: the leading ranks whose chains are expected to be at least blocksolve_lookahead_blocks() blocks
    // long -- the chains whose length is the iteration's critical path.  Their blocks are the first of every iteration's block table;
    // la_cap bounds them with room to spare (a chain beyond it: the plain form).
    const int la_min = blocksolve_lookahead_blocks(-1);
    double la_blocks = 0.0;
    while (la_min > 0 && la_ranks < n_hot && rate[la_ranks] >= static_cast<double>(la_min) * kBsLinks) {
        la_blocks += std::ceil(rate[la_ranks] / kBsLinks) + 1.0;
        ++la_ranks;
    }
    if (la_ranks > 0) la_cap = std::min(max_blocks, static_cast<int>(la_blocks * 1.25) + 4 * la_ranks + 8);
    for (int slot = 0; slot < 2; ++slot) {
        chains[slot].allocate(static_cast<size_t>(max_batch) * n_hot);
        blocks[slot].allocate(static_cast<size_t>(max_batch) * max_blocks);
    }
    tables.allocate(kBsTableFloats);
    Mbuf.allocate(static_cast<size_t>(max_blocks) * kBsRecFloats);
    ebuf.allocate(static_cast<size_t>(max_blocks) * kBsLinks);
    solve_started.allocate(16);
    solve_started.zero();
    gram_done.allocate(32 * 16);
    gram_done.zero();
    side_seq.allocate(16);
    side_seq.zero();
    if (la_cap > 0) Nbuf.allocate(static_cast<size_t>(la_cap) * kBsCrossFloats);
}

BlockSolve::~BlockSolve() {  // (the schedule has waited for its last call's end)
    if (upd) (void)hipStreamDestroy(upd);
    for (hipEvent_t e : {ev_call, ev_upd, ev_gram})
        if (e) (void)hipEventDestroy(e);
}

void BlockSolve::plan(int slot, const int *chain_ranges, int range_stride, int nb, hipStream_t sched) {
    hipLaunchKernelGGL(bs_plan_kernel, dim3(nb), dim3(256), 0, sched, chain_ranges, range_stride, n_hot, max_blocks, item_of_rank,
                       chains[slot].ptr, blocks[slot].ptr);
}

void BlockSolve::begin(const SgdArgs &a, hipStream_t stream) {
    if (a.nslots < 1 || a.nslots > kBsMaxSlots) fail(CU2REC_EUNSUPPORTED, "block-solve mode is compiled for n_factors <= 252");
    const bool same = tables_valid && tables_for.lr == a.h.lr && tables_for.q_reg == a.h.q_reg && tables_for.ib_reg == a.h.ib_reg;
    if (!same) {  // stream ordered: kernels already queued keep the old tables
        hipLaunchKernelGGL(bs_tables_kernel, dim3(1), dim3(192), 0, stream, a.h, tables.ptr);
        tables_for = a.h;
        tables_valid = true;
    }
    if (qstart_ld != a.ldq) {
        CU2REC_HIP(hipStreamSynchronize(stream));
        qstart.allocate(static_cast<size_t>(max_blocks) * a.ldq);
        qstart_ld = a.ldq;
    }
    if (!upd) {
        // default priority: a high-priority queue whose workgroups cannot all be placed (more hot chains than CUs) held back
        // the queues below it (a 300-chain test set ran into the waits' timeout)
        CU2REC_HIP(hipStreamCreateWithFlags(&upd, hipStreamNonBlocking));
        for (hipEvent_t *e : {&ev_call, &ev_upd, &ev_gram}) CU2REC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    unsigned *status = nullptr;
    {
        std::lock_guard<std::mutex> lock(device_runtime_mutex());
        DeviceRuntime &r = device_runtime();
        device_join = topology(r, stream, upd) == DeviceRuntime::kTopologyDevice;
        status = r.status + DeviceRuntime::kBlocksolveWord;
        host_status = r.host_status + 1;
    }
    // the side stream starts behind everything the caller has queued so far
    CU2REC_HIP(hipEventRecord(ev_call, stream));
    CU2REC_HIP(hipStreamWaitEvent(upd, ev_call, 0));
    const bool la_on = la_ranks > 0 && la_supported(a.nslots);  // (rows the rings have LDS for)
    it = BsIteration{};
    it.n_active = n_active;
    it.n_hot = n_hot;
    it.item_of_rank = item_of_rank;
    it.tables = tables.ptr;
    it.log2a = static_cast<float>(std::log2(1.0 - static_cast<double>(a.h.lr) * static_cast<double>(a.h.q_reg)));
    it.log2c = static_cast<float>(std::log2(1.0 - static_cast<double>(a.h.lr) * static_cast<double>(a.h.ib_reg)));
    it.Mbuf = Mbuf.ptr;
    it.ebuf = ebuf.ptr;
    it.qstart = qstart.ptr;
    it.max_blocks = max_blocks;
    it.launch_blocks = launch_blocks;
    it.la_ranks = la_on ? la_ranks : 0;
    it.la_cap = la_cap;
    it.la_grid = la_on ? la_cap : 0;
    it.Nbuf = Nbuf.ptr;
    it.status = status;
    it.solve_started = solve_started.ptr;
    it.wait_ticks = wait_ticks();
    if (device_join) {
        it.gram_done = gram_done.ptr;
        it.side_seq = side_seq.ptr;
    }
    upd_pending = false;
}

// One iteration = four launches: `stream`: phase 1 (bs_gram_kernel: every block's inverse factor) -> phase 2 (bs_solve_kernel: one
// workgroup per chain) -> phase 3 (bs_update_kernel: the user side); side stream `upd`: the other items' chains (two-wave form / walk),
// forked behind phase 1 -- beside it their thousands of workgroups take the CUs from phase 1's (measured: 71 instead of 19 us) -- and
// joined in front of the next phase 1, which reads rows they write.  Host order gram, solve, [gate], side, [signal], update: every
// launch behind what it waits for (streams sharing a hardware queue serialise, they cannot wait for each other).
//  * device_join (kTopologyDevice), no event on the main stream: phase 1's workgroups count themselves through, phase 2's count
//    themselves in, ONE wavefront queued in front of the side kernel (bs_gate_kernel) ends when both counts have reached what the host
//    has launched so far; a signal kernel behind the side kernel stores the iteration's number and one extra workgroup of phase 3's
//    launch waits for it.  (The host's counts move only behind a launch that succeeded: a launch that throws leaves gate and counters
//    in step for the calls that follow.)
//  * events (kTopologyEvents): fork on phase 1's completion signal, join by an event wait in front of the next phase 1 (5.4 + 2.5-3.3 us
//    per iteration on the main stream: DESIGN.md section 4).
void BlockSolve::iteration(const SgdArgs &a, int slot, int b, const uint32_t *keys, const uint64_t *vals, bool last, hipStream_t stream,
                           const SideChains &side) {
    it.keys = keys;
    it.vals = vals;
    it.chains = chains[slot].ptr + static_cast<size_t>(b) * n_hot;
    it.blocks = blocks[slot].ptr + static_cast<size_t>(b) * max_blocks;
    it.side_target = device_join ? side_seq_host + 1 : 0;
    if (upd_pending) CU2REC_HIP(hipStreamWaitEvent(stream, ev_upd, 0));  // (events) join: rows the next phase 1 reads
    launch_gram(a, it, stream, device_join ? nullptr : ev_gram);
    if (device_join) gram_done_target += static_cast<unsigned long long>(max_blocks + it.la_grid);
    else CU2REC_HIP(hipStreamWaitEvent(upd, ev_gram, 0));
    launch_solve(a, it, stream);
    if (device_join) {
        started_total += static_cast<unsigned long long>(n_hot);
        hipLaunchKernelGGL(bs_gate_kernel, dim3(1), dim3(64), 0, upd, gram_done.ptr, gram_done_target + ((dbg() & 32) ? (1ull << 40) : 0ull),
                           solve_started.ptr, started_total, it.wait_ticks);
        CU2REC_HIP(hipGetLastError());
    }
    // (device_join: only the batch's last side kernel carries the event the main stream waits for at the END of the batch -- an event on
    // a kernel's completion signal holds the next packet of its queue back, here the signal kernel: 5.4 us)
    side(upd, !device_join || last ? ev_upd : nullptr);
    if (device_join) {
        ++side_seq_host;
        if (!(dbg() & 16)) {
            hipLaunchKernelGGL(bs_signal_kernel, dim3(1), dim3(64), 0, upd, side_seq.ptr, side_seq_host);
            CU2REC_HIP(hipGetLastError());
        }
    }
    launch_update(a, it, stream);
    upd_pending = !device_join;
}

void BlockSolve::join(hipStream_t stream) {
    CU2REC_HIP(hipStreamWaitEvent(stream, ev_upd, 0));
    upd_pending = false;
}

void BlockSolve::end(hipStream_t stream) {  // (every batch ended with `stream` behind the side stream)
    CU2REC_HIP(hipMemcpyAsync(host_status, it.status, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
}

}  // namespace cu2rec
