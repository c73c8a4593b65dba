// Owned device objects and the C++ form of the raw hot-path entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include <memory>
#include <optional>
#include <utility>

#include "als.hpp"
#include "bpr.hpp"
#include "csr_views.hpp"
#include "hip_check.hpp"
#include "knn.hpp"
#include "lmf.hpp"
#include "ordered.hpp"
#include "softmax.hpp"

struct cu2rec_csr;
struct cu2rec_model;

namespace cu2rec {

// The ratings and the model as the hot path passes them on: plain views, nothing owned.  The extern "C" wrappers (device_raw.cpp) pack
// their loose parameters into these; an owned object hands out its own (DeviceCsr::ref, DeviceModel::ref).
struct RatingsRef {
    const int *indptr, *indices;
    const float *data;
    int n_rows;
};

struct FactorsRef {
    float *P;
    int ldp;
    float *Q;
    int ldq;
    float *user_bias, *item_bias;
    float global_bias;
    int n_factors;
};

// What a persistent or concurrent launch could not finish is reported at the next entry point, once: the words are cleared so that
// the process can go on.  (device_runtime.cpp, beside device_runtime() of hip_check.hpp)
void check_faults();

// fills the launch argument block after validating shapes / alignment (shared by all SGD modes)
SgdArgs make_sgd_args(const RatingsRef &r, const FactorsRef &m, int n_cols, const cu2rec_hyper &hyper, uint64_t seed,
                      int update_items, int user_offset);

void sgd_update(const RatingsRef &r, const FactorsRef &m, int n_cols, const cu2rec_hyper &hyper, uint64_t seed,
                uint64_t iter0, int n_iters, int mode, int update_items, int user_offset, hipStream_t stream,
                const void *sample_pairs = nullptr);

// CU2REC_SGD_PINGPONG on raw pointers (include/cu2rec_amd.h: cu2rec_sgd_update_pingpong); returns true if the item
// side's current values ended up in other.Q_target / other.item_bias_target (odd number of swaps)
bool sgd_update_pingpong(const RatingsRef &r, const FactorsRef &m, int n_cols, const PingPongArgs &other,
                         const cu2rec_hyper &hyper, uint64_t seed, uint64_t iter0, int n_iters, int update_items,
                         int user_offset, bool swap_last, hipStream_t stream);

// [nnz] x {item, rating} side by side for SgdArgs::pairs (8 bytes per rating, device memory)
void sample_pairs_build(const int *indices, const float *data, int nnz, void *pairs, hipStream_t stream);

void sgd_update_ordered(OrderedSchedule &schedule, const RatingsRef &r, const FactorsRef &m, int n_cols,
                        const cu2rec_hyper &hyper, uint64_t seed, uint64_t iter0, int n_iters, int update_items,
                        int user_offset, hipStream_t stream, bool blocksolve = false);

// reads the model only
void loss(const RatingsRef &r, int nnz, const FactorsRef &m, float *errors_out, void *workspace, double *sum_abs,
          double *sum_sq, float *mae, float *rmse, hipStream_t stream);

void error_metrics(const float *errors, int n, void *workspace, float *mae, float *rmse, hipStream_t stream);

// the step count of every conjugate-gradient entry point (cu2rec_model_als_cg, cu2rec_train_implicit_cg, ...), under the entry's name
inline void require_cg_steps(const char *fn, int cg_steps) {
    Need{fn}(cg_steps >= 1 && cg_steps <= CU2REC_ALS_CG_MAX_STEPS, CU2REC_EINVAL, ": cg_steps must be in [1, CU2REC_ALS_CG_MAX_STEPS]");
}

// Device CSR in the reference's layout (matrix.h:11-19): int32 indptr / indices, float32 data.
struct DeviceCsr {
    DeviceCsr(int rows, int cols, int nnz, const int *h_indptr, const int *h_indices, const float *h_data);
    DeviceBuffer<int> indptr, indices;
    DeviceBuffer<float> data;
    RatingsRef ref() const { return {indptr.ptr, indices.ptr, data.ptr, rows}; }
    int rows, cols, nnz;
    int max_item;
    int users_with_ratings;
    mutable std::unique_ptr<OrderedSchedule> schedule;  // created on first CU2REC_SGD_ORDERED use
    mutable DeviceBuffer<uint2> pairs;                   // sample array, created on first Hogwild use (SgdArgs::pairs)
    mutable CsrViews views;                              // item-major, row-sorted and row-of-entry views, each built on first request
    mutable AlsCache als;                                // the ALS row plans and workspaces
    mutable BprCache bpr;                                // the current sweep's negatives and their regrouping
};

// The rows one ALS half-step solves, as it reads them: the CSR itself for the users, its item-major view for the items, planned the
// first time the side is asked for (device_trainers.cpp).
AlsSide &als_side(const DeviceCsr &train, bool users, hipStream_t stream);

// P, Q, biases on the device with padded rows (see include/cu2rec_amd.h "Device data layout").
struct DeviceModel {
    DeviceModel(int rows, int cols, int n_factors, const float *P, const float *Q, const float *user_bias,
                const float *item_bias, float global_bias);
    void download(float *P, float *Q, float *user_bias, float *item_bias) const;
    // defer_last_swap (CU2REC_SGD_PINGPONG only): leave out the last iteration's swap; finish_swap() does it later
    // user_offset: global id of row 0 when the model holds one shard of a user-sharded set (enters the sampler only)
    void sgd(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, uint64_t iter0, int n_iters, int mode,
             int update_items, hipStream_t stream, bool defer_last_swap = false, int user_offset = 0);
    void finish_swap();
    // one exact ALS half-step (side: CU2REC_SIDE_USERS / CU2REC_SIDE_ITEMS); returns the rows a failed pivot left unchanged
    // cg_steps > 0: rows of at most CU2REC_ALS_CHUNK ratings take that many conjugate-gradient steps from their current factors
    // and bias (cu2rec_model_als_cg)
    int als(const DeviceCsr &train, const cu2rec_hyper &h, int side, hipStream_t stream, int cg_steps = 0);
    // one implicit-feedback half-step (confidence weight alpha * r per entry, every user x item pair counted); same return
    // cg_steps > 0: rows of at most CU2REC_ALS_CHUNK entries take that many conjugate-gradient steps from their current factors
    // (cu2rec_model_als_implicit_cg)
    int ials(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, hipStream_t stream, int cg_steps = 0);
    // the implicit objective at the current model (synchronises)
    double implicit_objective(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, hipStream_t stream);
    // one logistic-MF half-step (lmf.hpp: gradient over every pair, then AdaGrad); returns the rows left unchanged
    int lmf(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, hipStream_t stream);
    // the same gradient to the host ([n][n_factors] and [n], n = the side's rows inside the CSR); the model and accumulators untouched
    void lmf_gradient(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, float *grad_out, float *bias_grad_out,
                      hipStream_t stream);
    // the logistic log-posterior at the current model (synchronises)
    double lmf_objective(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, hipStream_t stream);
    void lmf_download_state(float *aP, float *aQ, float *a_ub, float *a_ib);  // zeros before the first logistic call
    void lmf_reset();
    // the argument checks of the logistic and the BPR calls, before the device or the model is touched; fn names the caller.
    // alpha (the logistic calls'), side and sweep (the BPR calls') are checked where given
    void logistic_check(const char *fn, const DeviceCsr &train, const cu2rec_hyper &h, std::optional<float> alpha, std::optional<int> side,
                        std::optional<long long> sweep) const;
    // one BPR half-step (bpr.hpp: the gradient over sweep `sweep`'s triples, then the logistic trainer's AdaGrad step on ITS
    // accumulators); returns the rows left unchanged
    int bpr(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, int side, hipStream_t stream);
    // the same gradient to the host, as lmf_gradient; the model and the accumulators untouched
    void bpr_gradient(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, int side, float *grad_out,
                      float *bias_grad_out, hipStream_t stream);
    // the BPR objective at the current model over sweep `sweep`'s triples, their number and the number with x_e > 0 (synchronises)
    double bpr_objective(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, long long *n_triples,
                         long long *n_ordered, hipStream_t stream);
    // one softmax-MF half-step (softmax.hpp: the users' log-sum-exp, the gradient over every pair, then the logistic trainer's AdaGrad
    // step on ITS accumulators); returns the rows left unchanged
    int softmax(const DeviceCsr &train, const cu2rec_hyper &h, int side, hipStream_t stream);
    // the same gradient to the host, as lmf_gradient; the model and the accumulators untouched
    void softmax_gradient(const DeviceCsr &train, const cu2rec_hyper &h, int side, float *grad_out, float *bias_grad_out, hipStream_t stream);
    // the softmax objective at the current model (synchronises)
    double softmax_objective(const DeviceCsr &train, const cu2rec_hyper &h, hipStream_t stream);
    // every user's log-sum-exp and sum_i pi_ui (the dense pass's column f) to the host, U floats each; either may be null
    void softmax_lse(const DeviceCsr &train, float *lse_out, float *mass_out, hipStream_t stream);
    // the argument checks of the softmax calls, before the device or the model is touched; fn names the caller
    void softmax_check(const char *fn, const DeviceCsr &train, const cu2rec_hyper &h, std::optional<int> side) const;
    // what the logistic and the BPR calls end in: lmf_st.grad's first n_own rows to the host (synchronises); the AdaGrad step from
    // lmf_st.grad on the accumulators of p's side, which returns the rows left unchanged
    void download_gradient(int n_own, float *grad_out, float *bias_grad_out, hipStream_t stream);
    int adagrad_half_step(const LmfProblem &p, bool users, hipStream_t stream);
    void loss(const DeviceCsr &ratings, double *sum_abs, double *sum_sq, float *mae, float *rmse,
              hipStream_t stream) const;
    FactorsRef ref() const { return {P.ptr, ld, Q.ptr, ldq, user_bias.ptr, item_bias.ptr, global_bias, n_factors}; }
    DeviceBuffer<float> P, Q, user_bias, item_bias;
    DeviceBuffer<float> Q_other, item_bias_other;  // CU2REC_SGD_PINGPONG: the second buffer pair, created on first use
    DeviceBuffer<unsigned long long> claim;
    bool other_in_sync = false;   // Q_other / item_bias_other were last written by the ping-pong mode itself
    bool swap_pending = false;
    mutable DeviceBuffer<double> workspace;
    LmfState lmf_st;  // AdaGrad accumulators and workspace of the logistic trainer, created by its first call
    SoftmaxState softmax_st;  // the users' log-sum-exp and row weights of the last softmax call
    int rows, cols, n_factors;
    int ld;   // row stride of P in floats: n_factors rounded up to 4 (16-byte aligned rows)
    int ldq;  // row stride of Q: rounded up to 32 floats, so that every item row is a whole number of 128-byte lines --
              // item rows are the ones several XCDs read AND write; rows that share a line cost extra coherence misses
              // and partial-line write-backs (resident launches: 18.0 -> 17.6 us per iteration at f = 100)
    float global_bias;
};

// padded device rows (stride ld) -> dense host rows (stride f)
void download_padded(const DeviceBuffer<float> &src, float *host, int rows, int f, int ld);

DeviceCsr &unwrap(cu2rec_csr *m);
const DeviceCsr &unwrap(const cu2rec_csr *m);
DeviceModel &unwrap(cu2rec_model *m);
const DeviceModel &unwrap(const cu2rec_model *m);

}  // namespace cu2rec

// the C ABI's opaque handles
struct cu2rec_schedule {
    cu2rec::OrderedSchedule impl;
    template <class... A>
    explicit cu2rec_schedule(A &&...a) : impl(std::forward<A>(a)...) {}
};
struct cu2rec_csr {
    cu2rec::DeviceCsr impl;
    template <class... A>
    explicit cu2rec_csr(A &&...a) : impl(std::forward<A>(a)...) {}
};
struct cu2rec_model {
    cu2rec::DeviceModel impl;
    template <class... A>
    explicit cu2rec_model(A &&...a) : impl(std::forward<A>(a)...) {}
};
