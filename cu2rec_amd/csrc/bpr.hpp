// Bayesian Personalized Ranking for implicit feedback (include/cu2rec_amd.h: cu2rec_model_bpr; Rendle et al. 2009) in a deterministic,
// full-batch form: a sweep draws one negative item per stored entry from the counter-based sampler (sampler.hpp), a half-step is the
// gradient of sum ln sigma(x_e) over the sweep's triples and then the logistic trainer's AdaGrad step (lmf.hip: lmf_step).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_check.hpp"

namespace cu2rec {

constexpr int kBprAttempts = 8;          // draws per entry and sweep before the entry goes without a triple
constexpr int kBprMaxSweep = 1 << 29;    // sweep * kBprAttempts + attempt fills the high word of the sampler's iteration

struct DeviceCsr;

// Cached on a cu2rec_csr, per (seed, sweep): the negatives, and for the item half-step their regrouping by item and the entries'
// coefficients.  The rows' ascending items (the membership test's haystack), the row of every entry and the item-major view are the
// CSR's own views (csr_views.hpp).
struct BprCache {
    DeviceBuffer<int> iota;           // [nnz]: the entries in CSR order, the regrouping sort's values
    DeviceBuffer<int> neg;            // [nnz]: j_e, or -1 where all attempts were stored items
    DeviceBuffer<unsigned> neg_key;   // [nnz]: j_e, or cols for -1 (sorts past the end)
    DeviceBuffer<unsigned> key_sorted;
    DeviceBuffer<int> neg_e;          // [nnz]: the entries e by ascending (j_e, e)
    DeviceBuffer<int> n_indptr;       // [cols + 1]: item i's negatives are neg_e[n_indptr[i] .. n_indptr[i + 1])
    DeviceBuffer<float> coef;         // [nnz]: sigma(-x_e) at the current model
    DeviceBuffer<unsigned char> sort_temp;
    DeviceBuffer<double> partials;
    bool allocated = false, have_neg = false, grouped = false;
    uint64_t seed = 0;
    int sweep = -1;
};

// The model and the CSR as the kernels read them.  t_*: the CSR's item-major view (the item half-step only).
struct BprProblem {
    const int *indptr, *indices;
    int rows, cols, nnz;
    const int *t_indptr, *t_indices, *t_pos;
    const float *P;
    int ldp;
    const float *Q;
    int ldq;
    const float *item_bias;
    int n_factors;
    float P_reg, Q_reg, item_bias_reg;
};

// train.bpr.neg (and neg_key) for (seed, sweep); a repeated call for the same pair is free
void bpr_negatives(const DeviceCsr &train, const BprProblem &p, uint64_t seed, int sweep, hipStream_t stream);
// grad[u][0 .. f] of every user u < p.rows, row stride ldg; column f, the bias', is a zero.  Needs bpr_negatives
void bpr_user_gradient(const DeviceCsr &train, const BprProblem &p, float *grad, int ldg, hipStream_t stream);
// grad[i][0 .. f] of every item i < p.cols (column f: the bias'): regroups the negatives by item once per (seed, sweep), writes
// the coefficients at the current model, then sums.  Needs bpr_negatives
void bpr_item_gradient(const DeviceCsr &train, const BprProblem &p, float *grad, int ldg, hipStream_t stream);
// out[6] = {sum over triples of ln sigma(x_e), sum |p_u|^2, sum |q_i|^2, sum ib_i^2, triples, triples with x_e > 0}, in double
// (synchronises).  Needs bpr_negatives
void bpr_objective(const DeviceCsr &train, const BprProblem &p, double (&out)[6], hipStream_t stream);

}  // namespace cu2rec
