// Logistic matrix factorization for implicit feedback (include/cu2rec_amd.h: cu2rec_model_lmf; Johnson 2014), full batch: one
// half-step is the gradient of the log-posterior over EVERY (own row, partner row) pair, then an element-wise AdaGrad step (lmf.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "hip_check.hpp"

namespace cu2rec {

// One half-step's view: the own side X (the rows that move, [0, n_own)) against the frozen partner side Y ([0, n_partner)), the
// own side's CSR (the user-major CSR itself, or the item-major view of als.hip).  The score of a pair is
//   ((global_bias + xb[own]) + yb[partner]) + x . y
struct LmfProblem {
    const int *indptr, *indices;
    const float *data;
    float *X;
    int ldx;
    float *xb;
    int n_own;
    const float *Y;
    int ldy;
    const float *yb;
    int n_partner;
    int n_factors;
    float global_bias, alpha, reg, reg_bias, lr;
};

// Kept with the cu2rec_model: the AdaGrad accumulators (P's and Q's strides, one float per factor and per bias; allocated zeroed
// by the first logistic call) and the half-step's workspace.
struct LmfState {
    DeviceBuffer<float> aP, aQ, a_ub, a_ib;
    DeviceBuffer<float> grad;  // [n_own][32 T]: the dense pass's sums, then the gradient; column f is the bias'
    DeviceBuffer<double> partials;
    DeviceBuffer<int> unchanged;
};

inline int lmf_tiles(int n_factors) { return (n_factors + 1 + 31) / 32; }  // 32-column blocks of [factors | 1]

// grad[row][0 .. f] = the gradient of every own row (column f: the bias'), row stride 32 lmf_tiles(f)
void lmf_gradient(LmfState &st, const LmfProblem &p, hipStream_t stream);
// the AdaGrad step from st.grad on the accumulators a / ab (the own side's); returns the rows left unchanged (synchronises)
int lmf_step(LmfState &st, const LmfProblem &p, float *a, float *ab, hipStream_t stream);
// sum over every pair of softplus(score), the scores in float32 on the matrix cores, the sum in double (synchronises)
double lmf_dense_objective(LmfState &st, const LmfProblem &p, hipStream_t stream);
// out[5] = {sum over entries of w (s - softplus(s)), sum |x|^2, sum xb^2, sum |y|^2, sum yb^2}, in double; p is the user side's
// view (synchronises)
void lmf_sparse_objective(LmfState &st, const LmfProblem &p, int nnz, double (&out)[5], hipStream_t stream);

}  // namespace cu2rec
