// Softmax matrix factorization for implicit feedback (include/cu2rec_amd.h: cu2rec_model_softmax; the multinomial likelihood of Liang
// et al. 2018 on a linear model), full batch: a user's items form one distribution pi_ui = softmax_i(s_ui).  One half-step is the
// gradient over EVERY (own row, partner row) pair, with the users' log-sum-exp taken first, then the logistic trainer's AdaGrad step
// (lmf.hpp: lmf_step, on its accumulators and its workspace) -- softmax.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "hip_check.hpp"
#include "lmf.hpp"

namespace cu2rec {

// Kept with the cu2rec_model beside LmfState: what every softmax call forms first, of the users inside the CSR it was given.
struct SoftmaxState {
    DeviceBuffer<float> lse;  // [U]: log sum_(i < I) exp(s_ui)
    DeviceBuffer<float> W;    // [U]: the row's stored values, added in entry order
};

// The problems below are LmfProblems (alpha is not read): `users` is the user side's view -- own rows the users on the CSR itself,
// partners the items -- and `p` the view of the side that moves (the item side's on the item-major view).

// sm.W and sm.lse of every user of `users`
void softmax_lse(SoftmaxState &sm, const LmfProblem &users, hipStream_t stream);
// st.grad[row][0 .. f] = the gradient of every own row of p in lmf_step's layout, from sm of the same model and CSR; the users'
// column f is a zero.  mass: st.grad[row][f] = sum_i pi_ui instead, the dense pass's own column f (the users' side only)
void softmax_gradient(LmfState &st, const SoftmaxState &sm, const LmfProblem &p, bool users, hipStream_t stream, bool mass = false);
// out[4] = {sum over entries of w (s - lse_u), sum |p|^2, sum |q|^2, sum ib^2}, in double (synchronises)
void softmax_objective_sums(LmfState &st, const SoftmaxState &sm, const LmfProblem &users, int nnz, double (&out)[4], hipStream_t stream);

}  // namespace cu2rec
