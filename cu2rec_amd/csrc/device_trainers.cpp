// The full-batch trainers' host drivers on the owned device objects: the ALS half-steps (explicit, implicit, their conjugate-gradient
// forms), logistic matrix factorization and BPR, their objectives, and the cu2rec_model_* wrappers of each.
#include <algorithm>
#include <cmath>

#include "device.hpp"
#include "hip_check.hpp"

namespace cu2rec {

namespace {
// One side's rows as every full-batch trainer reads them: the CSR itself for the users, its item-major view for the items.
RatingsRef side_rows(const DeviceCsr &train, bool users, hipStream_t stream) {
    if (users) return train.ref();
    const ItemMajorView &v = item_major_view(train, stream);
    return {v.indptr.ptr, v.indices.ptr, v.data.ptr, train.cols};
}
}  // namespace

// device.hpp: the rows one ALS half-step solves, as it reads them
AlsSide &als_side(const DeviceCsr &train, bool users, hipStream_t stream) {
    AlsSide &side = users ? train.als.users : train.als.items;
    if (!side.planned) {
        const RatingsRef r = side_rows(train, users, stream);
        side.indptr = r.indptr;
        side.indices = r.indices;
        side.data = r.data;
        side.rows = r.n_rows;
        als_plan_side(side, stream);
    }
    return side;
}

namespace {
// One side of the model as a half-step sees it: the rows that move, and the frozen partner side.
struct SideView {
    float *own, *own_bias, *partner, *partner_bias;
    int ld_own, ld_partner;
};

SideView side_view(DeviceModel &m, bool users) {
    return users ? SideView{m.P.ptr, m.user_bias.ptr, m.Q.ptr, m.item_bias.ptr, m.ld, m.ldq}
                 : SideView{m.Q.ptr, m.item_bias.ptr, m.P.ptr, m.user_bias.ptr, m.ldq, m.ld};
}

// what every trainer's call does between its argument checks and its work
void enter(DeviceModel &m) {
    require_device();
    check_faults();
    m.finish_swap();
}

bool is_side(int side) { return side == CU2REC_SIDE_USERS || side == CU2REC_SIDE_ITEMS; }
bool finite_at_least(float v, float low) { return std::isfinite(v) && v >= low; }

// One ALS half-step, explicit or implicit (include/cu2rec_amd.h: cu2rec_model_als, cu2rec_model_als_implicit and their _cg forms).
// Argument checks first: nothing on the device or in the model is touched by a call that fails them.
int als_half_step_of(DeviceModel &m, AlsKind kind, const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side,
                     hipStream_t stream, int cg_steps) {
    const bool implicit = kind == AlsKind::Implicit;
    const Need need{implicit ? (cg_steps > 0 ? "cu2rec_model_als_implicit_cg" : "cu2rec_model_als_implicit")
                             : (cg_steps > 0 ? "cu2rec_model_als_cg" : "cu2rec_model_als")};
    need(is_side(side), CU2REC_EINVAL, ": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS");
    const bool users = side == CU2REC_SIDE_USERS;
    const float reg = users ? h.P_reg : h.Q_reg, reg_bias = implicit ? 0.f : (users ? h.user_bias_reg : h.item_bias_reg);
    need(std::isfinite(reg) && reg > 0.f, CU2REC_EINVAL, ": the factor regulariser (P_reg for users, Q_reg for items) must be finite and > 0");
    if (implicit) need(finite_at_least(alpha, 0.f), CU2REC_EINVAL, ": alpha must be finite and >= 0");
    else need(finite_at_least(reg_bias, 0.f), CU2REC_EINVAL, ": the bias regulariser must be finite and >= 0");
    need(train.rows <= m.rows && train.max_item < m.cols && (!implicit || train.cols <= m.cols), CU2REC_EINVAL,
         ": ratings exceed the model's shape");
    need(m.n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
    enter(m);
    AlsSide &rows_of_side = als_side(train, users, stream);
    const SideView v = side_view(m, users);
    AlsProblem p{v.partner, v.ld_partner, v.partner_bias, v.own, v.ld_own, v.own_bias, m.n_factors, implicit ? 0.f : m.global_bias,
                 reg, reg_bias};
    if (implicit) {
        p.alpha = alpha;
        p.x_rows = users ? train.cols : train.rows;  // every partner row inside the CSR counts
    }
    const int unsolved = (implicit ? ials_half_step : als_half_step)(train.als, rows_of_side, p, users ? m.rows : m.cols, stream, cg_steps);
    m.other_in_sync = false;  // Q moved on without the ping-pong pair
    return unsolved;
}
}  // namespace

int DeviceModel::als(const DeviceCsr &train, const cu2rec_hyper &h, int side, hipStream_t stream, int cg_steps) {
    return als_half_step_of(*this, AlsKind::Explicit, train, h, 0.f, side, stream, cg_steps);
}

int DeviceModel::ials(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, hipStream_t stream, int cg_steps) {
    return als_half_step_of(*this, AlsKind::Implicit, train, h, alpha, side, stream, cg_steps);
}

double DeviceModel::implicit_objective(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, hipStream_t stream) {
    const Need need{"cu2rec_model_implicit_objective"};
    need(finite_at_least(h.P_reg, 0.f) && finite_at_least(h.Q_reg, 0.f), CU2REC_EINVAL, ": the factor regularisers must be finite and >= 0");
    need(finite_at_least(alpha, 0.f), CU2REC_EINVAL, ": alpha must be finite and >= 0");
    need(train.rows <= rows && train.max_item < cols && train.cols <= cols, CU2REC_EINVAL, ": ratings exceed the model's shape");
    need(n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
    enter(*this);
    const AlsObjectiveProblem o{train.indptr.ptr, train.indices.ptr, train.data.ptr, train.rows, train.cols, train.nnz,
                                P.ptr, ld, Q.ptr, ldq, n_factors, alpha, h.P_reg, h.Q_reg};
    return ials_objective(train.als, o, stream);
}

// Logistic matrix factorization and Bayesian Personalized Ranking (include/cu2rec_amd.h: cu2rec_model_lmf, cu2rec_model_bpr).  The
// checks of ials(), in its order, and the sweep's, before the device.
void DeviceModel::logistic_check(const char *fn, const DeviceCsr &train, const cu2rec_hyper &h, std::optional<float> alpha,
                                 std::optional<int> side, std::optional<long long> sweep) const {
    const Need need{fn};
    need(!side || is_side(*side), CU2REC_EINVAL, ": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS");
    for (float reg : {h.P_reg, h.Q_reg, h.user_bias_reg, h.item_bias_reg})
        need(finite_at_least(reg, 0.f), CU2REC_EINVAL, ": every regulariser must be finite and >= 0");
    need(!alpha || finite_at_least(*alpha, 0.f), CU2REC_EINVAL, ": alpha must be finite and >= 0");
    need(std::isfinite(h.learning_rate) && h.learning_rate > 0.f, CU2REC_EINVAL, ": learning_rate must be finite and > 0");
    need(train.rows <= rows && train.max_item < cols && train.cols <= cols, CU2REC_EINVAL, ": entries exceed the model's shape");
    need(!sweep || (*sweep >= 0 && *sweep < kBprMaxSweep), CU2REC_EINVAL, ": sweep must be in [0, 2^29)");
    need(n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
}

void DeviceModel::download_gradient(int n_own, float *grad_out, float *bias_grad_out, hipStream_t stream) {
    const size_t ldg = static_cast<size_t>(32) * lmf_tiles(n_factors) * sizeof(float);
    CU2REC_HIP(hipStreamSynchronize(stream));
    if (grad_out)
        CU2REC_HIP(hipMemcpy2D(grad_out, static_cast<size_t>(n_factors) * sizeof(float), lmf_st.grad.ptr, ldg,
                               static_cast<size_t>(n_factors) * sizeof(float), n_own, hipMemcpyDeviceToHost));
    if (bias_grad_out)
        CU2REC_HIP(hipMemcpy2D(bias_grad_out, sizeof(float), lmf_st.grad.ptr + n_factors, ldg, sizeof(float), n_own, hipMemcpyDeviceToHost));
}

int DeviceModel::adagrad_half_step(const LmfProblem &p, bool users, hipStream_t stream) {
    const int unchanged = lmf_step(lmf_st, p, users ? lmf_st.aP.ptr : lmf_st.aQ.ptr, users ? lmf_st.a_ub.ptr : lmf_st.a_ib.ptr, stream);
    other_in_sync = false;  // Q may have moved on without the ping-pong pair
    return unchanged;
}

namespace {
// the half-step's view of one side
LmfProblem lmf_problem(DeviceModel &m, const DeviceCsr &train, const cu2rec_hyper &h, float alpha, bool users, hipStream_t stream) {
    const RatingsRef s = side_rows(train, users, stream);
    const SideView v = side_view(m, users);
    return {s.indptr, s.indices, s.data, v.own, v.ld_own, v.own_bias, s.n_rows, v.partner, v.ld_partner,
            v.partner_bias, users ? train.cols : train.rows, m.n_factors, m.global_bias, alpha, users ? h.P_reg : h.Q_reg,
            users ? h.user_bias_reg : h.item_bias_reg, h.learning_rate};
}

void lmf_ensure_state(DeviceModel &m) {  // allocated zeroed by the first logistic call
    if (m.lmf_st.aP.ptr) return;
    m.lmf_st.aP.allocate(std::max<size_t>(m.P.count, 1));
    m.lmf_st.aQ.allocate(std::max<size_t>(m.Q.count, 1));
    m.lmf_st.a_ub.allocate(m.user_bias.count);
    m.lmf_st.a_ib.allocate(m.item_bias.count);
    m.lmf_reset();
}
}  // namespace

int DeviceModel::lmf(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, hipStream_t stream) {
    logistic_check("cu2rec_model_lmf", train, h, alpha, side, {});
    enter(*this);
    lmf_ensure_state(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    const LmfProblem p = lmf_problem(*this, train, h, alpha, users, stream);
    cu2rec::lmf_gradient(lmf_st, p, stream);
    return adagrad_half_step(p, users, stream);
}

void DeviceModel::lmf_gradient(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, float *grad_out, float *bias_grad_out,
                               hipStream_t stream) {
    logistic_check("cu2rec_model_lmf_gradient", train, h, alpha, side, {});
    enter(*this);
    const LmfProblem p = lmf_problem(*this, train, h, alpha, side == CU2REC_SIDE_USERS, stream);
    if (p.n_own == 0) return;
    cu2rec::lmf_gradient(lmf_st, p, stream);
    download_gradient(p.n_own, grad_out, bias_grad_out, stream);
}

double DeviceModel::lmf_objective(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, hipStream_t stream) {
    logistic_check("cu2rec_model_lmf_objective", train, h, alpha, {}, {});
    enter(*this);
    const LmfProblem p = lmf_problem(*this, train, h, alpha, true, stream);
    const double dense = lmf_dense_objective(lmf_st, p, stream);
    double s[5];
    lmf_sparse_objective(lmf_st, p, train.nnz, s, stream);
    return (s[0] - dense) - 0.5 * (static_cast<double>(h.P_reg) * s[1] + static_cast<double>(h.user_bias_reg) * s[2] +
                                   static_cast<double>(h.Q_reg) * s[3] + static_cast<double>(h.item_bias_reg) * s[4]);
}

namespace {
// the kernels' view; items: with the CSR's item-major view
BprProblem bpr_problem(DeviceModel &m, const DeviceCsr &train, const cu2rec_hyper &h, bool items, hipStream_t stream) {
    BprProblem p{train.indptr.ptr, train.indices.ptr, train.rows, train.cols, train.nnz, nullptr, nullptr, nullptr, m.P.ptr, m.ld,
                 m.Q.ptr, m.ldq, m.item_bias.ptr, m.n_factors, h.P_reg, h.Q_reg, h.item_bias_reg};
    if (items) {
        const ItemMajorView &v = item_major_view(train, stream);
        p.t_indptr = v.indptr.ptr;
        p.t_indices = v.indices.ptr;
        p.t_pos = v.pos.ptr;
    }
    return p;
}

// st.grad = the gradient of `side` over (seed, sweep)'s triples, in lmf_step's layout
void bpr_gradient_into(LmfState &st, const DeviceCsr &train, const BprProblem &p, uint64_t seed, int sweep, bool users, hipStream_t stream) {
    const int ldg = 32 * lmf_tiles(p.n_factors);
    const size_t need = static_cast<size_t>(std::max(users ? p.rows : p.cols, 1)) * ldg;
    if (st.grad.count < need) st.grad.allocate(need);
    bpr_negatives(train, p, seed, sweep, stream);
    (users ? bpr_user_gradient : bpr_item_gradient)(train, p, st.grad.ptr, ldg, stream);
}
}  // namespace

int DeviceModel::bpr(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, int side, hipStream_t stream) {
    logistic_check("cu2rec_model_bpr", train, h, {}, side, sweep);
    enter(*this);
    lmf_ensure_state(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    bpr_gradient_into(lmf_st, train, bpr_problem(*this, train, h, !users, stream), seed, sweep, users, stream);
    // the rows that move, and the learning rate
    return adagrad_half_step(lmf_problem(*this, train, h, 0.f, users, stream), users, stream);
}

void DeviceModel::bpr_gradient(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, int side, float *grad_out,
                               float *bias_grad_out, hipStream_t stream) {
    logistic_check("cu2rec_model_bpr_gradient", train, h, {}, side, sweep);
    enter(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    const int n_own = users ? train.rows : train.cols;
    if (n_own == 0) return;
    bpr_gradient_into(lmf_st, train, bpr_problem(*this, train, h, !users, stream), seed, sweep, users, stream);
    download_gradient(n_own, grad_out, bias_grad_out, stream);
}

double DeviceModel::bpr_objective(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, long long *n_triples,
                                  long long *n_ordered, hipStream_t stream) {
    logistic_check("cu2rec_model_bpr_objective", train, h, {}, {}, sweep);
    enter(*this);
    const BprProblem p = bpr_problem(*this, train, h, false, stream);
    bpr_negatives(train, p, seed, sweep, stream);
    double s[6];
    cu2rec::bpr_objective(train, p, s, stream);
    if (n_triples) *n_triples = static_cast<long long>(s[4]);
    if (n_ordered) *n_ordered = static_cast<long long>(s[5]);
    return s[0] - 0.5 * (static_cast<double>(h.P_reg) * s[1] + static_cast<double>(h.Q_reg) * s[2] + static_cast<double>(h.item_bias_reg) * s[3]);
}

// Softmax matrix factorization (include/cu2rec_amd.h: cu2rec_model_softmax).  The logistic calls' checks in their order, without an
// alpha and without the user bias' regulariser: the user biases cancel in the softmax and are never trained.
void DeviceModel::softmax_check(const char *fn, const DeviceCsr &train, const cu2rec_hyper &h, std::optional<int> side) const {
    const Need need{fn};
    need(!side || is_side(*side), CU2REC_EINVAL, ": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS");
    for (float reg : {h.P_reg, h.Q_reg, h.item_bias_reg})
        need(finite_at_least(reg, 0.f), CU2REC_EINVAL, ": P_reg, Q_reg and item_bias_reg must be finite and >= 0");
    need(std::isfinite(h.learning_rate) && h.learning_rate > 0.f, CU2REC_EINVAL, ": learning_rate must be finite and > 0");
    need(train.rows <= rows && train.max_item < cols && train.cols <= cols, CU2REC_EINVAL, ": entries exceed the model's shape");
    need(n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
}

namespace {
// softmax_st of the users inside `train` at the model's current values -> the user side's view
LmfProblem softmax_enter(DeviceModel &m, const DeviceCsr &train, const cu2rec_hyper &h, hipStream_t stream) {
    enter(m);
    const LmfProblem users = lmf_problem(m, train, h, 1.f, true, stream);
    cu2rec::softmax_lse(m.softmax_st, users, stream);
    return users;
}
}  // namespace

int DeviceModel::softmax(const DeviceCsr &train, const cu2rec_hyper &h, int side, hipStream_t stream) {
    softmax_check("cu2rec_model_softmax", train, h, side);
    const LmfProblem user_side = softmax_enter(*this, train, h, stream);
    lmf_ensure_state(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    const LmfProblem p = users ? user_side : lmf_problem(*this, train, h, 1.f, false, stream);
    cu2rec::softmax_gradient(lmf_st, softmax_st, p, users, stream);
    return adagrad_half_step(p, users, stream);
}

void DeviceModel::softmax_gradient(const DeviceCsr &train, const cu2rec_hyper &h, int side, float *grad_out, float *bias_grad_out,
                                   hipStream_t stream) {
    softmax_check("cu2rec_model_softmax_gradient", train, h, side);
    const LmfProblem user_side = softmax_enter(*this, train, h, stream);
    const bool users = side == CU2REC_SIDE_USERS;
    const LmfProblem p = users ? user_side : lmf_problem(*this, train, h, 1.f, false, stream);
    if (p.n_own == 0) return;
    cu2rec::softmax_gradient(lmf_st, softmax_st, p, users, stream);
    download_gradient(p.n_own, grad_out, bias_grad_out, stream);
}

double DeviceModel::softmax_objective(const DeviceCsr &train, const cu2rec_hyper &h, hipStream_t stream) {
    softmax_check("cu2rec_model_softmax_objective", train, h, {});
    const LmfProblem users = softmax_enter(*this, train, h, stream);
    double s[4];
    softmax_objective_sums(lmf_st, softmax_st, users, train.nnz, s, stream);
    return s[0] - 0.5 * (static_cast<double>(h.P_reg) * s[1] + static_cast<double>(h.Q_reg) * s[2] + static_cast<double>(h.item_bias_reg) * s[3]);
}

void DeviceModel::softmax_lse(const DeviceCsr &train, float *lse_out, float *mass_out, hipStream_t stream) {
    const Need need{"cu2rec_model_softmax_lse"};
    need(train.rows <= rows && train.max_item < cols && train.cols <= cols, CU2REC_EINVAL, ": entries exceed the model's shape");
    need(n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
    const LmfProblem users = softmax_enter(*this, train, cu2rec_hyper{}, stream);
    if (train.rows == 0) return;
    if (mass_out) {
        cu2rec::softmax_gradient(lmf_st, softmax_st, users, true, stream, /*mass=*/true);
        download_gradient(train.rows, nullptr, mass_out, stream);
    }
    CU2REC_HIP(hipStreamSynchronize(stream));
    if (lse_out) softmax_st.lse.download(lse_out, train.rows);
}

void DeviceModel::lmf_download_state(float *aP, float *aQ, float *a_ub, float *a_ib) {
    if (!lmf_st.aP.ptr) {
        if (aP) std::fill(aP, aP + static_cast<size_t>(rows) * n_factors, 0.f);
        if (aQ) std::fill(aQ, aQ + static_cast<size_t>(cols) * n_factors, 0.f);
        if (a_ub) std::fill(a_ub, a_ub + rows, 0.f);
        if (a_ib) std::fill(a_ib, a_ib + cols, 0.f);
        return;
    }
    CU2REC_HIP(hipDeviceSynchronize());
    if (aP) download_padded(lmf_st.aP, aP, rows, n_factors, ld);
    if (aQ) download_padded(lmf_st.aQ, aQ, cols, n_factors, ldq);
    if (a_ub && rows) lmf_st.a_ub.download(a_ub, rows);
    if (a_ib && cols) lmf_st.a_ib.download(a_ib, cols);
}

void DeviceModel::lmf_reset() {
    if (!lmf_st.aP.ptr) return;
    CU2REC_HIP(hipDeviceSynchronize());
    lmf_st.aP.zero();
    lmf_st.aQ.zero();
    lmf_st.a_ub.zero();
    lmf_st.a_ib.zero();
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

// the four ALS half-step entry points: the null check (and, cg: the step count's) under the entry's own name, then the half-step
static int als_entry(const char *fn, AlsKind kind, cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha,
                     int side, bool cg, int cg_steps, int *unsolved) {
    return guarded([&] {
        Need{fn}(m && train && hyper, CU2REC_EINVAL, ": null argument");
        if (cg) require_cg_steps(fn, cg_steps);
        const int n = kind == AlsKind::Implicit ? m->impl.ials(train->impl, *hyper, alpha, side, nullptr, cg ? cg_steps : 0)
                                                : m->impl.als(train->impl, *hyper, side, nullptr, cg ? cg_steps : 0);
        if (unsolved) *unsolved = n;
    });
}

int cu2rec_model_als(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, int *unsolved) {
    return als_entry("cu2rec_model_als", AlsKind::Explicit, m, train, hyper, 0.f, side, false, 0, unsolved);
}

int cu2rec_model_als_cg(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, int cg_steps, int *unsolved) {
    return als_entry("cu2rec_model_als_cg", AlsKind::Explicit, m, train, hyper, 0.f, side, true, cg_steps, unsolved);
}

int cu2rec_model_als_implicit(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side,
                              int *unsolved) {
    return als_entry("cu2rec_model_als_implicit", AlsKind::Implicit, m, train, hyper, alpha, side, false, 0, unsolved);
}

int cu2rec_model_als_implicit_cg(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side,
                                 int cg_steps, int *unsolved) {
    return als_entry("cu2rec_model_als_implicit_cg", AlsKind::Implicit, m, train, hyper, alpha, side, true, cg_steps, unsolved);
}

int cu2rec_model_implicit_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, double *L) {
    return guarded([&] {
        require(m && train && hyper && L, "cu2rec_model_implicit_objective: null argument");
        *L = m->impl.implicit_objective(train->impl, *hyper, alpha, nullptr);
    });
}

int cu2rec_model_lmf(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side, int *n_unchanged) {
    return guarded([&] {
        require(m && train && hyper, "cu2rec_model_lmf: null argument");
        const int n = m->impl.lmf(train->impl, *hyper, alpha, side, nullptr);
        if (n_unchanged) *n_unchanged = n;
    });
}

int cu2rec_model_lmf_gradient(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side,
                              float *grad_out, float *bias_grad_out) {
    return guarded([&] {
        require(m && train && hyper, "cu2rec_model_lmf_gradient: null argument");
        m->impl.lmf_gradient(train->impl, *hyper, alpha, side, grad_out, bias_grad_out, nullptr);
    });
}

int cu2rec_model_lmf_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, double *L) {
    return guarded([&] {
        require(m && train && hyper && L, "cu2rec_model_lmf_objective: null argument");
        *L = m->impl.lmf_objective(train->impl, *hyper, alpha, nullptr);
    });
}

int cu2rec_model_bpr(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, int sweep, int side,
                     int *n_unchanged) {
    return guarded([&] {
        require(m && train && hyper, "cu2rec_model_bpr: null argument");
        const int n = m->impl.bpr(train->impl, *hyper, seed, sweep, side, nullptr);
        if (n_unchanged) *n_unchanged = n;
    });
}

int cu2rec_model_bpr_gradient(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, int sweep, int side,
                              float *grad_out, float *bias_grad_out) {
    return guarded([&] {
        require(m && train && hyper, "cu2rec_model_bpr_gradient: null argument");
        m->impl.bpr_gradient(train->impl, *hyper, seed, sweep, side, grad_out, bias_grad_out, nullptr);
    });
}

int cu2rec_model_bpr_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, int sweep, double *L,
                               long long *n_triples, long long *n_ordered) {
    return guarded([&] {
        require(m && train && hyper && L, "cu2rec_model_bpr_objective: null argument");
        *L = m->impl.bpr_objective(train->impl, *hyper, seed, sweep, n_triples, n_ordered, nullptr);
    });
}

int cu2rec_csr_bpr_negatives(const cu2rec_csr *train, uint64_t seed, int sweep, int *neg_out) {
    return guarded([&] {
        require(train && neg_out, "cu2rec_csr_bpr_negatives: null argument");
        Need{"cu2rec_csr_bpr_negatives"}(sweep >= 0 && sweep < kBprMaxSweep, CU2REC_EINVAL, ": sweep must be in [0, 2^29)");
        const DeviceCsr &t = train->impl;
        require_device();
        const BprProblem p{t.indptr.ptr, t.indices.ptr, t.rows, t.cols, t.nnz, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr,
                           0, 0.f, 0.f, 0.f};
        bpr_negatives(t, p, seed, sweep, nullptr);
        CU2REC_HIP(hipStreamSynchronize(nullptr));
        if (t.nnz) t.bpr.neg.download(neg_out, t.nnz);
    });
}

int cu2rec_model_softmax(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, int *n_unchanged) {
    return guarded([&] {
        require(m && train && hyper, "cu2rec_model_softmax: null argument");
        const int n = m->impl.softmax(train->impl, *hyper, side, nullptr);
        if (n_unchanged) *n_unchanged = n;
    });
}

int cu2rec_model_softmax_gradient(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, float *grad_out,
                                  float *bias_grad_out) {
    return guarded([&] {
        require(m && train && hyper, "cu2rec_model_softmax_gradient: null argument");
        m->impl.softmax_gradient(train->impl, *hyper, side, grad_out, bias_grad_out, nullptr);
    });
}

int cu2rec_model_softmax_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, double *L) {
    return guarded([&] {
        require(m && train && hyper && L, "cu2rec_model_softmax_objective: null argument");
        *L = m->impl.softmax_objective(train->impl, *hyper, nullptr);
    });
}

int cu2rec_model_softmax_lse(cu2rec_model *m, const cu2rec_csr *train, float *lse_out) {
    return guarded([&] {
        require(m && train && lse_out, "cu2rec_model_softmax_lse: null argument");
        m->impl.softmax_lse(train->impl, lse_out, nullptr, nullptr);
    });
}

int cu2rec_model_softmax_mass(cu2rec_model *m, const cu2rec_csr *train, float *mass_out) {
    return guarded([&] {
        require(m && train && mass_out, "cu2rec_model_softmax_mass: null argument");
        m->impl.softmax_lse(train->impl, nullptr, mass_out, nullptr);
    });
}

int cu2rec_model_lmf_state(cu2rec_model *m, float *aP, float *aQ, float *a_ub, float *a_ib) {
    return guarded([&] {
        require(m, "cu2rec_model_lmf_state: model is null");
        m->impl.lmf_download_state(aP, aQ, a_ub, a_ib);
    });
}

int cu2rec_model_lmf_reset(cu2rec_model *m) {
    return guarded([&] {
        require(m, "cu2rec_model_lmf_reset: model is null");
        m->impl.lmf_reset();
    });
}

}  // extern "C"
