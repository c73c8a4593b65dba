// The raw-pointer hot path of the C ABI: the SGD modes, the loss pass and the error metrics on caller-owned device memory, and
// their extern "C" wrappers.  Host code calls HIP directly; there is no CPU fallback anywhere in this file.
#include <algorithm>
#include <cmath>
#include <string>

#include "device.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "resident.hpp"

namespace cu2rec {

namespace {

hipStream_t as_stream(void *s) { return static_cast<hipStream_t>(s); }


void check_ld(int ld, int n_factors, const char *what) {
    if (ld < n_factors || (ld & 3) != 0)
        fail(CU2REC_EINVAL, std::string(what) + ": row stride must be a multiple of 4 floats and >= n_factors");
}

void check_aligned(const void *p, const char *what) {
    if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0)
        fail(CU2REC_EINVAL, std::string(what) + ": factor matrix must be 16-byte aligned");
}

// The one validation of a factor view: row strides, then alignment.  n_factors > 0 stays in each caller's own "bad shape" check,
// which names the caller and holds for a loss over no ratings too; so do the null checks: such a loss reads no pointer.
void check_factors(const FactorsRef &m) {
    check_ld(m.ldp, m.n_factors, "P");
    check_ld(m.ldq, m.n_factors, "Q");
    check_aligned(m.P, "P");
    check_aligned(m.Q, "Q");
}

// Per-block partial sums come back to the host and are added there in block order, so the result
// does not depend on scheduling (the reference also sums its 256 block partials on the host,
// loss.cu:183-189).
struct PartialSums {
    double sum_abs = 0.0, sum_sq = 0.0;
};

// The per-block partial sums are added ON THE DEVICE (one more tiny launch, 6 us) and two doubles come back, into pinned memory:
// the reference copies every block's partial sum back and adds them on the host, twice per metric pair (loss.cu:183-190), and
// so did rounds 1-2 here (64 KB through a pageable staging copy).
PartialSums collect_partials(double *device_partials, int blocks, hipStream_t stream) {
    // two doubles of pinned memory per host thread, released with the thread (the runtime may be gone by then: errors ignored)
    struct Pinned {
        double *p = nullptr;
        ~Pinned() {
            if (p) (void)hipHostFree(p);
        }
    };
    thread_local Pinned holder;
    if (!holder.p) CU2REC_HIP(hipHostMalloc(reinterpret_cast<void **>(&holder.p), 2 * sizeof(double), hipHostMallocDefault));
    double *pinned = holder.p;
    launch_partials_reduce(device_partials, blocks, stream);
    CU2REC_HIP(hipGetLastError());
    CU2REC_HIP(hipMemcpyAsync(pinned, device_partials + 2 * kMaxPartialBlocks, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    CU2REC_HIP(hipStreamSynchronize(stream));
    PartialSums s;
    s.sum_abs = pinned[0];
    s.sum_sq = pinned[1];
    return s;
}

}  // namespace

SgdArgs make_sgd_args(const RatingsRef &r, const FactorsRef &m, int n_cols, const cu2rec_hyper &hyper, uint64_t seed,
                      int update_items, int user_offset) {
    require(r.indptr && m.P && m.Q && m.user_bias && m.item_bias, "cu2rec_sgd_update: null device pointer");
    require(r.n_rows >= 0 && n_cols >= 0 && m.n_factors > 0, "cu2rec_sgd_update: bad shape");
    require(r.n_rows == 0 || (r.indices && r.data), "cu2rec_sgd_update: null device pointer");
    check_factors(m);
    SgdArgs a{};
    a.indptr = r.indptr;
    a.indices = r.indices;
    a.data = r.data;
    a.P = m.P;
    a.Q = m.Q;
    a.user_bias = m.user_bias;
    a.item_bias = m.item_bias;
    a.n_rows = r.n_rows;
    a.ldp = m.ldp;
    a.ldq = m.ldq;
    a.nslots = (m.n_factors + 3) / 4;
    a.global_bias = m.global_bias;
    a.h = SgdHyper{hyper.learning_rate, hyper.P_reg, hyper.Q_reg, hyper.user_bias_reg, hyper.item_bias_reg};
    a.seed = seed;
    a.update_items = update_items ? 1 : 0;
    a.user_offset = user_offset;
    return a;
}

namespace {
// the loss pass's argument block, validated like make_sgd_args's (nnz > 0: every array is read)
LossArgs make_loss_args(const RatingsRef &r, int nnz, const FactorsRef &m, float *errors_out, void *workspace) {
    require(r.indptr && r.indices && r.data && m.P && m.Q && m.user_bias && m.item_bias && workspace,
            "cu2rec_loss: null device pointer");
    check_factors(m);
    LossArgs a{};
    a.indptr = r.indptr;
    a.indices = r.indices;
    a.data = r.data;
    a.P = m.P;
    a.Q = m.Q;
    a.user_bias = m.user_bias;
    a.item_bias = m.item_bias;
    a.n_rows = r.n_rows;
    a.nnz = nnz;
    a.ldp = m.ldp;
    a.ldq = m.ldq;
    a.nslots = (m.n_factors + 3) / 4;
    a.global_bias = m.global_bias;
    a.errors_out = errors_out;
    a.partials = static_cast<double *>(workspace);
    return a;
}
}  // namespace

void sgd_update(const RatingsRef &r, const FactorsRef &m, int n_cols, const cu2rec_hyper &hyper, uint64_t seed,
                uint64_t iter0, int n_iters, int mode, int update_items, int user_offset, hipStream_t stream,
                const void *sample_pairs) {
    require(mode == CU2REC_SGD_HOGWILD || mode == CU2REC_SGD_SERIAL,
            "cu2rec_sgd_update: unknown mode (CU2REC_SGD_ORDERED needs cu2rec_sgd_update_ordered and a schedule)");
    require(n_iters >= 0, "cu2rec_sgd_update: bad iteration count");
    SgdArgs a = make_sgd_args(r, m, n_cols, hyper, seed, update_items, user_offset);
    if (r.n_rows == 0 || n_iters == 0) return;
    require_device();
    check_faults();
    require((reinterpret_cast<uintptr_t>(sample_pairs) & 7u) == 0, "cu2rec_sgd_update: sample pairs must be 8-byte aligned");
    a.pairs = static_cast<const uint2 *>(sample_pairs);
    if (mode == CU2REC_SGD_SERIAL) {
        // one launch walks all iterations in order
        a.iter0 = iter0;
        a.iters = n_iters;
        launch_sgd(a, mode, stream);
    } else {
        // one launch per reference iteration (training.cu:107-113): the kernel boundary is the
        // point where every user's update of iteration i is visible to iteration i+1
        // frozen items (is_train == false, predict.cu:105,126): no update crosses users, so the whole call is ONE launch
        // with every user's row in registers for all its iterations -- the same results as one launch per iteration
        const int block = update_items ? 1 : n_iters;
        // the same iterations in ONE persistent launch (grid barrier where the kernel boundary was, user rows
        // resident in registers) whenever the rows fit and the policy allows it: resident.hip
        // (n_cols > 0: in a resident launch users without ratings read item row 0 and write to a sink)
        if (block == 1 && n_cols > 0 && resident_launch(a, iter0, n_iters, stream)) return;
        for (int i = 0; i < n_iters; i += block) {
            a.iter0 = iter0 + static_cast<uint64_t>(i);
            a.iters = std::min(block, n_iters - i);
            launch_sgd(a, mode, stream);
        }
    }
    CU2REC_HIP(hipGetLastError());
}

bool sgd_update_pingpong(const RatingsRef &r, const FactorsRef &m, int n_cols, const PingPongArgs &other,
                         const cu2rec_hyper &hyper, uint64_t seed, uint64_t iter0, int n_iters, int update_items,
                         int user_offset, bool swap_last, hipStream_t stream) {
    require(n_iters >= 0, "cu2rec_sgd_update_pingpong: bad iteration count");
    require(other.Q_target && other.item_bias_target && other.claim, "cu2rec_sgd_update_pingpong: null device pointer");
    check_aligned(other.Q_target, "Q_target");
    SgdArgs a = make_sgd_args(r, m, n_cols, hyper, seed, update_items, user_offset);
    if (r.n_rows == 0 || n_iters == 0) return false;
    require_device();
    check_faults();
    // claims carry the iteration number; a call may restart from an earlier one, so they start from "nobody"
    CU2REC_HIP(hipMemsetAsync(other.claim, 0xFF, static_cast<size_t>(std::max(n_cols, 1)) * sizeof(unsigned long long), stream));
    PingPongArgs pp = other;
    a.iters = 1;
    bool swapped = false;
    for (int i = 0; i < n_iters; ++i) {  // one claim + one update launch per iteration (training.cu:107-113)
        a.iter0 = iter0 + static_cast<uint64_t>(i);
        launch_sgd_pingpong(a, pp, stream);
        if (i + 1 < n_iters || swap_last) {  // training.cu:164-165
            std::swap(a.Q, pp.Q_target);
            std::swap(a.item_bias, pp.item_bias_target);
            swapped = !swapped;
        }
    }
    CU2REC_HIP(hipGetLastError());
    return swapped;
}

void sample_pairs_build(const int *indices, const float *data, int nnz, void *pairs, hipStream_t stream) {
    require(nnz >= 0, "cu2rec_sample_pairs_build: bad size");
    if (nnz == 0) return;
    require(indices && data && pairs, "cu2rec_sample_pairs_build: null device pointer");
    require((reinterpret_cast<uintptr_t>(pairs) & 7u) == 0, "cu2rec_sample_pairs_build: pairs must be 8-byte aligned");
    require_device();
    launch_sample_pairs_build(indices, data, static_cast<size_t>(nnz), static_cast<uint2 *>(pairs), stream);
    CU2REC_HIP(hipGetLastError());
}

void sgd_update_ordered(OrderedSchedule &schedule, const RatingsRef &r, const FactorsRef &m, int n_cols,
                        const cu2rec_hyper &hyper, uint64_t seed, uint64_t iter0, int n_iters, int update_items,
                        int user_offset, hipStream_t stream, bool blocksolve) {
    if (!update_items) {
        // frozen items: no two updates of an iteration share a written row, so the parallel schedule IS the
        // sequential result; no chains needed
        sgd_update(r, m, n_cols, hyper, seed, iter0, n_iters, CU2REC_SGD_HOGWILD, 0, user_offset, stream);
        return;
    }
    require(n_iters >= 0, "cu2rec_sgd_update_ordered: bad iteration count");
    require(schedule.n_rows == r.n_rows && schedule.n_cols == n_cols, "cu2rec_sgd_update_ordered: schedule built for another CSR");
    SgdArgs a = make_sgd_args(r, m, n_cols, hyper, seed, update_items, user_offset);
    if (r.n_rows == 0 || n_iters == 0) return;
    require_device();
    check_faults();
    schedule.run(a, iter0, n_iters, stream, blocksolve);
}

void loss(const RatingsRef &r, int nnz, const FactorsRef &m, float *errors_out, void *workspace, double *sum_abs,
          double *sum_sq, float *mae, float *rmse, hipStream_t stream) {
    require(r.n_rows >= 0 && nnz >= 0 && m.n_factors > 0, "cu2rec_loss: bad shape");
    PartialSums s;
    if (nnz > 0) {
        const LossArgs a = make_loss_args(r, nnz, m, errors_out, workspace);
        require_device();
        check_faults();
        const int blocks = loss_blocks(nnz);
        launch_loss(a, blocks, stream);
        CU2REC_HIP(hipGetLastError());
        s = collect_partials(a.partials, blocks, stream);
        check_faults();  // the stream has been drained: a resident launch before this pass has reported by now
    }
    if (sum_abs) *sum_abs = s.sum_abs;
    if (sum_sq) *sum_sq = s.sum_sq;
    // loss.cu:189: total / n and sqrt(total / n), narrowed to float by the return type
    if (mae) *mae = static_cast<float>(s.sum_abs / nnz);
    if (rmse) *rmse = static_cast<float>(std::sqrt(s.sum_sq / nnz));
}

void error_metrics(const float *errors, int n, void *workspace, float *mae, float *rmse, hipStream_t stream) {
    require(n >= 0, "cu2rec_error_metrics: bad size");
    PartialSums s;
    if (n > 0) {
        require(errors && workspace, "cu2rec_error_metrics: null device pointer");
        require_device();
        const int blocks = error_metrics_blocks(n);
        launch_error_metrics(errors, n, static_cast<double *>(workspace), blocks, stream);
        CU2REC_HIP(hipGetLastError());
        s = collect_partials(static_cast<double *>(workspace), blocks, stream);
    }
    if (mae) *mae = static_cast<float>(s.sum_abs / n);
    if (rmse) *rmse = static_cast<float>(std::sqrt(s.sum_sq / n));
}

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_sgd_update(const int *indptr, const int *indices, const float *data, int n_rows, int n_cols, float *P,
                      int ldp, float *Q, int ldq, float *user_bias, float *item_bias, float global_bias, int n_factors,
                      const cu2rec_hyper *hyper, uint64_t seed, uint64_t iter0, int n_iters, int mode, int update_items,
                      int user_offset, void *stream) {
    return guarded([&] {
        require(hyper, "cu2rec_sgd_update: hyper is null");
        sgd_update({indptr, indices, data, n_rows}, {P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors}, n_cols, *hyper, seed,
                   iter0, n_iters, mode, update_items, user_offset, as_stream(stream));
    });
}

int cu2rec_sgd_update_ex(const int *indptr, const int *indices, const float *data, int n_rows, int n_cols, float *P,
                         int ldp, float *Q, int ldq, float *user_bias, float *item_bias, float global_bias, int n_factors,
                         const cu2rec_hyper *hyper, uint64_t seed, uint64_t iter0, int n_iters, int mode, int update_items,
                         int user_offset, const void *sample_pairs, void *stream) {
    return guarded([&] {
        require(hyper, "cu2rec_sgd_update_ex: hyper is null");
        sgd_update({indptr, indices, data, n_rows}, {P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors}, n_cols, *hyper, seed,
                   iter0, n_iters, mode, update_items, user_offset, as_stream(stream), sample_pairs);
    });
}

size_t cu2rec_sample_pairs_bytes(int nnz) { return nnz > 0 ? static_cast<size_t>(nnz) * 8 : 0; }

int cu2rec_sample_pairs_build(const int *indices, const float *data, int nnz, void *pairs, void *stream) {
    return guarded([&] { sample_pairs_build(indices, data, nnz, pairs, as_stream(stream)); });
}

int cu2rec_sgd_update_pingpong(const int *indptr, const int *indices, const float *data, int n_rows, int n_cols,
                               float *P, int ldp, float *Q, float *Q_target, int ldq, float *user_bias,
                               float *item_bias, float *item_bias_target, unsigned long long *claim,
                               float global_bias, int n_factors, const cu2rec_hyper *hyper, uint64_t seed,
                               uint64_t iter0, int n_iters, int update_items, int user_offset, int swap_last,
                               int *swapped, void *stream) {
    return guarded([&] {
        require(hyper, "cu2rec_sgd_update_pingpong: hyper is null");
        const bool s = sgd_update_pingpong({indptr, indices, data, n_rows}, {P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors},
                                           n_cols, {Q_target, item_bias_target, claim}, *hyper, seed, iter0, n_iters, update_items,
                                           user_offset, swap_last != 0, as_stream(stream));
        if (swapped) *swapped = s ? 1 : 0;
    });
}

int cu2rec_hogwild_resident(int policy) { return resident_policy(policy); }

int cu2rec_hogwild_resident_refusals(void) { return resident_refusals(); }

int cu2rec_hogwild_resident_plan(int n_rows, int n_factors, int n_iters, int *blocks, int *users_per_group) {
    int yes = 0;
    const int rc = guarded([&] {
        require(n_rows >= 0 && n_factors > 0, "cu2rec_hogwild_resident_plan: bad shape");
        require_device();
        yes = resident_plan(n_rows, n_factors, n_iters, blocks, users_per_group) ? 1 : 0;
    });
    return rc == CU2REC_OK ? yes : rc;
}

int cu2rec_hogwild_resident_geometry(int n_rows, int n_factors, int n_cus, int *blocks, int *users_per_group,
                                     int *lds_rows) {
    return resident_geometry(n_rows, n_factors, n_cus, blocks, users_per_group, lds_rows) ? 1 : 0;
}

int cu2rec_hogwild_resident_streamed_rows(int n_rows, int n_factors, int n_cus) { return resident_streamed_rows(n_rows, n_factors, n_cus); }

int cu2rec_schedule_create(const int *indptr, const int *indices, int n_rows, int n_cols, int nnz,
                           cu2rec_schedule **out) {
    return guarded([&] {
        require(out, "out is null");
        *out = nullptr;
        *out = new cu2rec_schedule(indptr, indices, n_rows, n_cols, nnz);
    });
}

void cu2rec_schedule_destroy(cu2rec_schedule *s) { delete s; }

int cu2rec_sgd_update_ordered(cu2rec_schedule *schedule, const int *indptr, const int *indices, const float *data,
                              int n_rows, int n_cols, float *P, int ldp, float *Q, int ldq, float *user_bias,
                              float *item_bias, float global_bias, int n_factors, const cu2rec_hyper *hyper,
                              uint64_t seed, uint64_t iter0, int n_iters, int update_items, int user_offset,
                              void *stream) {
    return guarded([&] {
        require(schedule && hyper, "cu2rec_sgd_update_ordered: null argument");
        sgd_update_ordered(schedule->impl, {indptr, indices, data, n_rows}, {P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors},
                           n_cols, *hyper, seed, iter0, n_iters, update_items, user_offset, as_stream(stream));
    });
}

int cu2rec_sgd_update_blocksolve(cu2rec_schedule *schedule, const int *indptr, const int *indices, const float *data,
                                 int n_rows, int n_cols, float *P, int ldp, float *Q, int ldq, float *user_bias,
                                 float *item_bias, float global_bias, int n_factors, const cu2rec_hyper *hyper,
                                 uint64_t seed, uint64_t iter0, int n_iters, int update_items, int user_offset,
                                 void *stream) {
    return guarded([&] {
        require(schedule && hyper, "cu2rec_sgd_update_blocksolve: null argument");
        sgd_update_ordered(schedule->impl, {indptr, indices, data, n_rows}, {P, ldp, Q, ldq, user_bias, item_bias, global_bias, n_factors},
                           n_cols, *hyper, seed, iter0, n_iters, update_items, user_offset, as_stream(stream), true);
    });
}

float cu2rec_blocksolve_min_rate(float rate) { return blocksolve_min_rate(rate); }
int cu2rec_blocksolve_lookahead_blocks(int blocks) { return blocksolve_lookahead_blocks(blocks); }

size_t cu2rec_loss_workspace_bytes(void) { return sizeof(double) * (2 * kMaxPartialBlocks + 2); }

int cu2rec_loss(const int *indptr, const int *indices, const float *data, int n_rows, int nnz, const float *P, int ldp,
                const float *Q, int ldq, const float *user_bias, const float *item_bias, float global_bias,
                int n_factors, float *errors_out, void *workspace, double *sum_abs, double *sum_sq, float *mae,
                float *rmse, void *stream) {
    return guarded([&] {
        // (the view's pointers are not const: one type serves the trainers too; loss() only reads through them)
        const FactorsRef m{const_cast<float *>(P), ldp, const_cast<float *>(Q), ldq, const_cast<float *>(user_bias),
                           const_cast<float *>(item_bias), global_bias, n_factors};
        loss({indptr, indices, data, n_rows}, nnz, m, errors_out, workspace, sum_abs, sum_sq, mae, rmse, as_stream(stream));
    });
}

int cu2rec_error_metrics(const float *errors, int n, void *workspace, float *mae, float *rmse, void *stream) {
    return guarded([&] { error_metrics(errors, n, workspace, mae, rmse, as_stream(stream)); });
}

}  // extern "C"
