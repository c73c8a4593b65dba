// The owned device objects of the C ABI (the roles of CudaCSRMatrix / CudaDenseMatrix, matrix.h:11-28): DeviceCsr, and DeviceModel's
// create / download / sgd / loss, behind the cu2rec_csr_* and cu2rec_model_* handles.  The trainers' members are device_trainers.cpp's.
#include <algorithm>
#include <vector>

#include "device.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "resident.hpp"

namespace cu2rec {

// ---------------------------------------------------------------------------------- DeviceCsr
DeviceCsr::DeviceCsr(int rows_, int cols_, int nnz_, const int *h_indptr, const int *h_indices, const float *h_data)
    : rows(rows_), cols(cols_), nnz(nnz_) {
    require(rows >= 0 && cols >= 0 && nnz >= 0 && h_indptr, "cu2rec_csr_create: bad argument");
    require(nnz == 0 || (h_indices && h_data), "cu2rec_csr_create: null indices/data");
    // the reference trusts its input (Appendix: a test file with a larger id than train reads out of
    // bounds, mf.cu:50-51); a malformed CSR would fault the GPU, so check it here on the host
    require(h_indptr[0] == 0 && h_indptr[rows] == nnz, "cu2rec_csr_create: indptr must run from 0 to nnz");
    for (int u = 0; u < rows; ++u) require(h_indptr[u] <= h_indptr[u + 1], "cu2rec_csr_create: indptr must be non-decreasing");
    max_item = -1;
    for (int k = 0; k < nnz; ++k) {
        require(h_indices[k] >= 0, "cu2rec_csr_create: negative item id");
        if (h_indices[k] > max_item) max_item = h_indices[k];
    }
    require(max_item < cols, "cu2rec_csr_create: item id >= cols");
    users_with_ratings = 0;
    for (int u = 0; u < rows; ++u) users_with_ratings += h_indptr[u + 1] > h_indptr[u];
    require_device();
    indptr.allocate(static_cast<size_t>(rows) + 1);
    indptr.upload(h_indptr, static_cast<size_t>(rows) + 1);
    indices.allocate(std::max(nnz, 1));
    data.allocate(std::max(nnz, 1));
    if (nnz) {
        indices.upload(h_indices, nnz);
        data.upload(h_data, nnz);
    }
}

// ---------------------------------------------------------------------------------- DeviceModel
namespace {
// dense host rows (stride f) -> padded device rows (stride ld, zero fill)
void upload_padded(DeviceBuffer<float> &dst, const float *host, int rows, int f, int ld) {
    dst.allocate(std::max<size_t>(static_cast<size_t>(rows) * ld, 4));
    dst.zero();
    if (rows == 0) return;
    CU2REC_HIP(hipMemcpy2D(dst.ptr, static_cast<size_t>(ld) * sizeof(float), host, static_cast<size_t>(f) * sizeof(float),
                           static_cast<size_t>(f) * sizeof(float), rows, hipMemcpyHostToDevice));
}
}  // namespace

void download_padded(const DeviceBuffer<float> &src, float *host, int rows, int f, int ld) {
    if (rows == 0) return;
    CU2REC_HIP(hipMemcpy2D(host, static_cast<size_t>(f) * sizeof(float), src.ptr, static_cast<size_t>(ld) * sizeof(float),
                           static_cast<size_t>(f) * sizeof(float), rows, hipMemcpyDeviceToHost));
}

DeviceModel::DeviceModel(int rows_, int cols_, int f_, const float *hP, const float *hQ, const float *hub,
                         const float *hib, float gb)
    : rows(rows_), cols(cols_), n_factors(f_), ld((f_ + 3) & ~3), ldq((f_ + 31) & ~31), global_bias(gb) {
    require(rows >= 0 && cols >= 0 && n_factors > 0, "cu2rec_model_create: bad shape");
    if (slots_per_lane(ld / 4) > 8) fail(CU2REC_EUNSUPPORTED, "n_factors above 512 is not compiled in");
    require_device();
    // training.cu:28,54,212-213: every array starts from initialize_normal_array(size, n_factors) with seed 42
    std::vector<float> tmp;
    auto init_if_null = [&](const float *given, size_t n) -> const float * {
        if (given) return given;
        tmp.resize(n);
        cu2rec_init_normal(tmp.data(), n, n_factors, 0.f, 1.f, 42);
        return tmp.data();
    };
    upload_padded(P, init_if_null(hP, static_cast<size_t>(rows) * n_factors), rows, n_factors, ld);
    upload_padded(Q, init_if_null(hQ, static_cast<size_t>(cols) * n_factors), cols, n_factors, ldq);
    user_bias.allocate(std::max(rows, 1));
    item_bias.allocate(std::max(cols, 1));
    if (rows) user_bias.upload(init_if_null(hub, rows), rows);
    if (cols) item_bias.upload(init_if_null(hib, cols), cols);
    workspace.allocate(static_cast<size_t>(2) * kMaxPartialBlocks + 2);
}

void DeviceModel::download(float *hP, float *hQ, float *hub, float *hib) const {
    require(!swap_pending, "cu2rec_model_download: a ping-pong swap is pending (finish_swap)");
    CU2REC_HIP(hipDeviceSynchronize());
    check_faults();
    if (hP) download_padded(P, hP, rows, n_factors, ld);
    if (hQ) download_padded(Q, hQ, cols, n_factors, ldq);
    if (hub && rows) user_bias.download(hub, rows);
    if (hib && cols) item_bias.download(hib, cols);
}

void DeviceModel::finish_swap() {
    if (!swap_pending) return;
    Q.swap(Q_other);
    item_bias.swap(item_bias_other);
    swap_pending = false;
}

void DeviceModel::sgd(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, uint64_t iter0, int n_iters, int mode,
                      int update_items, hipStream_t stream, bool defer_last_swap, int user_offset) {
    require(train.rows <= rows && train.max_item < cols, "cu2rec_model_sgd: ratings exceed the model's shape");
    finish_swap();
    const RatingsRef ratings = train.ref();
    const FactorsRef factors = ref();  // after finish_swap: Q / item_bias name the current item side
    if (mode == CU2REC_SGD_PINGPONG) {
        if (!Q_other.ptr) {
            Q_other.allocate(Q.count);
            item_bias_other.allocate(item_bias.count);
            claim.allocate(std::max(cols, 1));
        }
        if (!other_in_sync) {  // training.cu:37,69-70: the targets start as copies of Q / item_bias
            CU2REC_HIP(hipMemcpyAsync(Q_other.ptr, Q.ptr, Q.count * sizeof(float), hipMemcpyDeviceToDevice, stream));
            CU2REC_HIP(hipMemcpyAsync(item_bias_other.ptr, item_bias.ptr, item_bias.count * sizeof(float),
                                      hipMemcpyDeviceToDevice, stream));
            other_in_sync = true;
        }
        const bool swapped = sgd_update_pingpong(ratings, factors, cols, {Q_other.ptr, item_bias_other.ptr, claim.ptr}, h, seed,
                                                 iter0, n_iters, update_items, user_offset, !defer_last_swap, stream);
        if (swapped) {  // Q / item_bias always name the current item side
            Q.swap(Q_other);
            item_bias.swap(item_bias_other);
        }
        swap_pending = defer_last_swap && n_iters > 0 && train.rows > 0;
        return;
    }
    other_in_sync = false;  // another mode moves Q on without the second pair
    if (mode == CU2REC_SGD_ORDERED || mode == CU2REC_SGD_BLOCKSOLVE) {
        if (!train.schedule || train.schedule->n_cols != cols) {
            train.schedule.reset(new OrderedSchedule(train.indptr.ptr, train.indices.ptr, train.rows, cols, train.nnz));
            train.schedule->speculate = true;  // the schedule is destroyed with the arrays it reads
        }
        sgd_update_ordered(*train.schedule, ratings, factors, cols, h, seed, iter0, n_iters, update_items, user_offset, stream,
                           mode == CU2REC_SGD_BLOCKSOLVE);
        return;
    }
    const void *pairs = nullptr;
    if (mode == CU2REC_SGD_HOGWILD && update_items && train.nnz > 0 &&
        resident_plan(train.rows, n_factors, n_iters, nullptr, nullptr)) {
        if (!train.pairs.ptr) {  // first resident call on this CSR: 8 bytes per rating, built once
            train.pairs.allocate(train.nnz);
            sample_pairs_build(train.indices.ptr, train.data.ptr, train.nnz, train.pairs.ptr, stream);
        }
        pairs = train.pairs.ptr;
    }
    sgd_update(ratings, factors, cols, h, seed, iter0, n_iters, mode, update_items, user_offset, stream, pairs);
}

void DeviceModel::loss(const DeviceCsr &ratings, double *sum_abs, double *sum_sq, float *mae, float *rmse,
                       hipStream_t stream) const {
    // Appendix quirk 6: a test file may have fewer users than train, never more
    require(ratings.rows <= rows && ratings.max_item < cols, "cu2rec_model_loss: ratings exceed the model's shape");
    cu2rec::loss(ratings.ref(), ratings.nnz, ref(), nullptr, workspace.ptr, sum_abs, sum_sq, mae, rmse, stream);
}

DeviceCsr &unwrap(cu2rec_csr *m) { return m->impl; }
const DeviceCsr &unwrap(const cu2rec_csr *m) { return m->impl; }
DeviceModel &unwrap(cu2rec_model *m) { return m->impl; }
const DeviceModel &unwrap(const cu2rec_model *m) { return m->impl; }

}  // namespace cu2rec

using namespace cu2rec;

extern "C" {

int cu2rec_csr_create(int rows, int cols, int nnz, const int *indptr, const int *indices, const float *data,
                      cu2rec_csr **out) {
    return guarded([&] {
        require(out, "out is null");
        *out = nullptr;
        *out = new cu2rec_csr(rows, cols, nnz, indptr, indices, data);
    });
}

int cu2rec_csr_info(const cu2rec_csr *m, int *rows, int *cols, int *nnz) {
    return guarded([&] {
        require(m, "csr is null");
        if (rows) *rows = m->impl.rows;
        if (cols) *cols = m->impl.cols;
        if (nnz) *nnz = m->impl.nnz;
    });
}

int cu2rec_csr_device_ptrs(const cu2rec_csr *m, const int **indptr, const int **indices, const float **data) {
    return guarded([&] {
        require(m, "csr is null");
        if (indptr) *indptr = m->impl.indptr.ptr;
        if (indices) *indices = m->impl.indices.ptr;
        if (data) *data = m->impl.data.ptr;
    });
}

int cu2rec_csr_blocksolve_items(const cu2rec_csr *train) {
    int n = -1;
    const int rc = guarded([&] {
        require(train, "cu2rec_csr_blocksolve_items: null argument");
        const DeviceCsr &m = unwrap(train);
        if (!m.schedule) {
            m.schedule.reset(new OrderedSchedule(m.indptr.ptr, m.indices.ptr, m.rows, m.cols, m.nnz));
            m.schedule->speculate = true;
        }
        n = m.schedule->blocksolve_items();
    });
    return rc == CU2REC_OK ? n : -1;
}

void cu2rec_csr_destroy(cu2rec_csr *m) { delete m; }

int cu2rec_model_create(int rows, int cols, int n_factors, const float *P, const float *Q, const float *user_bias,
                        const float *item_bias, float global_bias, cu2rec_model **out) {
    return guarded([&] {
        require(out, "out is null");
        *out = nullptr;
        *out = new cu2rec_model(rows, cols, n_factors, P, Q, user_bias, item_bias, global_bias);
    });
}

int cu2rec_model_item_stride(const cu2rec_model *m) { return m ? m->impl.ldq : 0; }

int cu2rec_model_info(const cu2rec_model *m, int *rows, int *cols, int *n_factors, int *ld, float *global_bias) {
    return guarded([&] {
        require(m, "model is null");
        if (rows) *rows = m->impl.rows;
        if (cols) *cols = m->impl.cols;
        if (n_factors) *n_factors = m->impl.n_factors;
        if (ld) *ld = m->impl.ld;
        if (global_bias) *global_bias = m->impl.global_bias;
    });
}

int cu2rec_model_device_ptrs(const cu2rec_model *m, float **P, float **Q, float **user_bias, float **item_bias) {
    return guarded([&] {
        require(m, "model is null");
        if (P) *P = m->impl.P.ptr;
        if (Q) *Q = m->impl.Q.ptr;
        if (user_bias) *user_bias = m->impl.user_bias.ptr;
        if (item_bias) *item_bias = m->impl.item_bias.ptr;
    });
}

int cu2rec_model_download(const cu2rec_model *m, float *P, float *Q, float *user_bias, float *item_bias) {
    return guarded([&] {
        require(m, "model is null");
        m->impl.download(P, Q, user_bias, item_bias);
    });
}

void cu2rec_model_destroy(cu2rec_model *m) { delete m; }

int cu2rec_model_sgd(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, uint64_t iter0,
                     int n_iters, int mode, int update_items) {
    return guarded([&] {
        require(m && train && hyper, "null argument");
        m->impl.sgd(train->impl, *hyper, seed, iter0, n_iters, mode, update_items, nullptr);
    });
}

int cu2rec_model_loss(const cu2rec_model *m, const cu2rec_csr *ratings, double *sum_abs, double *sum_sq, float *mae,
                      float *rmse) {
    return guarded([&] {
        require(m && ratings, "null argument");
        m->impl.loss(ratings->impl, sum_abs, sum_sq, mae, rmse, nullptr);
    });
}

}  // extern "C"
