// Device side of the C ABI: raw-pointer hot-path entry points, owned device objects
// (the roles of CudaCSRMatrix / CudaDenseMatrix, matrix.h:11-28) and the item-factor exchange
// helpers.  Host code calls HIP directly; there is no CPU fallback anywhere in this file.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "device.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "resident.hpp"

namespace cu2rec {

namespace {
std::mutex g_runtime_mutex;
std::map<int, DeviceRuntime> g_runtime;  // per device (a map: references stay valid while other devices are added)
}  // namespace

std::mutex &device_runtime_mutex() { return g_runtime_mutex; }

DeviceRuntime &device_runtime() {
    int dev = 0;
    CU2REC_HIP(hipGetDevice(&dev));
    DeviceRuntime &r = g_runtime[dev];
    if (r.status) return r;
    unsigned *words = nullptr, *host = nullptr;
    try {
        CU2REC_HIP(hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, dev));
        CU2REC_HIP(hipMalloc(reinterpret_cast<void **>(&words), 128 * sizeof(unsigned)));
        CU2REC_HIP(hipMemset(words, 0, 128 * sizeof(unsigned)));
        CU2REC_HIP(hipHostMalloc(reinterpret_cast<void **>(&host), 2 * sizeof(unsigned), hipHostMallocDefault));
    } catch (...) {  // (nothing kept: the next use tries again)
        if (words) (void)hipFree(words);
        throw;
    }
    host[0] = host[1] = 0;
    r.host_status = host;
    r.probe = words + 64;
    r.status = words;
    return r;
}

namespace {
// the current device's record if it has one (the caller holds g_runtime_mutex); no allocation, no error
DeviceRuntime *existing_device_runtime() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    const auto found = g_runtime.find(dev);
    return found != g_runtime.end() && found->second.status ? &found->second : nullptr;
}
}  // namespace

// What a persistent or concurrent launch could not finish is reported at the next entry point, once: the words are cleared so that
// the process can go on.
static void check_faults() {
    std::lock_guard<std::mutex> lock(g_runtime_mutex);
    DeviceRuntime *found = existing_device_runtime();
    if (!found) return;
    DeviceRuntime &r = *found;
    volatile unsigned *host = r.host_status;
    if (host[0] != 0) {
        (void)hipDeviceSynchronize();
        (void)hipMemset(r.status + DeviceRuntime::kResidentWord, 0, sizeof(unsigned));
        host[0] = 0;
        fail(CU2REC_EHIP,
             "cu2rec_amd: a persistent SGD launch gave up at its grid barrier (the grid was not co-resident: is another "
             "process or stream using this GPU?); the model state is undefined.  cu2rec_hogwild_resident(0) / "
             "CU2REC_RESIDENT=0 selects the one-launch-per-iteration Hogwild kernel");
    }
    const unsigned bs = host[1];
    if (bs == 0) return;
    (void)hipDeviceSynchronize();
    (void)hipMemset(r.status + DeviceRuntime::kBlocksolveWord, 0, sizeof(unsigned));
    host[1] = 0;
    const char *ordered = "CU2REC_SGD_ORDERED is the same result without concurrent launches";
    if (bs == 2u)  // a look-ahead ring wait (blocksolve_lookahead.hpp, la_wait*): the fork / join had no part in it
        fail(CU2REC_EHIP, std::string("cu2rec_amd: a block-solve iteration gave up at a wait inside a phase-2 workgroup (its wavefronts hand "
                                      "blocks over through flags: is another process or stream holding this GPU's compute units?); the "
                                      "model state is undefined.  ") + ordered);
    // the join gave up.  Self-healing: whatever kept the launches from running side by side will do so again -- every later block-solve
    // call of this process on this device forks and joins with events (unless the environment forces the device form)
    std::string what;
    if (r.topology_forced) {
        what = "(CU2REC_BS_GATE forces the device-side form: unset it to let the library fall back to events.)  ";
    } else if (r.topology == DeviceRuntime::kTopologyEvents) {
        what = "This process already forks and joins the iteration's streams with events.  ";
    } else {
        r.topology = DeviceRuntime::kTopologyEvents;
        r.topology_why = "a device-side join gave up mid-run: switched to the event fork / join";
        what = "From here on this process forks and joins the iteration's streams with events instead of device-side waits (slower by a "
               "few microseconds per iteration, independent of concurrent execution): re-create the model and run again.  ";
    }
    fail(CU2REC_EHIP, "cu2rec_amd: a block-solve iteration gave up waiting for one of its own launches (the three phases of an iteration "
                      "run side by side and hand blocks over through flags: is another process or stream holding this GPU's compute "
                      "units?); the model state is undefined.  " + what + ordered);
}


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

void download_padded(const DeviceBuffer<float> &src, float *host, int rows, int f, int ld) {
    if (rows == 0) return;
    CU2REC_HIP(hipMemcpy2D(host, static_cast<size_t>(f) * sizeof(float), src.ptr, static_cast<size_t>(ld) * sizeof(float),
                           static_cast<size_t>(f) * sizeof(float), rows, hipMemcpyDeviceToHost));
}
}  // namespace

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

namespace {
// The rows one ALS half-step solves, as it reads them: the CSR itself for the users, its item-major view for the items -- built on
// the device, and either side planned, the first time it is asked for.
AlsSide &als_side(const DeviceCsr &train, bool users, hipStream_t stream) {
    if (!train.als) train.als.reset(new AlsCache);
    AlsCache &c = *train.als;
    if (users) {
        if (!c.users_ready) {
            c.users.indptr = train.indptr.ptr;
            c.users.indices = train.indices.ptr;
            c.users.data = train.data.ptr;
            c.users.rows = train.rows;
            c.users.nnz = train.nnz;
            als_plan_side(c.users, stream);
            c.users_ready = true;
        }
        return c.users;
    }
    if (!c.items_ready) {  // the item-major view, built on the device once per rating matrix
        als_build_transpose(c, train.indptr.ptr, train.indices.ptr, train.data.ptr, train.rows, train.cols, train.nnz, stream);
        c.items.indptr = c.t_indptr.ptr;
        c.items.indices = c.t_indices.ptr;
        c.items.data = c.t_data.ptr;
        c.items.rows = train.cols;
        c.items.nnz = train.nnz;
        als_plan_side(c.items, stream);
        c.items_ready = true;
    }
    return c.items;
}

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
    const int unsolved = (implicit ? ials_half_step : als_half_step)(*train.als, rows_of_side, p, users ? m.rows : m.cols, stream, cg_steps);
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
    if (!train.als) train.als.reset(new AlsCache);
    const AlsObjectiveProblem o{train.indptr.ptr, train.indices.ptr, train.data.ptr, train.rows, train.cols, train.nnz,
                                P.ptr, ld, Q.ptr, ldq, n_factors, alpha, h.P_reg, h.Q_reg};
    return ials_objective(*train.als, o, stream);
}

// Logistic matrix factorization (include/cu2rec_amd.h: cu2rec_model_lmf).  The checks of ials(), in its order, before the device.
void DeviceModel::lmf_check(const char *fn, const DeviceCsr &train, const cu2rec_hyper &h, float alpha, const int *side) const {
    const Need need{fn};
    need(!side || is_side(*side), CU2REC_EINVAL, ": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS");
    for (float reg : {h.P_reg, h.Q_reg, h.user_bias_reg, h.item_bias_reg})
        need(finite_at_least(reg, 0.f), CU2REC_EINVAL, ": every regulariser must be finite and >= 0");
    need(finite_at_least(alpha, 0.f), CU2REC_EINVAL, ": alpha must be finite and >= 0");
    need(std::isfinite(h.learning_rate) && h.learning_rate > 0.f, CU2REC_EINVAL, ": learning_rate must be finite and > 0");
    need(train.rows <= rows && train.max_item < cols && train.cols <= cols, CU2REC_EINVAL, ": entries exceed the model's shape");
    need(n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
}

namespace {
// the half-step's view of one side; the item side reads the item-major view cached on the CSR by the ALS calls
LmfProblem lmf_problem(DeviceModel &m, const DeviceCsr &train, const cu2rec_hyper &h, float alpha, bool users, hipStream_t stream) {
    const AlsSide &s = als_side(train, users, stream);
    const SideView v = side_view(m, users);
    return {s.indptr, s.indices, s.data, v.own, v.ld_own, v.own_bias, users ? train.rows : train.cols, v.partner, v.ld_partner,
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
    lmf_check("cu2rec_model_lmf", train, h, alpha, &side);
    enter(*this);
    lmf_ensure_state(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    const LmfProblem p = lmf_problem(*this, train, h, alpha, users, stream);
    cu2rec::lmf_gradient(lmf_st, p, stream);
    const int unchanged = lmf_step(lmf_st, p, users ? lmf_st.aP.ptr : lmf_st.aQ.ptr, users ? lmf_st.a_ub.ptr : lmf_st.a_ib.ptr, stream);
    other_in_sync = false;  // Q may have moved on without the ping-pong pair
    return unchanged;
}

void DeviceModel::lmf_gradient(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, int side, float *grad_out, float *bias_grad_out,
                               hipStream_t stream) {
    lmf_check("cu2rec_model_lmf_gradient", train, h, alpha, &side);
    enter(*this);
    const LmfProblem p = lmf_problem(*this, train, h, alpha, side == CU2REC_SIDE_USERS, stream);
    if (p.n_own == 0) return;
    cu2rec::lmf_gradient(lmf_st, p, stream);
    const size_t ldg = static_cast<size_t>(32) * lmf_tiles(n_factors) * sizeof(float);
    CU2REC_HIP(hipStreamSynchronize(stream));
    if (grad_out)
        CU2REC_HIP(hipMemcpy2D(grad_out, static_cast<size_t>(n_factors) * sizeof(float), lmf_st.grad.ptr, ldg,
                               static_cast<size_t>(n_factors) * sizeof(float), p.n_own, hipMemcpyDeviceToHost));
    if (bias_grad_out)
        CU2REC_HIP(hipMemcpy2D(bias_grad_out, sizeof(float), lmf_st.grad.ptr + n_factors, ldg, sizeof(float), p.n_own, hipMemcpyDeviceToHost));
}

double DeviceModel::lmf_objective(const DeviceCsr &train, const cu2rec_hyper &h, float alpha, hipStream_t stream) {
    lmf_check("cu2rec_model_lmf_objective", train, h, alpha, nullptr);
    enter(*this);
    const LmfProblem p = lmf_problem(*this, train, h, alpha, true, stream);
    const double dense = lmf_dense_objective(lmf_st, p, stream);
    double s[5];
    lmf_sparse_objective(lmf_st, p, train.nnz, s, stream);
    return (s[0] - dense) - 0.5 * (static_cast<double>(h.P_reg) * s[1] + static_cast<double>(h.user_bias_reg) * s[2] +
                                   static_cast<double>(h.Q_reg) * s[3] + static_cast<double>(h.item_bias_reg) * s[4]);
}

// Bayesian Personalized Ranking (include/cu2rec_amd.h: cu2rec_model_bpr).  The logistic calls' checks with their codes, and the sweep.
void DeviceModel::bpr_check(const char *fn, const DeviceCsr &train, const cu2rec_hyper &h, const int *side, long long sweep) const {
    const Need need{fn};
    need(!side || is_side(*side), CU2REC_EINVAL, ": side must be CU2REC_SIDE_USERS or CU2REC_SIDE_ITEMS");
    for (float reg : {h.P_reg, h.Q_reg, h.user_bias_reg, h.item_bias_reg})
        need(finite_at_least(reg, 0.f), CU2REC_EINVAL, ": every regulariser must be finite and >= 0");
    need(std::isfinite(h.learning_rate) && h.learning_rate > 0.f, CU2REC_EINVAL, ": learning_rate must be finite and > 0");
    need(train.rows <= rows && train.max_item < cols && train.cols <= cols, CU2REC_EINVAL, ": entries exceed the model's shape");
    need(sweep >= 0 && sweep < kBprMaxSweep, CU2REC_EINVAL, ": sweep must be in [0, 2^29)");
    need(n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, ": n_factors above 252 is not supported");
}

namespace {
// the kernels' view; items: with the item-major view cached on the CSR by the ALS calls
BprProblem bpr_problem(DeviceModel &m, const DeviceCsr &train, const cu2rec_hyper &h, bool items, hipStream_t stream) {
    BprProblem p{train.indptr.ptr, train.indices.ptr, train.rows, train.cols, train.nnz, nullptr, nullptr, nullptr, m.P.ptr, m.ld,
                 m.Q.ptr, m.ldq, m.item_bias.ptr, m.n_factors, h.P_reg, h.Q_reg, h.item_bias_reg};
    if (items) {
        const AlsSide &s = als_side(train, false, stream);
        p.t_indptr = s.indptr;
        p.t_indices = s.indices;
        p.t_pos = train.als->t_pos.ptr;
    }
    if (!train.bpr) train.bpr.reset(new BprCache);
    return p;
}

// st.grad = the gradient of `side` over (seed, sweep)'s triples, in lmf_step's layout
void bpr_gradient_into(LmfState &st, const DeviceCsr &train, const BprProblem &p, uint64_t seed, int sweep, bool users, hipStream_t stream) {
    const int ldg = 32 * lmf_tiles(p.n_factors);
    const size_t need = static_cast<size_t>(std::max(users ? p.rows : p.cols, 1)) * ldg;
    if (st.grad.count < need) st.grad.allocate(need);
    bpr_negatives(*train.bpr, p, seed, sweep, stream);
    (users ? bpr_user_gradient : bpr_item_gradient)(*train.bpr, p, st.grad.ptr, ldg, stream);
}
}  // namespace

int DeviceModel::bpr(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, int side, hipStream_t stream) {
    bpr_check("cu2rec_model_bpr", train, h, &side, sweep);
    enter(*this);
    lmf_ensure_state(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    bpr_gradient_into(lmf_st, train, bpr_problem(*this, train, h, !users, stream), seed, sweep, users, stream);
    const LmfProblem step = lmf_problem(*this, train, h, 0.f, users, stream);  // the rows that move, and the learning rate
    const int unchanged = lmf_step(lmf_st, step, users ? lmf_st.aP.ptr : lmf_st.aQ.ptr, users ? lmf_st.a_ub.ptr : lmf_st.a_ib.ptr, stream);
    other_in_sync = false;  // Q may have moved on without the ping-pong pair
    return unchanged;
}

void DeviceModel::bpr_gradient(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, int side, float *grad_out,
                               float *bias_grad_out, hipStream_t stream) {
    bpr_check("cu2rec_model_bpr_gradient", train, h, &side, sweep);
    enter(*this);
    const bool users = side == CU2REC_SIDE_USERS;
    const int n_own = users ? train.rows : train.cols;
    if (n_own == 0) return;
    bpr_gradient_into(lmf_st, train, bpr_problem(*this, train, h, !users, stream), seed, sweep, users, stream);
    const size_t ldg = static_cast<size_t>(32) * lmf_tiles(n_factors) * sizeof(float);
    CU2REC_HIP(hipStreamSynchronize(stream));
    if (grad_out)
        CU2REC_HIP(hipMemcpy2D(grad_out, static_cast<size_t>(n_factors) * sizeof(float), lmf_st.grad.ptr, ldg,
                               static_cast<size_t>(n_factors) * sizeof(float), n_own, hipMemcpyDeviceToHost));
    if (bias_grad_out)
        CU2REC_HIP(hipMemcpy2D(bias_grad_out, sizeof(float), lmf_st.grad.ptr + n_factors, ldg, sizeof(float), n_own, hipMemcpyDeviceToHost));
}

double DeviceModel::bpr_objective(const DeviceCsr &train, const cu2rec_hyper &h, uint64_t seed, int sweep, long long *n_triples,
                                  long long *n_ordered, hipStream_t stream) {
    bpr_check("cu2rec_model_bpr_objective", train, h, nullptr, sweep);
    enter(*this);
    const BprProblem p = bpr_problem(*this, train, h, false, stream);
    bpr_negatives(*train.bpr, p, seed, sweep, stream);
    double s[6];
    cu2rec::bpr_objective(*train.bpr, p, s, stream);
    if (n_triples) *n_triples = static_cast<long long>(s[4]);
    if (n_ordered) *n_ordered = static_cast<long long>(s[5]);
    return s[0] - 0.5 * (static_cast<double>(h.P_reg) * s[1] + static_cast<double>(h.Q_reg) * s[2] + static_cast<double>(h.item_bias_reg) * s[3]);
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

void DeviceModel::loss(const DeviceCsr &ratings, double *sum_abs, double *sum_sq, float *mae, float *rmse,
                       hipStream_t stream) const {
    // Appendix quirk 6: a test file may have fewer users than train, never more
    require(ratings.rows <= rows && ratings.max_item < cols, "cu2rec_model_loss: ratings exceed the model's shape");
    cu2rec::loss(ratings.ref(), ratings.nnz, ref(), nullptr, workspace.ptr, sum_abs, sum_sq, mae, rmse, stream);
}

}  // namespace cu2rec

using namespace cu2rec;

struct cu2rec_schedule {
    OrderedSchedule impl;
    template <class... A>
    explicit cu2rec_schedule(A &&...a) : impl(std::forward<A>(a)...) {}
};
struct cu2rec_csr {
    DeviceCsr impl;
    template <class... A>
    explicit cu2rec_csr(A &&...a) : impl(std::forward<A>(a)...) {}
};
struct cu2rec_model {
    DeviceModel impl;
    template <class... A>
    explicit cu2rec_model(A &&...a) : impl(std::forward<A>(a)...) {}
};

namespace cu2rec {
DeviceCsr &unwrap(cu2rec_csr *m) { return m->impl; }
const DeviceCsr &unwrap(const cu2rec_csr *m) { return m->impl; }
DeviceModel &unwrap(cu2rec_model *m) { return m->impl; }
const DeviceModel &unwrap(const cu2rec_model *m) { return m->impl; }
}  // namespace cu2rec

extern "C" {

int cu2rec_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int cu2rec_set_device(int device) {
    return guarded([&] {
        require_device();
        CU2REC_HIP(hipSetDevice(device));
    });
}

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

int cu2rec_check_faults(void) {
    return guarded([&] {
        require_device();
        CU2REC_HIP(hipDeviceSynchronize());
        check_faults();
    });
}

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

int cu2rec_blocksolve_topology(char *why, size_t cap) {
    std::string text;
    int mode = -1;
    {
        std::lock_guard<std::mutex> lock(g_runtime_mutex);
        if (const DeviceRuntime *r = existing_device_runtime()) {
            mode = r->topology;
            text = r->topology_why;
        }
    }
    if (why && cap) {
        const size_t n = std::min(text.size(), cap - 1);
        std::memcpy(why, text.data(), n);
        why[n] = 0;
    }
    return mode;
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
        if (!t.bpr) t.bpr.reset(new BprCache);
        const BprProblem p{t.indptr.ptr, t.indices.ptr, t.rows, t.cols, t.nnz, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr,
                           0, 0.f, 0.f, 0.f};
        bpr_negatives(*t.bpr, p, seed, sweep, nullptr);
        CU2REC_HIP(hipStreamSynchronize(nullptr));
        if (t.nnz) t.bpr->neg.download(neg_out, t.nnz);
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

int cu2rec_model_loss(const cu2rec_model *m, const cu2rec_csr *ratings, double *sum_abs, double *sum_sq, float *mae,
                      float *rmse) {
    return guarded([&] {
        require(m && ratings, "null argument");
        m->impl.loss(ratings->impl, sum_abs, sum_sq, mae, rmse, nullptr);
    });
}

}  // extern "C"
