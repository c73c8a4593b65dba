// Item-based nearest-neighbour recommendation (include/cu2rec_amd.h: cu2rec_knn_*): a sparse x sparse product with a fused top-N
// selection, so that nothing of size items x items ever exists (knn.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "hip_check.hpp"

namespace cu2rec {

struct DeviceCsr;

constexpr int kKnnSliceItems = 2048;  // candidate ids one wavefront accumulates in LDS (cu2rec_knn_slice_items)
constexpr int kKnnMaxK = CU2REC_KNN_MAX_NEIGHBOURS;
constexpr size_t kKnnWorkspaceBytes = CU2REC_KNN_WORKSPACE_BYTES;  // per batch of queries

// The model behind a cu2rec_knn handle.
struct DeviceKnn {
    DeviceKnn(const DeviceCsr &train, int weighting, float k1, float b, int neighbours);
    void neighbors(const int *ids, int n, int k, int *out_ids, float *out_sims) const;
    void recommend(const DeviceCsr &history, const DeviceCsr *exclude, const int *users, int n, int k, int *out_items,
                   float *out_scores) const;
    void rank_metrics(const DeviceCsr &history, const DeviceCsr *exclude, const DeviceCsr &test, int k, float threshold,
                      cu2rec_rank_metrics *out, double *per_user) const;
    int items, neighbours, weighting;
    DeviceBuffer<int> ids;     // [items][neighbours]: best first, -1 padding
    DeviceBuffer<float> sims;  // NaN padding
    // the same lists by ascending id, padding last: row i is positions [s_begin[i], s_end[i]) of s_idx / s_val
    DeviceBuffer<int> s_begin, s_end, s_idx;
    DeviceBuffer<float> s_val;
};

// the weights of every stored entry (include/cu2rec_amd.h) into w (device, CSR entry order) and, if not null, into t_w (device,
// the order of the CSR's item-major view, csr_views.hpp); the arguments are checked by the caller
void knn_weights(const DeviceCsr &csr, int weighting, float k1, float b, float *w, float *t_w, hipStream_t stream);
// the argument checks cu2rec_knn_create and cu2rec_csr_knn_weights share; fn names the caller
void knn_check_weighting(const char *fn, int weighting, float k1, float b);

}  // namespace cu2rec

struct cu2rec_knn {
    cu2rec::DeviceKnn impl;
    template <class... A>
    explicit cu2rec_knn(A &&...a) : impl(std::forward<A>(a)...) {}
};
