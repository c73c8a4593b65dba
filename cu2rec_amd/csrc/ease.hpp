// EASE (include/cu2rec_amd.h: cu2rec_ease_*): the closed-form item x item weights B from the dense inverse of the regularised Gram
// matrix, and the lists scored from them (ease.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

#include "hip_check.hpp"

namespace cu2rec {

struct DeviceCsr;
struct SlimParams;  // slim.hpp

constexpr int kEaseBlock = 64;  // nb: the block order of the factorisation and the inverse (cu2rec_ease_block_items)
constexpr int kEaseMaxItems = CU2REC_EASE_MAX_ITEMS;
constexpr int kEaseMaxK = CU2REC_EASE_MAX_K;
constexpr size_t kEaseWorkspaceBytes = CU2REC_EASE_WORKSPACE_BYTES;  // per batch of queries

// The model behind a cu2rec_ease handle: a dense item x item matrix B and the lists scored from it.  Built by EASE's closed form
// (ease.hip) or by SLIM's coordinate descent (slim.hip); served by the same code either way.
struct DeviceEase {
    DeviceEase(const DeviceCsr &train, float l2);
    DeviceEase(const DeviceCsr &train, const SlimParams &slim, cu2rec_slim_report *report);  // report may be null
    void weights(const int *ids, int n, float *out) const;
    void neighbors(const int *ids, int n, int k, int *out_ids, float *out_vals) const;
    void recommend(const DeviceCsr &history, const DeviceCsr *exclude, const int *users, int n, int k, int *out_items,
                   float *out_scores) const;
    void rank_metrics(const DeviceCsr &history, const DeviceCsr *exclude, const DeviceCsr &test, int k, float threshold,
                      cu2rec_rank_metrics *out, double *per_user) const;
    int items;
    int ld;  // items rounded up to whole blocks: the order and the row stride of B (the padding is an identity block)
    float l2;
    DeviceBuffer<float> B;  // [ld][ld].  EASE: G, then L, then L^-1, then P, then B, each in place of the one before; SLIM: W
};

// the argument check cu2rec_ease_create and cu2rec_csr_ease_gram share; fn names the caller
void ease_check_l2(const char *fn, float l2);
// G, dense with row stride ld >= cols (a multiple of kEaseBlock; rows and columns past cols: the identity), into g (device)
void ease_gram(const DeviceCsr &csr, float l2, int ld, float *g, hipStream_t stream);
// items rounded up to whole blocks of kEaseBlock
int ease_padded(int items);
// hipMalloc of n floats into buf; memory that is not there is CU2REC_ENOMEM, reported in fn's name
void ease_allocate_matrix(DeviceBuffer<float> &buf, size_t n, const char *fn);

}  // namespace cu2rec

struct cu2rec_ease {
    cu2rec::DeviceEase impl;
    template <class... A>
    explicit cu2rec_ease(A &&...a) : impl(std::forward<A>(a)...) {}
};
