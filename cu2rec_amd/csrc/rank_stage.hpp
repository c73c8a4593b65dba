// The ranking-metrics stage (include/cu2rec_amd.h: cu2rec_rank_metrics) over top-k lists that are already on the device, whoever
// made them: cu2rec_model_rank_metrics' fused selection (topk.hip) or the item-neighbourhood recommender (knn.hip).  Lists come in
// batches of consecutive rows; one thread per row checks its list against a relevance bitmap of the test row, and a final
// block-wide sum reduces in double (one host synchronisation per call).  Implemented in topk.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "device.hpp"
#include "hip_check.hpp"

namespace cu2rec {

// what a call reports before any row is evaluated: every row skipped, NaN means
cu2rec_rank_metrics empty_rank_metrics(int k, int rows);

struct RankStage {
    // workspace bytes per listed row of a batch (the relevance bitmap and |R_u|), for the caller's batch size
    static size_t bytes_per_row(int cols) { return static_cast<size_t>((cols + 31) / 32) * 4 + sizeof(int); }
    // rows: the rows the means are taken over; cols: the catalogue; batch: the most rows one add() brings
    RankStage(int rows, int cols, int batch, hipStream_t stream);
    // the lists of rows p0 .. p0 + b - 1 (items: [b][k], -1 padding at the end), p0 + b <= test.rows
    void add(const DeviceCsr &test, float threshold, const int *items, int k, int p0, int b);
    // the means over evaluated rows into *out, the per-row values to per_user (host, [rows][5]) if not null; synchronises
    void finish(int k, cu2rec_rank_metrics *out, double *per_user);

    int rows, cols, words;
    hipStream_t stream;
    DeviceBuffer<double> d_per, d_sum;
    DeviceBuffer<unsigned> rel;
    DeviceBuffer<int> n_rel;
};

}  // namespace cu2rec
