// Expected number of SGD updates per iteration that the rows of a CSR make on each item: rate[y] = sum over the users u
// that rated y of 1 / degree(u) (each user samples uniformly among its ratings).  One computation for
// cu2rec_item_update_rates and the sharded driver's merge weights (shard_driver.hpp): double, users ascending, each row in
// CSR order, so both give the same bits.  Header-only, because tests/host_shard builds the driver with g++ and no HIP.
#pragma once

#include <algorithm>

#include "common.hpp"

namespace cu2rec {

inline void item_update_rates(const int *indptr, const int *indices, int n_rows, int n_cols, double *rate) {
    std::fill(rate, rate + n_cols, 0.0);
    for (int u = 0; u < n_rows; ++u) {
        const int lo = indptr[u], hi = indptr[u + 1];
        if (hi <= lo) continue;
        require(indices != nullptr, "indices is null");
        const double w = 1.0 / (hi - lo);
        for (int k = lo; k < hi; ++k) {
            require(indices[k] >= 0 && indices[k] < n_cols, "item id out of range");
            rate[indices[k]] += w;
        }
    }
}

}  // namespace cu2rec
