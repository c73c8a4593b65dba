// The views derived from a rating matrix, owned by its cu2rec_csr (DeviceCsr::views) and shared by every trainer and recommender that
// reads them: the item-major view (ALS and iALS, logistic MF, BPR's item half-step, ItemKNN), the row-sorted view (BPR's membership
// test, ItemKNN's products) and the row of every entry (BPR, the item-major build).  Each is built on the device the first time it is
// asked for and then kept; the accessors below are the only code that touches the buffers' lifetime (csr_views.hip).  A build may
// synchronise the stream once, before its temporaries are freed; a later call returns what is there.
#pragma once

#include <hip/hip_runtime.h>

#include "hip_check.hpp"

namespace cu2rec {

struct DeviceCsr;

// The transpose: item i's entries are positions [indptr[i], indptr[i + 1]).  A stable radix sort of the entry positions by column:
// rows ascend within an item, and entries that repeat a column within a row stay in CSR order.
struct ItemMajorView {
    DeviceBuffer<int> indptr;   // [cols + 1]
    DeviceBuffer<int> indices;  // [nnz]: the row of each entry
    DeviceBuffer<float> data;   // [nnz]
    DeviceBuffer<int> pos;      // [nnz]: item-major position -> the entry's position in the CSR (the sort's own values, kept)
    bool built = false;
};

// Every row's columns ascending (a stable segmented radix sort).  The positions and values cost 8 bytes per entry and are made only
// for a caller that asks for them: BPR reads idx alone.
struct RowSortedView {
    DeviceBuffer<int> idx;    // [nnz]: the sorted columns
    DeviceBuffer<int> pos;    // [nnz]: the CSR position of each, ascending among equal columns
    DeviceBuffer<float> val;  // [nnz]: data[pos]
    bool has_duplicate = false;  // some row stores a column twice (seen on idx)
    bool built = false, has_values = false;
};

struct CsrViews {
    ItemMajorView items;
    RowSortedView sorted;
    DeviceBuffer<int> row_of;  // [nnz]: the row of every CSR entry
    bool row_of_built = false;
};

// An empty matrix (nnz, rows or cols of 0) gives a zeroed indptr and one-element allocations.
const ItemMajorView &item_major_view(const DeviceCsr &m, hipStream_t stream);
const RowSortedView &row_sorted_view(const DeviceCsr &m, bool with_values, hipStream_t stream);
const int *row_of_view(const DeviceCsr &m, hipStream_t stream);

}  // namespace cu2rec
