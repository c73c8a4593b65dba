// PureSVD (include/cu2rec_amd.h: cu2rec_model_svd): the rank-f dominant subspace of the rating matrix by block subspace iteration,
//   each sweep:  Y = orth(X Q)   Q = orth(X^T Y)      at the end:  P = X Q
// built from two stages (svd.hip): a sparse x dense-skinny product over either view of the CSR, and CholeskyQR2 of a tall, skinny
// matrix.
#pragma once

#include <hip/hip_runtime.h>

#include "als.hpp"
#include "hip_check.hpp"

namespace cu2rec {

struct DeviceCsr;

// out[row, 0 : f] = sum over the row's entries of data * D[idx, 0 : f], for every row of `side` (the CSR itself, or its item-major
// view: device.hpp's als_side, whose row plan cuts the rows longer than kAlsChunk; their chunks' partial rows go through c.workspace
// and are added in chunk order).  D and out have row strides ldd and ldo, multiples of 4 and >= f rounded up to 4; D's columns past f
// are never read as data, out's are written as zero; a row without entries gives a zero row.  1 <= f <= kAlsMaxFactors.
void svd_multiply(AlsCache &c, const AlsSide &side, const float *D, int ldd, float *out, int ldo, int f, hipStream_t stream);

// What svd_orthonormalize keeps between its calls: the dense Gram, the dense inverse factor and the status word.
struct SvdOrthScratch {
    DeviceBuffer<float> gram, dense, inverse;
    DeviceBuffer<int> status;
};

// Y (n rows of stride ld, a multiple of 4 and >= f rounded up to 4) <- its orthonormal basis, in place, by two passes of Cholesky-QR:
// G = Y^T Y (als_global_gram), G = L L^T and L^-1 by one workgroup, Y <- Y L^-T on the matrix cores.  Returns -1, or the column whose
// pivot was not a finite number above 2^-22 of its diagonal entry: Y is then partly transformed and the caller drops it.  The host
// reads the status word once per pass: two stream synchronisations per call.
int svd_orthonormalize(AlsCache &c, SvdOrthScratch &s, float *Y, int ld, int n, int f, hipStream_t stream);

// sum of squares of the first f floats of n rows of stride ld, in double, in a fixed order (synchronises the stream)
double svd_sum_squares(const float *x, int n, int f, int ld, hipStream_t stream);
// |X|_F^2 of the matrix a CSR stores, entries that repeat a column within a row summed first (synchronises the stream)
double svd_total(const DeviceCsr &csr, hipStream_t stream);

}  // namespace cu2rec
