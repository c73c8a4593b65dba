// The nb x nb tile of the dense item x item kernels (ease.hip, slim.hip): nb = kEaseBlock = 64, a tile product as 2 x 2 accumulators
// of v_mfma_f32_32x32x2_f32, one per wavefront of a 256-thread workgroup.  Every matrix these kernels see is padded to whole tiles,
// so nothing here checks a bound.
#pragma once

#include <hip/hip_runtime.h>

#include "ease.hpp"
#include "mfma_f32.hpp"

namespace cu2rec {

constexpr int kNb = kEaseBlock;
constexpr int kLs = kNb + 1;  // row stride of a tile in LDS: odd, so that a column read is conflict free
static_assert(kNb == 64, "a tile is 2 x 2 MFMA accumulators, one per wavefront of a 256-thread workgroup; a row or column per lane");

__device__ __forceinline__ float *tile_at(float *g, int ld, int bi, int bj) {
    return g + static_cast<size_t>(bi) * kNb * ld + static_cast<size_t>(bj) * kNb;
}

// tile (row stride ld) -> t[kNb][kLs], by all `threads` threads of the workgroup; coalesced rows
__device__ __forceinline__ void load_tile(float (*t)[kLs], const float *src, size_t ld, int threads) {
    for (int x = threadIdx.x; x < kNb * kNb; x += threads) t[x >> 6][x & 63] = src[static_cast<size_t>(x >> 6) * ld + (x & 63)];
}

// this wavefront's 32 x 32 quarter (wi, wj) of a tile: acc += X Y, the operands in LDS.  Every caller starts a tile product from
// zero_tile() and adds or subtracts the finished product with one rounding per element: a sum over many tiles is then a sum of
// tile-sized parts, whose error grows with the number of tiles and not with the number of terms.  XT: X is read transposed
// (X[i][k] = x[k][i]); NEG: -X.  Y[k][j] = y[k][j] (YT false) or y[j][k] (YT true).  The contraction runs k = 0 .. kNb - 1 in
// ascending pairs.
template <bool XT, bool YT, bool NEG>
__device__ __forceinline__ void tile_mma(f32x16 &acc, const float (*x)[kLs], const float (*y)[kLs], int wi, int wj, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll 8
    for (int k = 0; k < kNb; k += 2) {
        float av = XT ? x[k + h][wi * 32 + r] : x[wi * 32 + r][k + h];
        const float bv = YT ? y[wj * 32 + r][k + h] : y[k + h][wj * 32 + r];
        if (NEG) av = -av;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
}

__device__ __forceinline__ f32x16 zero_tile() {
    f32x16 z;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) z[reg] = 0.f;
    return z;
}

__device__ __forceinline__ void store_quarter(const f32x16 &acc, float *dst, size_t ld, int wi, int wj, int lane) {
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) dst[static_cast<size_t>(wi * 32 + acc_row(reg, h)) * ld + wj * 32 + c] = acc[reg];
}

}  // namespace cu2rec
