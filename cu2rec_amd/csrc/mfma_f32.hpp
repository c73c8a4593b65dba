// The accumulator of v_mfma_f32_32x32x2_f32 (exact f32 products on the matrix cores): one wavefront holds a 32 x 32 tile, every lane
// 16 floats of column lane & 31.  Shared by the score tile (score_tile.hpp) and the block-solve mode's phase 1 (blocksolve_gram.hpp).
#pragma once

#include <hip/hip_runtime.h>

namespace cu2rec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row of the 32x32 accumulator tile held in register `reg` of a lane of half h (column = lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
// its inverse: the register and half that hold `row` of the tile (acc_row(reg, h) == row)
__device__ __forceinline__ void acc_reg_of_row(int row, int &reg, int &h) {
    h = (row >> 2) & 1;
    reg = (row & 3) + 4 * (row >> 3);
}

}  // namespace cu2rec
