// The score tile shared by cu2rec_model_scores / cu2rec_model_recommend (predict.hip) and cu2rec_model_topk (topk.hip): one
// wavefront accumulates a 32 users x 32 items block of p_u . q_i on the matrix cores (v_mfma_f32_32x32x2_f32).  Both callers
// contract through the same functions with the same chunking, so a (user, item) score is the same float in both.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "mfma_f32.hpp"

namespace cu2rec {

constexpr int kTile = 32;
constexpr size_t kMaxLds = 160 * 1024;  // LDS of one workgroup on gfx950

// 32 rows x slots [slot0, slot0 + n) of a row-major matrix into an LDS tile [32][RS], by one wavefront: 8 lanes x 16 bytes
// per row piece, 8 rows per pass; rows beyond n_rows are zero.  Loads are unconditional at clamped addresses.
__device__ __forceinline__ void stage_rows(float4 *tile, const float *__restrict__ base, int ld, int first_row, int n_rows,
                                           int slot0, int n, int RS, int lane) {
    const int rsub = lane >> 3, cs = lane & 7;
    const int nch = (n + 7) >> 3;
    for (int c = 0; c < nch; ++c) {
        float4 v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = min(first_row + 8 * p + rsub, n_rows - 1);
            v[p] = reinterpret_cast<const float4 *>(base + static_cast<size_t>(row) * ld)[slot0 + min(8 * c + cs, n - 1)];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int slot = 8 * c + cs;
            if (slot < n) tile[(8 * p + rsub) * RS + slot] = first_row + 8 * p + rsub < n_rows ? v[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// acc += U[32 x 4n] * I[32 x 4n]^T over the n slots staged in utile / itile
__device__ __forceinline__ void contract(f32x16 &acc, const float4 *utile, const float4 *itile, int RS, int n, int r, int h) {
    const int S0 = (n + 1) >> 1;
    for (int c = 0; c < S0; c += 2) {
        float4 a4[2], b4[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int slot = h * S0 + c + i;
            const bool ok = c + i < S0 && slot < n;
            const float4 ua = utile[r * RS + min(slot, n - 1)], ib = itile[r * RS + min(slot, n - 1)];
            a4[i] = ok ? ua : make_float4(0.f, 0.f, 0.f, 0.f);
            b4[i] = ok ? ib : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i].x, b4[i].x, acc, 0, 0, 0);  // rows: users, columns: items
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i].y, b4[i].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i].z, b4[i].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i].w, b4[i].w, acc, 0, 0, 0);
        }
    }
}

}  // namespace cu2rec
