// Alternating least squares (include/cu2rec_amd.h: cu2rec_model_als): one exact half-step solves every row of one side of
// the model against the other side, frozen.  For a row with n ratings, Z is the n x (f + 2) matrix of its gathered partner
// rows [x_i, 1, t_i] (t_i = r - gb - partner bias); the augmented Gram Z^T Z is formed on the matrix cores and the row's
// (f + 1)-order system is solved by Cholesky in LDS (als.hip).  The implicit-feedback half-step (cu2rec_model_als_implicit) runs on the
// same kernels: every partner row enters through G0 = X^T X, a row's entries add sum w x x^T, and the system has order f.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "hip_check.hpp"

namespace cu2rec {

// Length thresholds (include/cu2rec_amd.h mirrors them as CU2REC_ALS_*; the tests read them there).  A row's ratings are
// staged kAlsStep at a time; a row of at most kAlsChunk ratings is gathered, reduced and solved by ONE workgroup; a longer row
// is cut into ceil(n / kAlsChunk) chunks -- at most kAlsMaxChunks, beyond which the chunks grow instead, in whole steps --
// whose partial Grams are summed in chunk order.  Either way the order of every sum is a function of n alone.
constexpr int kAlsStep = CU2REC_ALS_STEP;                // 32
constexpr int kAlsChunk = CU2REC_ALS_CHUNK;              // 1024
constexpr int kAlsMaxChunks = CU2REC_ALS_MAX_CHUNKS;     // 64
constexpr size_t kAlsWorkspaceBytes = CU2REC_ALS_WORKSPACE_BYTES;  // 64 MiB of partial Grams at once: the workspace bound
constexpr int kAlsMaxFactors = CU2REC_ALS_MAX_FACTORS;   // 252: system order f + 1 <= 253, the packed factor fits one workgroup's LDS

// What a kernel template is compiled for: the explicit half-step ([x | 1 | t] staged once, order f + 1), the implicit one (two
// operands, seeded from G0, order f), or a tile of the global Gram G0 itself ([x | 0] gathered by row number).  The
// conjugate-gradient kernel (als_cg.hip) is compiled for the first two.
enum class AlsKind { Explicit, Implicit, Gram };

__host__ __device__ inline int als_chunks(int n) {
    const int c = (n + kAlsChunk - 1) / kAlsChunk;
    return c < kAlsMaxChunks ? c : kAlsMaxChunks;
}
__host__ __device__ inline int als_chunk_len(int n) {  // ratings per chunk (the last one may be shorter)
    const int c = als_chunks(n);
    const int per = (n + c - 1) / c;
    return (per + kAlsStep - 1) / kAlsStep * kAlsStep;
}

// One side's rows as the half-step reads them -- the CSR itself for the users, its item-major view (csr_views.hpp) for the items --
// plus the row plan: the host list of the side's long rows, cut into chunks.
struct AlsSide {
    const int *indptr = nullptr, *indices = nullptr;
    const float *data = nullptr;
    int rows = 0;
    bool planned = false;  // als_plan_side has filled what follows
    int rows_with_ratings = 0;
    std::vector<int> long_rows, long_first_chunk;  // long_first_chunk[r + 1] - long_first_chunk[r]: chunks of long row r
    DeviceBuffer<int> d_long_rows, d_long_first_chunk, d_chunk_lo, d_chunk_hi;
};

// Cached on a cu2rec_csr: what is ALS's own, the two row plans and the half-steps' workspaces.
struct AlsCache {
    AlsSide users, items;
    DeviceBuffer<float> workspace;  // the partial Grams of one batch of long rows, kAlsWorkspaceBytes at most
    DeviceBuffer<int> unsolved;
    // implicit feedback: X^T X of the partner side (and of the other side, for the objective) in the accumulator layout
    // [tile pair][16][64] of als.hip, rebuilt by every call that reads it; the objective pass's per-block partial sums
    DeviceBuffer<float> g0, g0_other;
    DeviceBuffer<float> g0_dense;  // the conjugate-gradient half-step's G0: dense [f][f rounded up to 4], unpacked from g0 (als_cg.hip)
    DeviceBuffer<double> objective;
};

struct AlsProblem {
    const float *X;   // partner rows (stride ldx) and biases
    int ldx;
    const float *xb;
    float *Y;         // solved rows (stride ldy) and biases
    int ldy;
    float *yb;
    int n_factors;
    float global_bias, reg, reg_bias;
    float alpha = 0.f;  // implicit half-step only: an entry's weight is alpha * r; the partner rows are [0, x_rows)
    int x_rows = 0;
};

// the implicit objective (include/cu2rec_amd.h: cu2rec_model_implicit_objective) over the user-major CSR and rows [0, rows) of P,
// [0, cols) of Q
struct AlsObjectiveProblem {
    const int *indptr, *indices;
    const float *data;
    int rows, cols, nnz;
    const float *P;
    int ldp;
    const float *Q;
    int ldq;
    int n_factors;
    float alpha, P_reg, Q_reg;
};

__host__ __device__ inline int tri(int i) { return i * (i + 1) / 2; }  // tile pairs ti >= tj of the lower triangle: pair tri(ti) + tj

// 32-column tiles of the implicit half-step's staged operands: f factor columns and the right-hand side's weight
inline int ials_tiles(int n_factors) { return (n_factors + 1 + 31) / 32; }

// fills side.long_rows / chunk lists from the device indptr of a side whose pointers and shape are set (once per side)
void als_plan_side(AlsSide &side, hipStream_t stream);
// one half-step over every row of `side` (rows < max_rows); returns the number of rows left unchanged by a failed pivot
// cg_steps > 0 (cu2rec_model_als_cg): the rows of 1 .. kAlsChunk ratings take cg_steps conjugate-gradient steps from their current
// [factors; bias] instead (als_cg_short_rows); the longer rows are solved exactly by the same kernels, to the same bits, either way
int als_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream, int cg_steps = 0);
// als_cg.hip: every row of `side` (rows < max_rows) of 1 .. kAlsChunk ratings: cg_steps steps of CG on its order-(f + 1) system
//   A v = sum_i z_i (z_i . v) + n diag(reg, ..., reg, reg_bias) v,   b = sum_i t_i z_i,   z_i = [x_i; 1]
// applied as an operator, from x0 = [the row's factors; its bias].  Rows without ratings and longer rows are not touched.  A row whose
// iteration meets a non-finite or negative curvature, or ends non-finite, keeps its bits and is counted in c.unsolved (allocated and
// zeroed by the caller)
void als_cg_short_rows(AlsCache &c, const AlsSide &side, const AlsProblem &p, int max_rows, int cg_steps, hipStream_t stream);
// the implicit-feedback half-step: G0 = X^T X over partner rows [0, p.x_rows), then every row of `side` -- rows without entries become
// zero rows; p.global_bias, p.reg_bias and p.xb are not read, the solved biases are written as 0.  Returns als_half_step's count.
// cg_steps > 0: the rows of 1 .. kAlsChunk entries take cg_steps conjugate-gradient steps from their current factors instead
// (ials_cg_short_rows); the longer rows are solved exactly by the same kernels, to the same bits, either way
int ials_half_step(AlsCache &c, AlsSide &side, const AlsProblem &p, int max_rows, hipStream_t stream, int cg_steps = 0);
// als_cg.hip: c.g0 (formed by the caller on `stream`) unpacked into c.g0_dense, then every row of `side` (rows < max_rows) of at
// most kAlsChunk entries: cg_steps steps of CG on its order-f system applied as an operator; rows without entries become zero
// rows, longer rows are not touched.  A row whose iteration meets a non-finite or negative curvature, or ends non-finite, keeps
// its bits and is counted in c.unsolved (allocated and zeroed by the caller)
void ials_cg_short_rows(AlsCache &c, const AlsSide &side, const AlsProblem &p, int max_rows, int cg_steps, hipStream_t stream);
// out = X^T X over rows [0, n) of X (row stride ldx, a multiple of 4 and >= f rounded up to 4; the columns past f are never read as data)
// in the accumulator layout [tile pair][16][64] of ceil(f / 32) tiles: the implicit half-step's G0 kernels, for a caller that wants the
// Gram alone (svd.hip).  The rows go in tiles of kAlsChunk through c.workspace, the tiles' partial Grams are added in tile order
void als_global_gram(AlsCache &c, const float *X, int ldx, int n, int f, DeviceBuffer<float> &out, hipStream_t stream);
// als_cg.hip: a Gram in that layout -> dense [f][S], symmetric, the columns f .. S - 1 zero
void als_unpack_gram(const float *acc, float *dense, int f, int S, hipStream_t stream);
// the implicit objective L (two global Grams, one pass over the entries and both sides' rows in double); synchronises the stream
double ials_objective(AlsCache &c, const AlsObjectiveProblem &o, hipStream_t stream);

}  // namespace cu2rec
