// ---- phase 1: the inverse factor of every block --------------------------------------------------------------------
// One workgroup of four wavefronts per block.  The 64 user rows are gathered with coalesced 128-byte pieces into LDS
// (odd row stride: a column read is conflict free), 16 rows per wavefront, all of a lane's loads in flight together.
// v_mfma_f32_32x32x2_f32 wants A[i = l & 31][kk = l >> 5] and B[kk = l >> 5][j = l & 31]: lane (k = l & 31, h = l >> 5)
// feeds half h of the columns of row k, so for the two diagonal tiles (B = A^T) the SAME register is both operands.
// The three Gram tiles are FOUR wavefronts' work (one matrix pipe each: the waves of a workgroup sit on SIMD 0-3 in order): wavefronts
// 0-2 contract the leading three quarters of the K range of one tile each, wavefront 3 the last quarter of all three, and the partial
// tiles are added through LDS (gram_split).  With N = lr L in tiles [[N00, 0], [N10, N11]]
// (strictly lower triangular diagonal tiles):
//     M = (I + N)^-1 = [[M11, 0], [M21, M22]],  M11 = (I + N00)^-1,  M22 = (I + N11)^-1,  M21 = -M22 N10 M11.
// The two triangular inversions run side by side in the two lane halves of wavefront 0 (lane = column, forward
// substitution with the N rows broadcast from LDS one row ahead of their use, four partial sums per row); the two
// products for M21 are matrix-core work again, the first one's accumulator tile being the second one's B operand as it
// stands.
#pragma once

#include "blocksolve_device.hpp"
#include "mfma_f32.hpp"

namespace cu2rec {
namespace bs_dev {

constexpr int kGramTabFloats = 2 * kB;  // a^d | c^d, d in [0, 64)
__host__ __device__ inline size_t gram_tile_float4s(int nslots) { return static_cast<size_t>(kB) * (nslots | 1); }

// LDS of a workgroup: [the block's 64 rows, RS float4 apart, later the five 32 x 32 tiles in their place | the powers | the base errors]
// (gram_block); a cross block's workgroup keeps two blocks' rows and nothing else (gram_cross_block)
__host__ __device__ inline int gram_tab_offset(int RS) { return max(4 * kB * RS, 5 * kH * kMS); }  // floats in front of the powers
__host__ __device__ inline size_t gram_lds_bytes(int nslots, bool with_cross_blocks) {
    const size_t own = static_cast<size_t>(gram_tab_offset(nslots | 1) + kGramTabFloats + kB) * sizeof(float);
    const size_t cross = with_cross_blocks ? 2 * gram_tile_float4s(nslots) * sizeof(float4) : 0;
    return own > cross ? own : cross;
}

// The K split of the Gram products: of the S0 = ceil(nslots / 2) float4 slots of each lane half, wavefronts 0-2 take [0, gram_split(S0))
// and wavefront 3 takes the rest, for all three tiles -- 3 Sa = 3 (S0 - Sa) + at most 3.  Whole slots only; up to S0 = 3 wavefront 3's
// range is empty (n_factors <= 24).  f = 100: S0 = 13, 40 dependent MFMAs on each of wavefronts 0-2 and 36 on wavefront 3 instead of 52 on three.
// Measured (ML-20M shape, profiles/r08_phase1_ab.txt): bs_gram_kernel 18.6 -> 17.4 us on average, 17.6 -> 16.0 in the median iteration,
// -1.2 us per benchmark step.  One more barrier and one LDS round trip of three tiles pay for it.
// Registers: the kernel sits exactly at its 128 VGPRs (__launch_bounds__(256, 4)), no scratch; the three accumulator tiles are live in
// every wavefront across the products -- whatever is added to this kernel has to win registers back first.
__host__ __device__ inline int gram_split(int S0) { return (3 * S0 + 3) >> 2; }

// One block of phase 1 (the body of bs_gram_kernel): its rows -> LDS, the Gram tiles, (I + N)^-1, the record.  Workgroup uniform.
__device__ __forceinline__ void gram_block(const SgdArgs &a, const BsIteration &it, int g, float4 *bs_smem) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const BsBlockDesc bd = it.blocks[g];
    if (bd.n_valid == 0) return;  // (the grid is an upper bound of the iteration's blocks)
    const int nslots = a.nslots, RS = nslots | 1;
    // The five 32 x 32 tiles TAKE THE PLACE of the user rows once the Gram products have read them (barrier below): 34.6 instead of
    // 57.6 KB of LDS at f = 128 -- three workgroups a CU instead of two on the Netflix shape, whose 7,500 blocks come in rounds
    float4 *tile = bs_smem;  // [kB][RS]
    float *Ms = reinterpret_cast<float *>(bs_smem);                               // M11 | M22
    float *Ns = Ms + 2 * kH * kMS;                                                // N00 (later M21) | N11 | N10
    float *tab = Ms + gram_tab_offset(RS);
    float *basev = tab + kGramTabFloats;      // [kB] r - gb - ub, 0 past the end of a short block
    const bool mine = lane < bd.n_valid;  // lane l: link l
    const uint64_t val = it.vals[bd.pos0 + min(lane, bd.n_valid - 1)];
    const int x = static_cast<int>(val >> 32);
    if (wave == 3) {
        // what the link's error starts from: r - gb - ub (mf_sequential.cu:119-126 without b and p.q)
        const float r0 = (__uint_as_float(static_cast<uint32_t>(val)) - a.global_bias) - a.user_bias[x];
        basev[lane] = mine ? r0 : 0.f;
        tab[lane] = it.tables[kTabApow + lane];
        tab[kB + lane] = it.tables[kTabCpow + lane];
    }
    // gather: 8 lanes x 16 bytes per row piece, 8 rows per pass, this wavefront's 16 rows.  Every load is unconditional at
    // a clamped address: a predicated load makes the compiler branch around it and wait for each one separately.
    const int rsub = lane >> 3, cs = lane & 7;
    const int nch = (nslots + 7) >> 3;
    for (int c0 = 0; c0 < nch; c0 += 4) {
        float4 v[2][4];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int xr = __shfl(x, 16 * wave + 8 * pp + rsub);
            const float4 *src = reinterpret_cast<const float4 *>(a.P + static_cast<size_t>(xr) * a.ldp);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[pp][c] = src[min(8 * (c0 + c) + cs, nslots - 1)];
        }
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int row = 16 * wave + 8 * pp + rsub;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int slot = 8 * (c0 + c) + cs;
                if (slot < nslots) tile[row * RS + slot] = row < bd.n_valid ? v[pp][c] : zero4();
            }
        }
    }
    __syncthreads();
    const int k = lane & 31, h = lane >> 5;
    const int S0 = (nslots + 1) >> 1;  // slots per lane half
    const int Sa = gram_split(S0);
    f32x16 acc, acc1, acc2;  // (acc1, acc2: wavefront 3's second and third partial tile)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = acc1[i] = acc2[i] = 0.f;
    if (wave < 3) {  // 0: G00 -> N00, 1: G11 -> N11, 2: G10 -> N10 (rows: links 32.., columns: links 0..31); slots [0, Sa) of each lane half
        // D[i][j] = (A row i) . (B row j) lands in lane j = l & 31 at the rows i = acc_row(reg, h) of its registers.  The lane's own
        // link is the tile's ROW here, the registers' index its columns -- for the diagonal tiles by symmetry, for N10 because
        // A = links 0..31 and B = links 32..63: every lane then holds 4 x 4 CONTIGUOUS columns of its row and writes them with four
        // 16-byte LDS stores (round 4; it was sixteen scattered 4-byte stores behind two table reads each: 3.3 us of phase 1)
        const float4 *ra = tile + (wave == 1 ? kH + k : k) * RS, *rb = tile + (wave == 0 ? k : kH + k) * RS;
        for (int c = 0; c < Sa; c += 2) {
            float4 va[2], vb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int slot = h * S0 + c + i;
                const bool ok = c + i < Sa && slot < nslots;
                const float4 t0 = ra[min(slot, nslots - 1)], t1 = rb[min(slot, nslots - 1)];
                va[i] = ok ? t0 : zero4();
                vb[i] = ok ? t1 : zero4();
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float pa[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, pb[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[e], pb[e], acc, 0, 0, 0);
            }
        }
    } else {  // slots [Sa, S0) of each lane half, all three tiles: one read of the two rows feeds three independent accumulators
        const float4 *ra = tile + k * RS, *rb = tile + (kH + k) * RS;
        for (int c = Sa; c < S0; c += 2) {
            float4 va[2], vb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int slot = h * S0 + c + i;
                const bool ok = c + i < S0 && slot < nslots;
                const float4 t0 = ra[min(slot, nslots - 1)], t1 = rb[min(slot, nslots - 1)];
                va[i] = ok ? t0 : zero4();
                vb[i] = ok ? t1 : zero4();
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float pa[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, pb[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[e], pa[e], acc, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pb[e], pb[e], acc1, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[e], pb[e], acc2, 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();  // every wavefront is through with the rows: the tiles take their place
    if (wave == 3) {
        // the partial tiles, each element where the lane of wavefronts 0-2 that owns it will write its N: that lane reads it back and
        // nobody else does
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float *dst = Ns + k * kMS + 4 * h + 8 * m;
            *reinterpret_cast<f32x4 *>(dst) = f32x4{acc[4 * m], acc[4 * m + 1], acc[4 * m + 2], acc[4 * m + 3]};
            *reinterpret_cast<f32x4 *>(dst + kH * kMS) = f32x4{acc1[4 * m], acc1[4 * m + 1], acc1[4 * m + 2], acc1[4 * m + 3]};
            *reinterpret_cast<f32x4 *>(dst + 2 * kH * kMS) = f32x4{acc2[4 * m], acc2[4 * m + 1], acc2[4 * m + 2], acc2[4 * m + 3]};
        }
    }
    __syncthreads();
    if (wave < 3) {
        // N[K][J] = lr (c^d + a^d G[K][J]), d = K - 1 - J (links of the block), for J < K < n_valid; the powers by v_exp_f32 from
        // log2 a, log2 c (they multiply lr-sized terms only: an ulp of the power is 1e-9 of an entry)
        const float lr = a.h.lr;
        const int K = (wave == 0 ? 0 : kH) + k;            // this lane's link: the row
        const int J0 = (wave == 1 ? kH : 0) + 4 * h;       // first column of register 0
        const bool row_ok = K < bd.n_valid;
        float *dst = Ns + (wave * kH + k) * kMS + 4 * h;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const f32x4 part = *reinterpret_cast<const f32x4 *>(dst + 8 * m);  // wavefront 3's share of the sum
            f32x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d = K - 1 - (J0 + 8 * m + e);
                const float fd = static_cast<float>(d);
                const float v = lr * (__builtin_amdgcn_exp2f(fd * it.log2c) + __builtin_amdgcn_exp2f(fd * it.log2a) * (acc[4 * m + e] + part[e]));
                out[e] = d >= 0 && row_ok ? v : 0.f;
            }
            *reinterpret_cast<f32x4 *>(dst + 8 * m) = out;
        }
    }
    __syncthreads();
    // (Tried and removed: each diagonal tile inverted in 16 x 16 quarters, one unit-triangular quarter of 15 steps per wavefront, the
    // quarters below the diagonal and M21 -- one quarter per wavefront -- on v_mfma_f32_16x16x4_f32, 16-byte stores.  128 VGPRs, no
    // scratch, same results; two more barriers, and without the row prefetch below, which spilled 27 registers there.  bs_gram_kernel
    // 17.42 -> 17.50 us on average on top of the four-wavefront products, 18.50 -> 18.42 alone: inside the run-to-run spread either way,
    // the benchmark step unchanged.  profiles/r08_phase1_ab.txt; the code: profiles/r08_gram_quartered_inverse.patch.)
    if (wave == 0) {
    // M11 (lanes 0-31) and M22 (lanes 32-63): lane = column, m[kk] = M[kk][column]
    float m[kH];
    {
        const float *Nh = Ns + h * kH * kMS;
        float4 cur[8], nxt[8];
        m[0] = k == 0 ? 1.f : 0.f;
        cur[0] = *reinterpret_cast<const float4 *>(Nh + kMS);
#pragma unroll
        for (int kk = 1; kk < kH; ++kk) {
            if (kk + 1 < kH) {
#pragma unroll
                for (int i4 = 0; i4 < (kk + 4) / 4; ++i4) nxt[i4] = *reinterpret_cast<const float4 *>(Nh + (kk + 1) * kMS + 4 * i4);
            }
            __builtin_amdgcn_sched_barrier(0);
            float s[4] = {kk == k ? 1.f : 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i4 = 0; i4 < (kk + 3) / 4; ++i4) {
                const float nv[4] = {cur[i4].x, cur[i4].y, cur[i4].z, cur[i4].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * i4 + e < kk) s[e] = __builtin_fmaf(-nv[e], m[4 * i4 + e], s[e]);
            }
            m[kk] = (s[0] + s[1]) + (s[2] + s[3]);
            __builtin_amdgcn_sched_barrier(0);
            if (kk + 1 < kH) {
#pragma unroll
                for (int i4 = 0; i4 < (kk + 4) / 4; ++i4) cur[i4] = nxt[i4];
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < kH; ++kk) Ms[(h * kH + kk) * kMS + k] = m[kk];
    __builtin_amdgcn_wave_barrier();
    // T = N10 M11, then M21 = -M22 T
    f32x16 tacc, macc;
#pragma unroll
    for (int i = 0; i < 16; ++i) tacc[i] = macc[i] = 0.f;
    {
        const float4 *arow = reinterpret_cast<const float4 *>(Ns + (2 * kH + k) * kMS + 16 * h);  // N10[k][16h + s]
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const float4 a4 = arow[t4];
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                tacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], Ms[(16 * h + 4 * t4 + e) * kMS + k], tacc, 0, 0, 0);
        }
        // step s contracts over T's rows acc_row(s, 0) and acc_row(s, 1): exactly what lane half h holds in register s
        const float *mrow = Ms + (kH + k) * kMS + 4 * h;  // M22[k][8 t + 4 h + e] = M22[k][acc_row(4 t + e, h)]
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const float4 a4 = *reinterpret_cast<const float4 *>(mrow + 8 * t4);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) macc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], tacc[4 * t4 + e], macc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) Ns[acc_row(reg, h) * kMS + k] = -macc[reg];  // M21 where N00 was (its last reader is done)
    }  // wave 0
    __syncthreads();
    // The block's record leaves the workgroup: [M11 | M21 | M22 | base], 16 bytes per lane (phase 2 is queued behind this launch:
    // the kernel boundary publishes it).
    float *rec = it.Mbuf + static_cast<size_t>(g) * kBsRecFloats;
    {
        const int t = threadIdx.x, row = t >> 3, c4 = t & 7;
        const float *src[3] = {Ms, Ns, Ms + kH * kMS};
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<f32x4 *>(rec + q * kH * kH + 4 * t) = *reinterpret_cast<const f32x4 *>(src[q] + row * kMS + 4 * c4);
        if (t < kB / 4) *reinterpret_cast<f32x4 *>(rec + kBsFactorFloats + 4 * t) = *reinterpret_cast<const f32x4 *>(basev + 4 * t);
    }
}

// ---- phase 1, look-ahead chains: the cross block N_i = lr L[block i][block i - 1] ---------------------------------------------------
//     N_i[k][j] = lr (c^(63 + k - j) + a^(63 + k - j) (p_(i,k) . p_(i-1,j)))        (tests/test_blocksolve_algebra.py, lookahead_chain)
// One workgroup of four wavefronts, one 32 x 32 tile each.  Both blocks' 128 rows are gathered into LDS the way phase 1 gathers its
// own (coalesced 128-byte pieces, every load unconditional at a clamped address) and the MFMA operands are read from there: with every
// lane reading its two rows straight from memory (the first form) a workgroup took 18 us -- 64 different rows per load instruction.
// Rows of links past the block's end are zero.  LDS: 2 x 64 rows (the launch asks for that much when there are such workgroups).
__device__ __forceinline__ void gram_cross_block(const SgdArgs &a, const BsIteration &it, int g, float4 *smem) {
    const BsBlockDesc bd = it.blocks[g];
    if (bd.n_valid == 0 || bd.m == 0 || !chain_is_lookahead(it, bd.chain, it.chains[bd.chain])) return;  // workgroup uniform
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = lane & 31, h = lane >> 5;
    const int rt = wave >> 1, ct = wave & 1;  // tile: rows 32 rt .. of this block, columns 32 ct .. of the previous one
    const int nslots = a.nslots, RS = nslots | 1, S0 = (nslots + 1) >> 1;
    float4 *tile_c = smem, *tile_p = smem + kB * RS;  // this block's rows | the previous block's
    {
        // lane l: link l of this block and of the one before it (all 64 of those exist)
        const int xc = static_cast<int>(it.vals[bd.pos0 + min(lane, bd.n_valid - 1)] >> 32);
        const int xp = static_cast<int>(it.vals[bd.pos0 - kB + lane] >> 32);
        const int rsub = lane >> 3, cs = lane & 7;
        const int nch = (nslots + 7) >> 3;
        for (int c0 = 0; c0 < nch; c0 += 2) {
            float4 vc[2][2], vp[2][2];
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int src_lane = 16 * wave + 8 * pp + rsub;
                const float4 *sc = reinterpret_cast<const float4 *>(a.P + static_cast<size_t>(__shfl(xc, src_lane)) * a.ldp);
                const float4 *sp = reinterpret_cast<const float4 *>(a.P + static_cast<size_t>(__shfl(xp, src_lane)) * a.ldp);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    vc[pp][c] = sc[min(8 * (c0 + c) + cs, nslots - 1)];
                    vp[pp][c] = sp[min(8 * (c0 + c) + cs, nslots - 1)];
                }
            }
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int row = 16 * wave + 8 * pp + rsub;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int slot = 8 * (c0 + c) + cs;
                    if (slot < nslots) {
                        tile_c[row * RS + slot] = row < bd.n_valid ? vc[pp][c] : zero4();
                        tile_p[row * RS + slot] = vp[pp][c];
                    }
                }
            }
        }
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    {
        const float4 *ra = tile_c + (kH * rt + k) * RS, *rb = tile_p + (kH * ct + k) * RS;
        // (gram_block's contraction loop again, on purpose: as one shared __forceinline__ function the compiler lays this kernel out
        // differently -- this loop's exit block behind it, a compare inverted -- and phase 1 gates both streams of the iteration)
        for (int c = 0; c < S0; c += 2) {
            float4 va[2], vb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int slot = h * S0 + c + i;
                const bool ok = c + i < S0 && slot < nslots;
                const float4 t0 = ra[min(slot, nslots - 1)], t1 = rb[min(slot, nslots - 1)];
                va[i] = ok ? t0 : zero4();
                vb[i] = ok ? t1 : zero4();
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float pa[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, pb[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[e], pb[e], acc, 0, 0, 0);
            }
        }
    }
    const float lr = a.h.lr;
    float *dst = it.Nbuf + static_cast<size_t>(g) * kBsCrossFloats;
    const int j = kH * ct + k;  // this lane's column: link j of the previous block
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = kH * rt + acc_row(reg, h);  // link i of this block
        const float fd = static_cast<float>(kB - 1 + i - j);  // 0 .. 126
        const float v = lr * (__builtin_amdgcn_exp2f(fd * it.log2c) + __builtin_amdgcn_exp2f(fd * it.log2a) * acc[reg]);
        dst[i * kB + j] = i < bd.n_valid ? v : 0.f;
    }
    __syncthreads();  // (the next block of this workgroup's loop writes the tiles again)
}

}  // namespace bs_dev
}  // namespace cu2rec
