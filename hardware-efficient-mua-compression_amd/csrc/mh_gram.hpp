// mh_gram.hpp -- the kernel of mhi_gram (include/muahuff_ingest.h): gram[i][j] (+)= sum over t of a[i][t] * b[j][t] on
// uint8 counts, exact, on the int8 matrix cores (v_mfma_i32_16x16x64_i8).  The tiles, the runs of K slices, the grid and
// which (tile, run) a workgroup owns are mh_gram_layout.hpp's; this file is what runs on them.
//
// A workgroup of 4 waves owns a 128 x 128 tile for one run of columns; wave (wm, wn) owns the 64 x 64 quarter: 4 x 4
// MFMA tiles of 16 x 16, 64 int32 accumulators per lane.  Both operands are row-major with the columns contiguous, so a
// lane's fragment of one MFMA is 16 consecutive bytes of ONE row -- lane l holds row (l & 15), bytes 16 (l >> 4) .. + 16
// of the 64-column step -- and is loaded straight from global memory at any byte address (mh_device.hpp); the re-use of
// a row block by the other waves and tiles comes out of L1 / L2, there is no LDS staging.  A and B take the same columns
// into the same K positions, so their order inside a step does not matter; the C/D map does: register g of lane l is
// (a's row 4 (l >> 4) + g, b's row l & 15) of the 16 x 16 tile.
// The MFMA's operands are signed: z = x XOR 0x80 is x - 128 as int8, and per run of K columns (K a multiple of 64: a
// ragged end is loaded as x = 0)
//     sum x_i x_j = sum z_i z_j + 128 (sum x_i + sum x_j) - 16384 K                               (exact, int64)
// The row sums come from the same loads (v_sad_u8), in the waves with wn == 0 for a and wm == 0 for b.  |z z'| <= 16384,
// so int32 holds 131071 columns and a run is at most 65536: after every run the tile is widened, fixed up and added to
// gram with 64-bit atomics -- integer sums do not depend on the order, the result is the same from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.hpp"
#include "mh_gram_layout.hpp"

namespace mh {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct GramParams {
    const uint8_t *a;
    uint64_t a_row_stride, a_rows;
    const uint8_t *b;
    uint64_t b_row_stride, b_rows, cols;
    uint8_t *gram;
    uint64_t gram_row_stride;
    unsigned long long *sum_a, *sum_b;
    uint32_t symmetric, nta, ntb, run_slices;
    uint64_t tiles, items;
};

// the n <= 16 bytes of a row at src, zero padded: one 16-byte load at any address, or byte by byte at a ragged end, so
// that no byte outside the row's cols is read
__device__ __forceinline__ u32x4 gram_load_end(const uint8_t *src, int64_t n)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n >= 16) {
        v = *reinterpret_cast<const u32x4_u *>(src);
    } else {
        for (int64_t j = 0; j < n; ++j) v[j >> 2] |= (uint32_t)src[j] << (8 * (j & 3));
    }
    return v;
}

__device__ __forceinline__ uint32_t gram_sum16(const u32x4 &v, uint32_t acc)
{
    acc = __builtin_amdgcn_sad_u8(v[0], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v[1], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v[2], 0u, acc);
    return __builtin_amdgcn_sad_u8(v[3], 0u, acc);
}

__device__ __forceinline__ i32x4 gram_signed(const u32x4 &v)
{
    const i32x4 z = {(int)(v[0] ^ 0x80808080u), (int)(v[1] ^ 0x80808080u), (int)(v[2] ^ 0x80808080u), (int)(v[3] ^ 0x80808080u)};
    return z;
}

// one 64-column step of the wave's 64 x 64 quarter: the row sums where this wave owns them, 16 MFMAs
template <bool SUM_A, bool SUM_B>
__device__ __forceinline__ void gram_step(const u32x4 (&av)[4], const u32x4 (&bv)[4], i32x4 (&acc)[4][4], uint32_t (&sa)[4],
                                          uint32_t (&sb)[4])
{
    i32x4 za[4], zb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (SUM_A) sa[m] = gram_sum16(av[m], sa[m]);
        if (SUM_B) sb[m] = gram_sum16(bv[m], sb[m]);
        za[m] = gram_signed(av[m]), zb[m] = gram_signed(bv[m]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(za[m], zb[n], acc[m][n], 0, 0, 0);
}

// the columns [k0, k1) of the quarter; whole steps with the next step's loads in flight, then the ragged end
template <bool SUM_A, bool SUM_B>
__device__ __forceinline__ void gram_run(const uint8_t *(&pa)[4], const uint8_t *(&pb)[4], uint64_t k0, uint64_t k1,
                                         uint32_t q, i32x4 (&acc)[4][4], uint32_t (&sa)[4], uint32_t (&sb)[4])
{
    const uint64_t whole = k0 + (k1 - k0) / kGramStep * kGramStep;
    u32x4 av[4], bv[4];
    if (k0 < whole) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            av[m] = *reinterpret_cast<const u32x4_u *>(pa[m] + k0);
            bv[m] = *reinterpret_cast<const u32x4_u *>(pb[m] + k0);
        }
        for (uint64_t k = k0 + kGramStep; k < whole; k += kGramStep) {
            u32x4 an[4], bn[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                an[m] = *reinterpret_cast<const u32x4_u *>(pa[m] + k);
                bn[m] = *reinterpret_cast<const u32x4_u *>(pb[m] + k);
            }
            gram_step<SUM_A, SUM_B>(av, bv, acc, sa, sb);
#pragma unroll
            for (int m = 0; m < 4; ++m) av[m] = an[m], bv[m] = bn[m];
        }
        gram_step<SUM_A, SUM_B>(av, bv, acc, sa, sb);
    }
    if (whole < k1) {  // pa / pb already point at this lane's 16 bytes of a step: whole + 16 q is its first column
        const int64_t n = (int64_t)(k1 - whole) - 16 * (int64_t)q;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            av[m] = gram_load_end(pa[m] + whole, n);
            bv[m] = gram_load_end(pb[m] + whole, n);
        }
        gram_step<SUM_A, SUM_B>(av, bv, acc, sa, sb);
    }
}

__global__ __launch_bounds__(kGramThreads) void k_gram(const GramParams p)
{
    __shared__ uint32_t s_sum[2][kGramTile];  // the run's row sums of the tile's rows of a and of b
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wm = wave >> 1, wn = wave & 1u;
    const uint32_t r = lane & 15u, q = lane >> 4;
    for (uint64_t item = gram_first_item(blockIdx.x, gridDim.x); item < p.items; item += gridDim.x) {
        const GramItem it = gram_owner(p.symmetric, p.nta, p.ntb, p.tiles, p.run_slices, p.cols, item);
        const uint64_t row_a = (uint64_t)it.ti * kGramTile + wm * 64u + r, row_b = (uint64_t)it.tj * kGramTile + wn * 64u + r;
        const uint8_t *pa[4], *pb[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {  // a row past the end reads the last row instead: its results are not stored
            const uint64_t ia = row_a + 16u * m < p.a_rows ? row_a + 16u * m : p.a_rows - 1;
            const uint64_t ib = row_b + 16u * m < p.b_rows ? row_b + 16u * m : p.b_rows - 1;
            pa[m] = p.a + ia * p.a_row_stride + 16u * q;
            pb[m] = p.b + ib * p.b_row_stride + 16u * q;
        }
        i32x4 acc[4][4];
        uint32_t sa[4] = {0u, 0u, 0u, 0u}, sb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = i32x4{0, 0, 0, 0};
        if (wn == 0 && wm == 0) gram_run<true, true>(pa, pb, it.k0, it.k1, q, acc, sa, sb);
        else if (wn == 0) gram_run<true, false>(pa, pb, it.k0, it.k1, q, acc, sa, sb);
        else if (wm == 0) gram_run<false, true>(pa, pb, it.k0, it.k1, q, acc, sa, sb);
        else gram_run<false, false>(pa, pb, it.k0, it.k1, q, acc, sa, sb);
        // a row's sum is spread over the 4 lanes with the same r
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            sa[m] += __shfl_xor(sa[m], 16), sa[m] += __shfl_xor(sa[m], 32);
            sb[m] += __shfl_xor(sb[m], 16), sb[m] += __shfl_xor(sb[m], 32);
            if (wn == 0 && q == 0) s_sum[0][wm * 64u + 16u * m + r] = sa[m];
            if (wm == 0 && q == 0) s_sum[1][wn * 64u + 16u * m + r] = sb[m];
        }
        __syncthreads();
        const int64_t kpad = (int64_t)((it.k1 - it.k0 + kGramStep - 1) / kGramStep * kGramStep);
        const bool mirror = p.symmetric && it.ti != it.tj;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const uint32_t lj = wn * 64u + 16u * n + r;
                const uint64_t j = (uint64_t)it.tj * kGramTile + lj;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint32_t li = wm * 64u + 16u * m + 4u * q + g;
                    const uint64_t i = (uint64_t)it.ti * kGramTile + li;
                    if (i < p.a_rows && j < p.b_rows) {
                        const int64_t v = (int64_t)acc[m][n][g] + 128 * ((int64_t)s_sum[0][li] + (int64_t)s_sum[1][lj]) - 16384 * kpad;
                        atomicAdd(reinterpret_cast<unsigned long long *>(p.gram + i * p.gram_row_stride) + j, (unsigned long long)v);
                        if (mirror)
                            atomicAdd(reinterpret_cast<unsigned long long *>(p.gram + j * p.gram_row_stride) + i, (unsigned long long)v);
                    }
                }
            }
        // the row sums themselves: from the tile on the diagonal (symmetric), or from the first tile of the row / column
        if (threadIdx.x < kGramTile) {
            const uint64_t i = (uint64_t)it.ti * kGramTile + threadIdx.x, j = (uint64_t)it.tj * kGramTile + threadIdx.x;
            if (p.symmetric) {
                if (it.ti == it.tj && i < p.a_rows) {
                    if (p.sum_a) atomicAdd(p.sum_a + i, (unsigned long long)s_sum[0][threadIdx.x]);
                    if (p.sum_b) atomicAdd(p.sum_b + i, (unsigned long long)s_sum[0][threadIdx.x]);
                }
            } else {
                if (p.sum_a && it.tj == 0 && i < p.a_rows) atomicAdd(p.sum_a + i, (unsigned long long)s_sum[0][threadIdx.x]);
                if (p.sum_b && it.ti == 0 && j < p.b_rows) atomicAdd(p.sum_b + j, (unsigned long long)s_sum[1][threadIdx.x]);
            }
        }
        __syncthreads();  // s_sum is written again by the next item
    }
}

}  // namespace mh
