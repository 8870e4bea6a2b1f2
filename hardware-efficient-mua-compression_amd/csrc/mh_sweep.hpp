// mh_sweep.hpp -- the kernels of mhq_gram_clips and mhq_xty_clips (include/muahuff_sweep.h).  The items, the runs and
// the grids are mh_sweep_layout.hpp's; DESIGN.md section 4 has the reasoning.
//
// k_gram_clips: what k_gram (mh_gram.hpp) does on a 128 x 128 tile for one run of columns -- four waves, each a 64 x 64
// quarter of 4 x 4 MFMA tiles (v_mfma_i32_16x16x64_i8), fragments of 16 consecutive bytes of one row loaded straight from
// global memory at any byte address, the operands z = x XOR 0x80 with the row-sum fix-up
//     sum x_i x_j = sum z_i z_j + 128 (sum x_i + sum x_j) - 16384 K
// -- with three differences.  The b operand is the same matrix d bytes earlier (the lag difference of the item); every
// fragment is clamped to the item's clip in registers right after its load, so the row sums of the fix-up are those of
// the clamped bytes; and the range, the clip and d come out of the item number, so one launch covers all of them.
// The clamp: gfx950 has no packed byte minimum.  The even bytes of a dword are masked out and go through one
// v_pk_min_u16 against (q, q); the odd bytes stay where they are and the whole dword goes through a second one against
// (256 q + 255, 256 q + 255), which leaves min(byte, q) in the high byte of either 16-bit lane whatever the low byte is;
// the halves are put together under the mask 0xff00ff00.  As compiled: v_and, two v_pk_min_u16 and v_and_or -- four VALU
// instructions a dword -- where the clip is at most 127 (kSweepDirectClip): the clamped bytes are then their own int8
// operands, so the DIRECT form has no XOR and no fix-up -- 127^2 * 65536 < 2^31 keeps the run inside int32 -- and sums
// rows only on the diagonal tile of d = 0, where they are a result.  Above 127 the XOR form: v_and, two v_pk_min_u16,
// v_and and one v_bitop3 that puts together and flips the sign bits, five a dword.
//
// k_xty_clips<K>: the body of k_xty (mh_wiener.hpp) over (run of a range, clip, channel) items: the same columns per
// thread, the same FMA chain, the same butterfly and the same order of the four waves, so an item's partial sums are the
// bits mhw_xty computes for that range and clip alone.  k_xty_clips_sum adds an element's runs in run order and stores
// once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.hpp"
#include "mh_sweep_layout.hpp"

namespace mh {

typedef int sw_i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short sw_u16x2 __attribute__((ext_vector_type(2)));

struct GramClipsParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows, lags, n_clips, nt;
    uint64_t tiles0, tiles1, dt, items;
    unsigned long long *gram;  // [n_ranges][n_clips][lags][rows][rows]
    unsigned long long *sums;  // [n_ranges][n_clips][rows]
    SweepRanges ranges;
    SweepClips clips;
};

// the clip q as the two operands of the packed minima: (q, q) and (256 q + 255, 256 q + 255)
struct ClipPair {
    sw_u16x2 even, odd;
};

__device__ __forceinline__ ClipPair sweep_clip_pair(uint32_t q)
{
    ClipPair c;
    c.even = sw_u16x2{(unsigned short)q, (unsigned short)q};
    c.odd = sw_u16x2{(unsigned short)(256u * q + 255u), (unsigned short)(256u * q + 255u)};
    return c;
}

// min(byte, q) on the four bytes of a dword.  The odd bytes stay where they are: a 16-bit lane 256 b + a against
// 256 q + 255 keeps b where b <= q and gives q where b > q in its high byte, whatever a is; its low byte is dropped.
__device__ __forceinline__ uint32_t sweep_clamp4(uint32_t v, const ClipPair &c)
{
    const sw_u16x2 e = __builtin_elementwise_min(__builtin_bit_cast(sw_u16x2, v & 0x00ff00ffu), c.even);
    const sw_u16x2 o = __builtin_elementwise_min(__builtin_bit_cast(sw_u16x2, v), c.odd);
    return (__builtin_bit_cast(uint32_t, o) & 0xff00ff00u) | __builtin_bit_cast(uint32_t, e);
}

__device__ __forceinline__ u32x4 sweep_clamp16(const u32x4 &v, const ClipPair &c)
{
    const u32x4 r = {sweep_clamp4(v[0], c), sweep_clamp4(v[1], c), sweep_clamp4(v[2], c), sweep_clamp4(v[3], c)};
    return r;
}

// the n <= 16 bytes of a row at src, zero padded: one 16-byte load at any address, or byte by byte at a ragged end, so
// that no byte outside the run's columns is read
__device__ __forceinline__ u32x4 sweep_load_end(const uint8_t *src, int64_t n)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n >= 16) {
        v = *reinterpret_cast<const u32x4_u *>(src);
    } else {
        for (int64_t j = 0; j < n; ++j) v[j >> 2] |= (uint32_t)src[j] << (8 * (j & 3));
    }
    return v;
}

__device__ __forceinline__ uint32_t sweep_sum16(const u32x4 &v, uint32_t acc)
{
    acc = __builtin_amdgcn_sad_u8(v[0], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v[1], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v[2], 0u, acc);
    return __builtin_amdgcn_sad_u8(v[3], 0u, acc);
}

__device__ __forceinline__ sw_i32x4 sweep_signed(const u32x4 &v)
{
    const sw_i32x4 z = {(int)(v[0] ^ 0x80808080u), (int)(v[1] ^ 0x80808080u), (int)(v[2] ^ 0x80808080u), (int)(v[3] ^ 0x80808080u)};
    return z;
}

// one 64-column step of the wave's 64 x 64 quarter: the clamp, the row sums where this wave owns them, 16 MFMAs.
// DIRECT: the clip is at most 127, the clamped bytes are their own int8 operands
template <bool DIRECT, bool SUM_A, bool SUM_B>
__device__ __forceinline__ void sweep_step(const u32x4 (&av)[4], const u32x4 (&bv)[4], const ClipPair &c, sw_i32x4 (&acc)[4][4],
                                           uint32_t (&sa)[4], uint32_t (&sb)[4])
{
    sw_i32x4 za[4], zb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const u32x4 ca = sweep_clamp16(av[m], c), cb = sweep_clamp16(bv[m], c);
        if (SUM_A) sa[m] = sweep_sum16(ca, sa[m]);
        if (SUM_B) sb[m] = sweep_sum16(cb, sb[m]);
        za[m] = DIRECT ? __builtin_bit_cast(sw_i32x4, ca) : sweep_signed(ca);
        zb[m] = DIRECT ? __builtin_bit_cast(sw_i32x4, cb) : sweep_signed(cb);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(za[m], zb[n], acc[m][n], 0, 0, 0);
}

// the columns [k0, k1) of the quarter; whole steps with the next step's loads in flight, then the ragged end
template <bool DIRECT, bool SUM_A, bool SUM_B>
__device__ __forceinline__ void sweep_run(const uint8_t *(&pa)[4], const uint8_t *(&pb)[4], uint64_t k0, uint64_t k1, uint32_t q,
                                          const ClipPair &c, sw_i32x4 (&acc)[4][4], uint32_t (&sa)[4], uint32_t (&sb)[4])
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
            sweep_step<DIRECT, SUM_A, SUM_B>(av, bv, c, acc, sa, sb);
#pragma unroll
            for (int m = 0; m < 4; ++m) av[m] = an[m], bv[m] = bn[m];
        }
        sweep_step<DIRECT, SUM_A, SUM_B>(av, bv, c, acc, sa, sb);
    }
    if (whole < k1) {  // pa / pb already point at this lane's 16 bytes of a step: whole + 16 q is its first column
        const int64_t n = (int64_t)(k1 - whole) - 16 * (int64_t)q;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            av[m] = sweep_load_end(pa[m] + whole, n);
            bv[m] = sweep_load_end(pb[m] + whole, n);
        }
        sweep_step<DIRECT, SUM_A, SUM_B>(av, bv, c, acc, sa, sb);
    }
}

__global__ __launch_bounds__(kGramThreads) void k_gram_clips(const GramClipsParams p)
{
    __shared__ uint32_t s_sum[2][kGramTile];  // the run's row sums of the tile's clamped rows, as a and as b
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wm = wave >> 1, wn = wave & 1u;
    const uint32_t r = lane & 15u, q = lane >> 4;
    for (uint64_t item = gram_first_item(blockIdx.x, gridDim.x); item < p.items; item += gridDim.x) {
        const GramClipsItem it = gram_clips_owner(p.ranges, p.n_clips, p.nt, p.tiles0, p.tiles1, p.dt, item);
        const uint32_t clip = p.clips.q[it.n];
        const ClipPair c = sweep_clip_pair(clip);
        const bool direct = clip <= kSweepDirectClip, diag = it.d == 0 && it.ti == it.tj;
        const uint64_t row_a = (uint64_t)it.ti * kGramTile + wm * 64u + r, row_b = (uint64_t)it.tj * kGramTile + wn * 64u + r;
        const uint8_t *pa[4], *pb[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {  // a row past the end reads the last row instead: its results are not stored
            const uint64_t ia = row_a + 16u * m < p.rows ? row_a + 16u * m : p.rows - 1;
            const uint64_t ib = row_b + 16u * m < p.rows ? row_b + 16u * m : p.rows - 1;
            pa[m] = p.x + ia * p.x_row_stride + 16u * q;
            pb[m] = p.x + ib * p.x_row_stride + 16u * q - it.d;  // column u - d: k0 - d >= first[0] - (lags - 1) >= 0
        }
        sw_i32x4 acc[4][4];
        uint32_t sa[4] = {0u, 0u, 0u, 0u}, sb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = sw_i32x4{0, 0, 0, 0};
        if (direct) {  // no fix-up: the row sums are wanted only where they are a result, on the diagonal tile of d = 0
            if (wn == 0 && diag) sweep_run<true, true, false>(pa, pb, it.k0, it.k1, q, c, acc, sa, sb);
            else sweep_run<true, false, false>(pa, pb, it.k0, it.k1, q, c, acc, sa, sb);
        } else {
            if (wn == 0 && wm == 0) sweep_run<false, true, true>(pa, pb, it.k0, it.k1, q, c, acc, sa, sb);
            else if (wn == 0) sweep_run<false, true, false>(pa, pb, it.k0, it.k1, q, c, acc, sa, sb);
            else if (wm == 0) sweep_run<false, false, true>(pa, pb, it.k0, it.k1, q, c, acc, sa, sb);
            else sweep_run<false, false, false>(pa, pb, it.k0, it.k1, q, c, acc, sa, sb);
        }
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
        const bool mirror = it.d == 0 && it.ti != it.tj;
        const uint64_t rn = (uint64_t)it.r * p.n_clips + it.n;
        unsigned long long *const g = p.gram + (rn * p.lags + it.d) * p.rows * p.rows;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const uint32_t lj = wn * 64u + 16u * n + r;
                const uint64_t j = (uint64_t)it.tj * kGramTile + lj;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t li = wm * 64u + 16u * m + 4u * q + e;
                    const uint64_t i = (uint64_t)it.ti * kGramTile + li;
                    if (i < p.rows && j < p.rows) {
                        const int64_t fix = direct ? 0 : 128 * ((int64_t)s_sum[0][li] + (int64_t)s_sum[1][lj]) - 16384 * kpad;
                        const int64_t v = (int64_t)acc[m][n][e] + fix;
                        atomicAdd(g + i * p.rows + j, (unsigned long long)v);
                        if (mirror) atomicAdd(g + j * p.rows + i, (unsigned long long)v);
                    }
                }
            }
        // the row sums themselves: from the tile on the diagonal at d = 0
        if (diag && threadIdx.x < kGramTile) {
            const uint64_t i = (uint64_t)it.ti * kGramTile + threadIdx.x;
            if (i < p.rows) atomicAdd(p.sums + rn * p.rows + i, (unsigned long long)s_sum[0][threadIdx.x]);
        }
        __syncthreads();  // s_sum is written again by the next item
    }
}

struct XtyClipsParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows, lags, lead, n_clips;
    const uint8_t *y;  // float rows, y_row_stride bytes apart
    uint64_t y_row_stride;
    double *scratch;
    uint64_t items;
    SweepRanges ranges;
    SweepClips clips;
};

template <int K>
__global__ __launch_bounds__(kXtyThreads) void k_xty_clips(const XtyClipsParams p)
{
    constexpr int LB = (int)kXtyLagBlock;
    __shared__ double red[kXtyThreads / 64][LB * K];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const XtyClipsItem it = xty_clips_owner(p.ranges, p.n_clips, p.rows, item);
        const uint32_t clip = p.clips.q[it.n];
        // column t of the range is column first - (lags - 1) + t of mhw_xty's x and column first + lead + t of its y
        const uint8_t *const xr = p.x + (uint64_t)it.c * p.x_row_stride + (p.ranges.first[it.r] - (p.lags - 1));
        const uint8_t *const yr = p.y + 4 * (p.ranges.first[it.r] + p.lead);
        double *const dst = p.scratch + item * (uint64_t)(p.lags * K);
        for (uint32_t l0 = 0; l0 < p.lags; l0 += LB) {
            // lag l0 + i reads column t + lags - 1 - (l0 + i); an i past the last lag repeats it (in bounds) and is not stored
            uint32_t off[LB];
#pragma unroll
            for (int i = 0; i < LB; ++i) off[i] = p.lags - 1 - (l0 + i < p.lags ? l0 + i : p.lags - 1);
            double acc[LB][K];
#pragma unroll
            for (int i = 0; i < LB; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) acc[i][j] = 0.0;
            for (uint64_t t = it.c0 + tid; t < it.c1; t += kXtyThreads) {
                double yv[K];
#pragma unroll
                for (int j = 0; j < K; ++j) yv[j] = (double)*reinterpret_cast<const float *>(yr + j * p.y_row_stride + 4 * t);
#pragma unroll
                for (int i = 0; i < LB; ++i) {
                    const uint32_t v = xr[t + off[i]];
                    const double xv = (double)(v < clip ? v : clip);
#pragma unroll
                    for (int j = 0; j < K; ++j) acc[i][j] = fma(xv, yv[j], acc[i][j]);
                }
            }
#pragma unroll
            for (int i = 0; i < LB; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    double v = acc[i][j];
#pragma unroll
                    for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s);
                    if (lane == 0) red[wave][i * K + j] = v;
                }
            __syncthreads();
            if (tid < LB * K && l0 + tid / K < p.lags) {
                double s = red[0][tid];
#pragma unroll
                for (uint32_t w = 1; w < kXtyThreads / 64; ++w) s += red[w][tid];
                dst[(uint64_t)l0 * K + tid] = s;  // (l0 + i) * K + j with tid = i * K + j
            }
            __syncthreads();
        }
    }
}

// element e = (((r * n_clips + n) * rows + c) * lags + l) * k + j: its partial sum of run u is
// scratch[((u * n_clips + n) * rows + c) * lags * k + l * k + j]; out is [n_ranges][n_clips][lags][rows][k]
__global__ __launch_bounds__(kXtySumThreads) void k_xty_clips_sum(const double *scratch, const SweepRanges R, uint32_t n_clips, uint32_t rows,
                                                                  uint32_t lags, uint32_t k, uint64_t elements, double *out)
{
    const uint32_t per = lags * k;
    for (uint64_t e = (uint64_t)blockIdx.x * kXtySumThreads + threadIdx.x; e < elements; e += (uint64_t)gridDim.x * kXtySumThreads) {
        const uint64_t rnc = e / per;
        const uint32_t lj = (uint32_t)(e - rnc * per), l = lj / k, j = lj - l * k;
        const uint64_t rn = rnc / rows;
        const uint32_t c = (uint32_t)(rnc - rn * rows), r = (uint32_t)(rn / n_clips), n = (uint32_t)(rn - (uint64_t)r * n_clips);
        double s = 0.0;
        const uint64_t u0 = R.run_first[r], u1 = R.run_first[r + 1];
        if (u0 < u1) {
            s = scratch[((u0 * n_clips + n) * rows + c) * per + lj];
            for (uint64_t u = u0 + 1; u < u1; ++u) s += scratch[((u * n_clips + n) * rows + c) * per + lj];
        }
        out[((rn * lags + l) * rows + c) * k + j] = s;
    }
}

}  // namespace mh
