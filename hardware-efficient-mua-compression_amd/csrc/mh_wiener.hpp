// mh_wiener.hpp -- the kernels of mhw_xty and mhw_fir (include/muahuff_wiener.h).  What a workgroup owns, the runs, the
// tiles and the grids are mh_wiener_layout.hpp's; DESIGN.md section 4 has the reasoning.
//
// k_xty<K>: one (run, channel) item per workgroup visit.  Lanes lie along time: thread t of the workgroup takes the
// columns c0 + t, c0 + t + 256, ... of the run, converts the K covariates of a column to float64 once and multiplies
// them with the clipped counts of kXtyLagBlock lags, each product an exact float64 FMA (8 bits x 24 bits) into its own
// accumulator.  A butterfly over the wave, the four waves in wave order through LDS, and the item's partial sums go to
// scratch: a fixed tree, no atomics.  k_xty_sum adds an element's runs in run order and stores or adds once.
//
// k_fir: one (workgroup tile, M-tile) item per workgroup visit.  P[m][u] = sum over channels of w[m][c] * xq[c][u] on
// v_mfma_f32_32x32x2_f32: the 32 rows m are (output, lag), the reduction dimension is the channel pair (lane half
// l >> 5 picks the channel), the 32 columns are time.  A lane loads ONE dword of x -- 4 bins of its channel, from
// aligned dwords and a shift, since a row starts at any byte -- converts the 4 bytes and feeds 4 accumulator tiles, one per
// byte position: a wave owns 32 rows x 128 P columns in 64 registers, a workgroup 512 P columns.  The waves store their
// tiles into one LDS image [32][512]; after the barrier output i is P[(j,0)][i+L-1] + P[(j,1)][i+L-2] + ... + bias[j],
// in that order.  Every output is one fixed chain: channels ascending (the instruction's k order), lags ascending, the
// bias last.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_wiener_layout.hpp"

namespace mh {

struct XtyParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows;
    uint64_t cols;
    uint32_t lags, clip;
    const uint8_t *y;  // float rows, y_row_stride bytes apart
    uint64_t y_row_stride;
    double *scratch;
    uint64_t items;
};

template <int K>
__global__ __launch_bounds__(kXtyThreads) void k_xty(XtyParams p)
{
    constexpr int LB = (int)kXtyLagBlock;
    __shared__ double red[kXtyThreads / 64][LB * K];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint64_t run = item / p.rows;
        const uint32_t c = (uint32_t)(item - run * p.rows);
        uint64_t c0, c1;
        xty_run_cols(run, p.cols, &c0, &c1);
        const uint8_t *const xr = p.x + (uint64_t)c * p.x_row_stride;
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
            for (uint64_t t = c0 + tid; t < c1; t += kXtyThreads) {
                double yv[K];
#pragma unroll
                for (int j = 0; j < K; ++j) yv[j] = (double)*reinterpret_cast<const float *>(p.y + j * p.y_row_stride + 4 * t);
#pragma unroll
                for (int i = 0; i < LB; ++i) {
                    const uint32_t v = xr[t + off[i]];
                    const double xv = (double)(v < p.clip ? v : p.clip);
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

// element e = (c * lags + l) * k + j: its partial sum of run r is scratch[r * elements + e]
__global__ __launch_bounds__(kXtySumThreads) void k_xty_sum(const double *scratch, uint64_t runs, uint32_t rows, uint32_t lags,
                                                            uint32_t k, uint64_t elements, double *out, uint32_t accumulate)
{
    const uint32_t per = lags * k;
    for (uint64_t e = (uint64_t)blockIdx.x * kXtySumThreads + threadIdx.x; e < elements; e += (uint64_t)gridDim.x * kXtySumThreads) {
        const uint32_t c = (uint32_t)(e / per), r = (uint32_t)(e - (uint64_t)c * per), l = r / k, j = r - l * k;
        double s = scratch[e];
        for (uint64_t run = 1; run < runs; ++run) s += scratch[run * elements + e];
        const uint64_t o = ((uint64_t)l * rows + c) * k + j;
        out[o] = accumulate ? out[o] + s : s;
    }
}

struct FirParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows;
    uint64_t cols;
    uint32_t lags;
    float clip;
    const float *w, *bias;
    uint32_t k;
    uint8_t *out;  // float rows, out_row_stride bytes apart
    uint64_t out_row_stride;
    uint32_t tile_outputs, per_mtile, mtiles;
    uint64_t items;
};

typedef float fir_f32x16 __attribute__((ext_vector_type(16)));

// the 4 bytes at row + u .. row + u + 3 as one dword, from the aligned dwords that hold them; `end` is one past the
// row's last readable byte and row + u is below it: no dword without a byte of the row is touched
__device__ inline uint32_t fir_load4(const uint8_t *row, uint64_t u, const uint8_t *end)
{
    const uintptr_t a = (uintptr_t)(row + u), a0 = a & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t lo = *reinterpret_cast<const uint32_t *>(a0);
    uint32_t hi = 0;
    if (sh && a0 + 4 < (uintptr_t)end) hi = *reinterpret_cast<const uint32_t *>(a0 + 4);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}

__global__ __launch_bounds__(kFirThreads) void k_fir(FirParams p)
{
    __shared__ float img[kFirMRows * kFirTileCols];  // P of the workgroup tile, [row m][P column]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const uint64_t ncol = p.cols + p.lags - 1;
    // this lane's row of the A operand: m = col is (output jj of the M-tile, lag l)
    const uint32_t jj_a = col / p.lags, l_a = col - jj_a * p.lags;
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint64_t tile = item / p.mtiles;
        const uint32_t mt = (uint32_t)(item - tile * p.mtiles);
        const uint64_t i0 = tile * p.tile_outputs;                  // the tile's first output and first P column
        const uint64_t u = i0 + wave * kFirWaveCols + 4 * col;      // this lane's 4 P columns
        const uint32_t j_a = mt * p.per_mtile + jj_a;
        const bool arow = jj_a < p.per_mtile && j_a < p.k;          // the other rows of the M-tile are zero
        const float *const wr = p.w + ((uint64_t)j_a * p.lags + l_a) * p.rows;
        const bool live = u < ncol;
        fir_f32x16 acc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        // channel pair (c2, c2 + 1): lane half h takes channel c2 + h; an odd last channel is padded with zeros.  The
        // next pair's operands are loaded before this pair's products are issued.
        float a_n = 0.f;
        uint32_t d_n = 0;
        if (h < p.rows) {
            if (arow) a_n = wr[h];
            if (live) d_n = fir_load4(p.x + (uint64_t)h * p.x_row_stride, u, p.x + (uint64_t)h * p.x_row_stride + ncol);
        }
        for (uint32_t c2 = 0; c2 < p.rows; c2 += 2) {
            const float a = a_n;
            const uint32_t d = d_n;
            const uint32_t c = c2 + 2 + h;
            a_n = 0.f, d_n = 0;
            if (c < p.rows) {
                const uint8_t *const row = p.x + (uint64_t)c * p.x_row_stride;
                if (arow) a_n = wr[c];
                if (live) d_n = fir_load4(row, u, row + ncol);
            }
            const float b0 = fminf((float)(d & 0xffu), p.clip), b1 = fminf((float)((d >> 8) & 0xffu), p.clip);
            const float b2 = fminf((float)((d >> 16) & 0xffu), p.clip), b3 = fminf((float)(d >> 24), p.clip);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b3, acc[3], 0, 0, 0);
        }
        // C/D: register r of lane (col, h) is row (r & 3) + 8 (r >> 2) + 4 h, column col; tile b is byte position b
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t m = (r & 3) + 8 * (r >> 2) + 4 * h;
            *reinterpret_cast<float4 *>(&img[m * kFirTileCols + wave * kFirWaveCols + 4 * col]) =
                make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        }
        __syncthreads();
        const uint64_t left = p.cols - i0;
        const uint32_t n_out = left < p.tile_outputs ? (uint32_t)left : p.tile_outputs;
        for (uint32_t jj = 0; jj < p.per_mtile; ++jj) {
            const uint32_t j = mt * p.per_mtile + jj;
            if (j >= p.k) break;
            const float bias = p.bias[j];
            float *const orow = reinterpret_cast<float *>(p.out + (uint64_t)j * p.out_row_stride) + i0;
            const float *const base = img + jj * p.lags * kFirTileCols + p.lags - 1;
            for (uint32_t il = tid; il < n_out; il += kFirThreads) {
                float s = base[il];
                for (uint32_t l = 1; l < p.lags; ++l) s += base[l * kFirTileCols + il - l];
                orow[il] = s + bias;
            }
        }
        __syncthreads();
    }
}

}  // namespace mh
