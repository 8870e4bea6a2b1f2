// mh_lstm.hpp -- the kernels of mhl_inproj and mhl_windows (include/muahuff_lstm.h).  What a workgroup owns, the tiles,
// the permutation of the gates and the grids are mh_lstm_layout.hpp's; DESIGN.md section 4 has the reasoning.
//
// k_inproj: one (column tile, g-tile) item per workgroup visit.  P[t][g] = sum over channels of xq[c][t] * wx[g][c] on
// v_mfma_f32_32x32x2_f32 with TIME as the M dimension: the reduction dimension is the channel pair (lane half l >> 5
// picks the channel), the 32 columns are pre-activations.  A lane loads ONE dword of x -- 4 bins of its channel --
// converts the 4 bytes and feeds 4 accumulator tiles, one per byte position, as k_fir does; its B operand is one weight.
// In the C layout a register holds one bin and the 32 lanes of a half 32 consecutive pre-activations, so a store
// instruction writes two runs of 128 bytes of the time-major p.  Every output is one chain: 0, the channels ascending
// (the instruction's k order), then the bias.
//
// k_windows<NB, KS>: one tile of 32 consecutive windows per workgroup visit, the windows as the MFMA's N.  A wave holds
// the rows of Wh of its NB blocks as A fragments in registers for the whole kernel (KS k-steps each), h of the tile's
// windows lies in LDS as the B operand [unit][window], double-buffered, and c stays in registers: a lane owns the four
// gates of its 4 units per block.  Step s starts its accumulators from p's row i + s in the C layout and adds the
// recurrent half over the units ascending; step 0 has h = 0 and issues no product.  The dense layer reads the last h
// from LDS: one thread per (output, window), the units ascending, then the bias.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_lstm_layout.hpp"

namespace mh {

typedef float lstm_f32x16 __attribute__((ext_vector_type(16)));

struct InprojParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows;
    uint64_t cols;
    float clip;
    const float *wx, *bias;
    uint32_t units;
    float *p;
    uint32_t gtiles;
    uint64_t items;
};

__global__ __launch_bounds__(kInThreads) void k_inproj(InprojParams q)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const uint32_t G = 4 * q.units;
    for (uint64_t item = blockIdx.x; item < q.items; item += gridDim.x) {
        const uint64_t tile = item / q.gtiles;
        const uint32_t gt = (uint32_t)(item - tile * q.gtiles);
        const uint64_t t0 = tile * kInTileCols + wave * kInWaveCols;  // the wave's first column
        const uint64_t u = t0 + 4 * col;                              // this lane's 4 columns: rows of the A operand
        const uint32_t g = gt * kInGTile + col;                       // this lane's column of the B operand
        const bool bcol = g < G;                                      // the other columns of the g-tile are zero
        const float *const wr = q.wx + (uint64_t)(bcol ? g : 0) * q.rows;
        const bool live = u < q.cols;
        lstm_f32x16 acc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        // channel pair (c2, c2 + 1): lane half h takes channel c2 + h; an odd last channel is padded with zeros.  The
        // next pair's operands are loaded before this pair's products are issued.
        float w_n = 0.f;
        uint32_t d_n = 0;
        if (h < q.rows) {
            if (bcol) w_n = wr[h];
            if (live) d_n = load4(q.x + (uint64_t)h * q.x_row_stride, u, q.cols);
        }
        for (uint32_t c2 = 0; c2 < q.rows; c2 += 2) {
            const float w = w_n;
            const uint32_t d = d_n;
            const uint32_t c = c2 + 2 + h;
            w_n = 0.f, d_n = 0;
            if (c < q.rows) {
                if (bcol) w_n = wr[c];
                if (live) d_n = load4(q.x + (uint64_t)c * q.x_row_stride, u, q.cols);
            }
            const float a0 = fminf((float)(d & 0xffu), q.clip), a1 = fminf((float)((d >> 8) & 0xffu), q.clip);
            const float a2 = fminf((float)((d >> 16) & 0xffu), q.clip), a3 = fminf((float)(d >> 24), q.clip);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, w, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, w, acc[3], 0, 0, 0);
        }
        // C/D: register r of lane (col, h) is row i = (r & 3) + 8 (r >> 2) + 4 h, column col; row i of tile b is the
        // column t0 + 4 i + b of x
        if (bcol) {
            const float bias = q.bias[g];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint64_t t = t0 + 4 * i + b;
                    if (t < q.cols) q.p[t * G + g] = acc[b][r] + bias;
                }
            }
        }
    }
}

struct WinParams {
    const float *p;
    uint32_t lags, units;
    const float *wh, *wd, *bd;
    uint32_t k;
    uint8_t *out;  // float rows, out_row_stride bytes apart
    uint64_t out_row_stride;
    uint64_t windows, tiles;
};

// 1 / (1 + e^-x): e^-x = inf gives 0, e^-x = 0 gives 1; never inf / inf
__device__ inline float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// with m = e^(-2|x|) - 1 in [-1, 0]: tanh |x| = -m / (2 + m), a quotient of a numerator in [0, 1] and a denominator in
// [1, 2]; m = -1 gives 1
__device__ inline float lstm_tanh(float x)
{
    const float m = expm1f(-2.0f * fabsf(x));
    return copysignf(-m / (2.0f + m), x);
}

template <int NB, int KS>
__global__ __launch_bounds__(kWinThreads) void k_windows(WinParams q)
{
    __shared__ float hbuf[2][2 * KS][kWinTile];  // h of the tile's windows, [unit][window]; the rows from units on stay zero
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
    const uint32_t U = q.units, G = 4 * U;
    // the A fragments: lane (col, hh) holds row m = col of its blocks, the previous units 2 ks + hh
    float a[NB][KS];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint32_t unit = win_row_unit(wave + kWinWaves * b, col), gate = win_row_gate(col);
        const float *const wr = q.wh + (uint64_t)(gate * U + (unit < U ? unit : 0)) * U;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint32_t v = 2 * ks + hh;
            a[b][ks] = unit < U && v < U ? wr[v] : 0.f;
        }
    }
    for (uint32_t i = tid; i < 2 * 2 * KS * kWinTile; i += kWinThreads) (&hbuf[0][0][0])[i] = 0.f;
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
        const uint64_t i0 = tile * kWinTile;
        const bool valid = i0 + col < q.windows;  // a window past the last one runs on zeros and is not stored
        const float *pr = q.p + (i0 + col) * G;   // row i + s of p
        float c[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[b][j] = 0.f;
        for (uint32_t s = 0; s < q.lags; ++s, pr += G) {
            // the accumulators start from p's row in the C layout (the wave that shares the SIMD covers the wait)
            lstm_f32x16 acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t unit = win_unit(wave + kWinWaves * b, hh, r);
                    acc[b][r] = valid && unit < U ? pr[win_gate(r) * U + unit] : 0.f;
                }
            if (s > 0) {
                const float *const hb = &hbuf[s & 1][hh][col];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const float bv = hb[2 * ks * kWinTile];
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[b][ks], bv, acc[b], 0, 0, 0);
                }
            }
            float *const hn = &hbuf[(s + 1) & 1][0][col];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t unit = win_unit(wave + kWinWaves * b, hh, j);
                    const float gi = lstm_sigmoid(acc[b][j]), gf = lstm_sigmoid(acc[b][4 + j]);
                    const float gg = lstm_tanh(acc[b][8 + j]), go = lstm_sigmoid(acc[b][12 + j]);
                    c[b][j] = gf * c[b][j] + gi * gg;
                    if (unit < U) hn[unit * kWinTile] = go * lstm_tanh(c[b][j]);
                }
            __syncthreads();
        }
        // the dense layer on the last h: thread (output j, window n), the units ascending, then the bias
        if (tid < kWinTile * q.k) {
            const uint32_t j = tid >> 5, n = tid & 31;
            if (i0 + n < q.windows) {
                const float *const hf = &hbuf[q.lags & 1][0][n];
                const float *const wd = q.wd + (uint64_t)j * U;
                float sum = 0.f;
                for (uint32_t v = 0; v < U; ++v) sum = fmaf(wd[v], hf[v * kWinTile], sum);
                *reinterpret_cast<float *>(q.out + (uint64_t)j * q.out_row_stride + 4 * (i0 + n)) = sum + q.bd[j];
            }
        }
        __syncthreads();
    }
}

}  // namespace mh
