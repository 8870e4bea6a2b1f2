// mh_train.hpp -- the kernels of mht_loss_grad (include/muahuff_train.h).  The rows, the scratch, the tiles and the grids
// are mh_train_layout.hpp's; DESIGN.md section 4 has the reasoning.  Row r = b * lags + s is step s of window b.
//
// k_train_inproj: act[r][g] = sum over channels of u[c][bin of r] * wx[g][c] + bias[g] on v_mfma_f32_32x32x2_f32, the rows
// as M (a wave owns 32), the channel pair as the reduction, 32 pre-activations as N.  A lane gathers ONE byte of x per
// channel pair and z-scores it in place: u = (min(x, clip) - mean[c]) * inv[c].
//
// k_train_forward<NB, KS>: k_windows of mh_lstm.hpp on the gathered windows, with a tape: the lane that read a
// pre-activation from act writes the activated gate back, and c and h of every step go to their tapes.  Then the dense
// layer, out, the loss of every window and dout = scale * err / (k * loss), 0 where the loss is 0.
//
// k_train_backward<UB>: per tile of 32 windows, for s = lags-1 down to 0: thread (unit, window) takes dh from LDS, forms
// dc and the four dz, stores them to the dz rows and to LDS [g][window]; then dh of step s-1 = Wh^T dz on the matrix
// cores, Wh^T as A fragments in registers for the whole kernel, the reduction over g cut in two halves that two waves
// take and add through LDS, first half + second half.
//
// k_train_wgrad: one wave per item.  dwx[g][c] = sum over r of dz[r][g] u[c][bin of r] and dwh[g][v] = sum over the rows r
// with s >= 1 of dz[r][g] h[r-1][v] on the matrix cores with the rows as the reduction, ascending; dbias, dwd and dbd are
// plain chains of one thread each.  Every output starts at 0 and takes its rows in ascending order: no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_lstm.hpp"
#include "mh_train_layout.hpp"

namespace mh {

struct TrainParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows;
    uint64_t cols;
    float clip;
    const float *mean, *inv;
    const int64_t *idx;
    uint32_t batch, lags, units, k;
    uint64_t lead;
    const float *wx, *bias, *wh, *wd, *bd;
    const uint8_t *y;  // float rows, y_row_stride bytes apart
    uint64_t y_row_stride;
    float scale;
    float *act, *dz, *c, *h, *dout;  // the scratch
    float *out, *loss, *dwx, *dbias, *dwh, *dwd, *dbd;
    uint32_t R;  // batch * lags
    uint32_t gtiles;
    uint64_t in_items;
    uint32_t tiles;
    uint32_t ctiles, ublocks;
    uint64_t wx_items, grad_items;
    uint32_t wh_items;
};

// the first bin of window b
__device__ inline uint64_t train_first_bin(const TrainParams &q, uint32_t b)
{
    return train_bin(q.idx[b], q.lags, q.cols, q.lead) - (q.lags - 1);
}

// u of channel c (below rows) at bin t
__device__ inline float train_u(const TrainParams &q, uint32_t c, uint64_t t)
{
    return (fminf((float)q.x[(uint64_t)c * q.x_row_stride + t], q.clip) - q.mean[c]) * q.inv[c];
}

__global__ __launch_bounds__(kTrainInThreads) void k_train_inproj(TrainParams q)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
    const uint32_t G = 4 * q.units;
    for (uint64_t item = blockIdx.x; item < q.in_items; item += gridDim.x) {
        const uint64_t rb = item / q.gtiles;
        const uint32_t gt = (uint32_t)(item - rb * q.gtiles);
        const uint64_t r0 = rb * kTrainInRows + wave * 32;  // the wave's first row
        const uint64_t r = r0 + col;                        // this lane's row of the A operand
        const uint32_t g = gt * kGradTile + col;            // this lane's column of the B operand
        const bool live = r < q.R, bcol = g < G;
        uint64_t t = 0;
        if (live) {
            const uint32_t b = (uint32_t)(r / q.lags);
            t = train_first_bin(q, b) + (uint32_t)(r - (uint64_t)b * q.lags);
        }
        const float *const wr = q.wx + (uint64_t)(bcol ? g : 0) * q.rows;
        lstm_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        // channel pair (c2, c2 + 1): lane half hh takes channel c2 + hh; an odd last channel is padded with zeros
        for (uint32_t c2 = 0; c2 < q.rows; c2 += 2) {
            const uint32_t c = c2 + hh;
            float a = 0.f, w = 0.f;
            if (c < q.rows) {
                if (live) a = train_u(q, c, t);
                if (bcol) w = wr[c];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w, acc, 0, 0, 0);
        }
        // C/D: register i of lane (col, hh) is row (i & 3) + 8 (i >> 2) + 4 hh of the wave, column col
        if (bcol) {
            const float bias = q.bias[g];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint64_t rr = r0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (rr < q.R) q.act[rr * G + g] = acc[i] + bias;
            }
        }
    }
}

template <int NB, int KS>
__global__ __launch_bounds__(kWinThreads) void k_train_forward(TrainParams q)
{
    __shared__ float hbuf[2][2 * KS][kWinTile];  // h of the tile's windows, [unit][window]; the rows from units on stay zero
    __shared__ float obuf[kLstmMaxK][kWinTile];  // out of the tile's windows
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
    for (uint32_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
        const uint32_t i0 = tile * kWinTile;
        const bool valid = i0 + col < q.batch;  // a window past the last one runs on zeros and nothing of it is stored
        const uint32_t row0 = (i0 + col) * q.lags;  // rows and the offsets below stay inside 32 bits: R 4U < 2^30
        float c[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[b][j] = 0.f;
        for (uint32_t s = 0; s < q.lags; ++s) {
            const uint32_t po = (row0 + s) * G, co = (row0 + s) * U;  // this step's row of act, and of c and h
            lstm_f32x16 acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t unit = win_unit(wave + kWinWaves * b, hh, r);
                    acc[b][r] = valid && unit < U ? q.act[po + win_gate(r) * U + unit] : 0.f;
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
                    const float hv = go * lstm_tanh(c[b][j]);
                    if (unit < U) {
                        hn[unit * kWinTile] = hv;
                        if (valid) {  // the tape
                            float *const ar = q.act + po + unit;
                            ar[0] = gi, ar[U] = gf, ar[2 * U] = gg, ar[3 * U] = go;
                            q.c[co + unit] = c[b][j];
                            q.h[co + unit] = hv;
                        }
                    }
                }
            __syncthreads();
        }
        // the dense layer on the last h: thread (output j, window n), the units ascending, then the bias
        if (tid < kWinTile * q.k) {
            const uint32_t j = tid >> 5, n = tid & 31;
            const float *const hf = &hbuf[q.lags & 1][0][n];
            const float *const wd = q.wd + (uint64_t)j * U;
            float sum = 0.f;
            for (uint32_t v = 0; v < U; ++v) sum = fmaf(wd[v], hf[v * kWinTile], sum);
            sum += q.bd[j];
            obuf[j][n] = sum;
            if (i0 + n < q.batch) q.out[(uint64_t)j * q.batch + i0 + n] = sum;
        }
        __syncthreads();
        // the loss of a window, sqrt(mean over j of err^2), and dout = scale * err / (k * loss); 0 where the loss is 0
        if (tid < kWinTile && i0 + tid < q.batch) {
            const uint32_t b = i0 + tid;
            const uint64_t t = train_bin(q.idx[b], q.lags, q.cols, q.lead) + q.lead;
            float err[kLstmMaxK], ss = 0.f;
#pragma unroll
            for (uint32_t j = 0; j < kLstmMaxK; ++j) {
                err[j] = 0.f;
                if (j < q.k) {
                    err[j] = obuf[j][tid] - *reinterpret_cast<const float *>(q.y + (uint64_t)j * q.y_row_stride + 4 * t);
                    ss = fmaf(err[j], err[j], ss);
                }
            }
            const float loss = sqrtf(ss / (float)q.k);
            q.loss[b] = loss;
            const float f = loss > 0.f ? q.scale / ((float)q.k * loss) : 0.f;
#pragma unroll
            for (uint32_t j = 0; j < kLstmMaxK; ++j) q.dout[(uint64_t)b * kTrainDoutPitch + j] = j < q.k ? f * err[j] : 0.f;
        }
        __syncthreads();
    }
}

template <int UB>
__global__ __launch_bounds__(kBwdThreads) void k_train_backward(TrainParams q)
{
    constexpr int KS = kBwdKSteps * UB;            // k-steps of a wave: the 2U pre-activations of its half, padded
    __shared__ float dzb[4 * KS][kBwdPitch];       // dz of the tile's windows, [g][window]; the rows from 4U on stay zero
    __shared__ float dhb[32 * UB][kBwdPitch];      // dh of the tile's windows, [unit][window]
    __shared__ float dcb[32 * UB][kBwdPitch];      // dc of the tile's windows, each value its thread's own
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
    const uint32_t U = q.units, G = 4 * U, L = q.lags;
    const uint32_t mb = wave & 3, rh = wave >> 2;  // the unit block and the half of the reduction of this wave
    const bool works = mb < UB;
    // the A fragments of Wh^T: lane (col, hh) holds row m = col, unit 32 mb + col, the pre-activations rh 2U + 2 ks + hh
    float a[KS];
    {
        const uint32_t v = 32 * mb + col;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint32_t g = rh * 2 * U + 2 * ks + hh;
            a[ks] = works && v < U && (uint32_t)ks < U ? q.wh[(uint64_t)g * U + v] : 0.f;
        }
    }
    for (uint32_t i = tid; i < 4 * KS * kBwdPitch; i += kBwdThreads) (&dzb[0][0])[i] = 0.f;
    for (uint32_t i = tid; i < 32 * UB * kBwdPitch; i += kBwdThreads) (&dhb[0][0])[i] = 0.f;
    __syncthreads();
    // the elementwise part: thread (v0, n) takes the units v0, v0 + 16, ..
    const uint32_t n = tid >> 4, v0 = tid & 15;
    for (uint32_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
        const uint32_t b = tile * kWinTile + n;
        const bool valid = b < q.batch;
        const uint64_t row0 = (uint64_t)b * L;
        // dh of the last step from the dense layer: the outputs ascending
#pragma unroll 1
        for (uint32_t v = v0; v < U; v += 16) {
            dcb[v][n] = 0.f;
            {
                float sum = 0.f;
                if (valid)
                    for (uint32_t o = 0; o < q.k; ++o) sum = fmaf(q.wd[(uint64_t)o * U + v], q.dout[(uint64_t)b * kTrainDoutPitch + o], sum);
                dhb[v][n] = sum;
            }
        }
        for (uint32_t s = L; s-- > 0;) {
#pragma unroll 1
            for (uint32_t v = v0; v < U; v += 16) {
                {
                    float zi = 0.f, zf = 0.f, zg = 0.f, zo = 0.f;
                    if (valid) {
                        const float *const ar = q.act + (row0 + s) * G;
                        const float gi = ar[v], gf = ar[U + v], gg = ar[2 * U + v], go = ar[3 * U + v];
                        const float cv = q.c[(row0 + s) * U + v], cp = s > 0 ? q.c[(row0 + s - 1) * U + v] : 0.f;
                        const float tc = lstm_tanh(cv), dh = dhb[v][n];
                        const float d = dcb[v][n] + dh * go * (1.f - tc * tc);
                        zi = d * gg * gi * (1.f - gi);
                        zf = d * cp * gf * (1.f - gf);
                        zg = d * gi * (1.f - gg * gg);
                        zo = dh * tc * go * (1.f - go);
                        dcb[v][n] = d * gf;
                        float *const dr = q.dz + (row0 + s) * G;
                        dr[v] = zi, dr[U + v] = zf, dr[2 * U + v] = zg, dr[3 * U + v] = zo;
                    }
                    dzb[v][n] = zi, dzb[U + v][n] = zf, dzb[2 * U + v][n] = zg, dzb[3 * U + v][n] = zo;
                }
            }
            if (s == 0) break;
            __syncthreads();
            lstm_f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (works) {
                const float *const zb = &dzb[rh * 2 * U + hh][col];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const float bv = (uint32_t)ks < U ? zb[2 * ks * kBwdPitch] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], bv, acc, 0, 0, 0);
                }
                // C/D: register r of lane (col, hh) is unit 32 mb + (r & 3) + 8 (r >> 2) + 4 hh, window col
                if (rh == 1)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dhb[32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hh][col] = acc[r];
            }
            __syncthreads();
            if (works && rh == 0)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float *const d = &dhb[32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hh][col];
                    *d = acc[r] + *d;
                }
            __syncthreads();
        }
        __syncthreads();
    }
}

// row r -> its window and step
struct TrainRow {
    uint32_t b, s;
};
__device__ inline TrainRow train_row(uint32_t r, uint32_t lags)
{
    const uint32_t b = r / lags;
    return {b, r - b * lags};
}

__global__ __launch_bounds__(kGradThreads) void k_train_wgrad(TrainParams q)
{
    const uint32_t lane = threadIdx.x, col = lane & 31, hh = lane >> 5;
    const uint32_t U = q.units, G = 4 * U, R = q.R, L = q.lags;
    for (uint64_t item = blockIdx.x; item < q.grad_items; item += gridDim.x) {
        if (item < q.wx_items + q.wh_items) {
            const bool is_wx = item < q.wx_items;
            const uint64_t it = is_wx ? item : item - q.wx_items;
            const uint32_t ntiles = is_wx ? q.ctiles : q.ublocks;
            const uint32_t gt = (uint32_t)(it / ntiles), nt = (uint32_t)(it - (uint64_t)gt * ntiles);
            const uint32_t g = gt * kGradTile + col;   // this lane's row of the A operand
            const uint32_t nn = nt * kGradTile + col;  // this lane's column of the B operand: a channel or a unit
            const uint32_t nmax = is_wx ? q.rows : U;
            const bool arow = g < G, bcol = nn < nmax;
            lstm_f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            // the reduction: the row pair (r2, r2 + 1), lane half hh takes row r2 + hh; an odd last row is padded with zeros
            if (is_wx) {
                const float mean = bcol ? q.mean[nn] : 0.f, inv = bcol ? q.inv[nn] : 0.f;
                const uint8_t *const xr = q.x + (uint64_t)(bcol ? nn : 0) * q.x_row_stride;

                for (uint32_t r2 = 0; r2 < R; r2 += 2) {
                    const uint32_t r = r2 + hh;
                    float av = 0.f, bv = 0.f;
                    if (r < R) {
                        if (arow) av = q.dz[(uint64_t)r * G + g];
                        if (bcol) {
                            const TrainRow w = train_row(r, L);
                            bv = (fminf((float)xr[train_first_bin(q, w.b) + w.s], q.clip) - mean) * inv;
                        }
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                }
            } else {

                for (uint32_t r2 = 0; r2 < R; r2 += 2) {
                    const uint32_t r = r2 + hh;
                    float av = 0.f, bv = 0.f;
                    if (r < R) {
                        if (arow) av = q.dz[(uint64_t)r * G + g];
                        if (bcol && train_row(r, L).s > 0) bv = q.h[(uint64_t)(r - 1) * U + nn];
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                }
            }
            // C/D: register i of lane (col, hh) is row gt 32 + (i & 3) + 8 (i >> 2) + 4 hh, column nn
            if (bcol) {
                float *const dst = is_wx ? q.dwx : q.dwh;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t gg = gt * kGradTile + (i & 3) + 8 * (i >> 2) + 4 * hh;
                    if (gg < G) dst[(uint64_t)gg * nmax + nn] = acc[i];
                }
            }
        } else {
            // the remaining sums, one thread per output: dbias [4U], then dwd [k][U], then dbd [k]
            const uint32_t o = (uint32_t)(item - q.wx_items - q.wh_items) * kGradThreads + lane;
            float sum = 0.f;
            if (o < G) {
                for (uint32_t r = 0; r < R; ++r) sum += q.dz[(uint64_t)r * G + o];
                q.dbias[o] = sum;
            } else if (o < G + q.k * U) {
                const uint32_t j = (o - G) / U, v = o - G - j * U;
                for (uint32_t b = 0; b < q.batch; ++b)
                    sum = fmaf(q.dout[(uint64_t)b * kTrainDoutPitch + j], q.h[((uint64_t)b * L + L - 1) * U + v], sum);
                q.dwd[o - G] = sum;
            } else if (o < G + q.k * U + q.k) {
                const uint32_t j = o - G - q.k * U;
                for (uint32_t b = 0; b < q.batch; ++b) sum += q.dout[(uint64_t)b * kTrainDoutPitch + j];
                q.dbd[j] = sum;
            }
        }
    }
}

}  // namespace mh
