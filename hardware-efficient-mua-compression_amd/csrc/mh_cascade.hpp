// mh_cascade.hpp -- the kernels of mhc_moments and mhc_polyval (include/muahuff_cascade.h).  What a workgroup owns, the
// runs, the tiles and the grids are mh_cascade_layout.hpp's; DESIGN.md section 4 has the reasoning.
//
// k_moments<D>: one (run, output) item per workgroup visit.  Lanes lie along time: thread t of the workgroup takes the
// groups of 4 columns c0 + 4t, c0 + 4t + 1024, ... of the run, one 16-byte load of p and one of y each (at dword
// alignment: a pitched row starts at any float, and where the loads are cut must not depend on where the row lies, or
// the order of the sums would), and what is left of a run that is no multiple of 4 goes to threads 0..2 as dwords.  No
// load touches a float outside [c0, c1).  Per column: u = (p - center) * inv_scale, the powers u^2 .. u^2D, the
// products u^i * y, y * y and (u - y)^2, every one a float64 operation rounded on its own (contraction is off in this
// file: NumPy reproduces each term bit for bit), each added to its own accumulator: 3D + 3 doubles in registers (T_0 is
// the column count).  A butterfly over the wave, the four waves in wave order through LDS, and the item's partial sums
// go to scratch: a fixed tree, no atomics.  k_moments_sum adds an element's runs in run order and stores or adds once.
//
// k_polyval<D>: one (tile, output) item per workgroup visit, 4 columns per thread, 16-byte loads and stores at dword
// alignment, the tile's last columns as dwords.  u = (p - center) * inv_scale in float32, two roundings, then Horner as
// D fmaf: one fixed chain per output, owned by one thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_cascade_layout.hpp"

// every float operation below is rounded where it is written: no a * b + c becomes an FMA unless it says fma
#pragma clang fp contract(off)

namespace mh {

// 4 floats at dword alignment: one global_load_dwordx4 / global_store_dwordx4, which global memory takes at any dword
struct __attribute__((packed, aligned(4))) casc_f32x4 {
    float v[4];
};

struct MomParams {
    const uint8_t *p, *y;  // float rows, *_row_stride bytes apart
    uint64_t p_row_stride, y_row_stride;
    uint32_t k;
    const double *center, *inv_scale;  // NULL: 0 and 1
    double *scratch;
    uint64_t items;
    MomRanges ranges;
};

// one column into the accumulators: acc[0..2D-1] = T_1..T_2D, acc[2D..3D] = Q_0..Q_D, acc[3D+1] = YY, acc[3D+2] = E
template <int D>
__device__ inline void mom_column(double (&acc)[3 * D + 3], float pf, float yf, double c, double s)
{
    const double u = ((double)pf - c) * s, y = (double)yf;
    double w = u;
    acc[0] += w;
    acc[2 * D] += y;
    acc[2 * D + 1] += w * y;
#pragma unroll
    for (int i = 2; i <= 2 * D; ++i) {
        w = w * u;  // u^i = u^(i-1) * u
        acc[i - 1] += w;
        if (i <= D) acc[2 * D + i] += w * y;
    }
    acc[3 * D + 1] += y * y;
    const double d = u - y;
    acc[3 * D + 2] += d * d;
}

template <int D>
__global__ __launch_bounds__(kMomThreads) void k_moments(MomParams p)
{
    constexpr int N = 3 * D + 3;
    __shared__ double red[kMomThreads / 64][N];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint64_t run = item / p.k;
        const uint32_t j = (uint32_t)(item - run * p.k);
        uint64_t c0, c1;
        mom_run_cols(p.ranges, run, &c0, &c1);
        const float *const pr = reinterpret_cast<const float *>(p.p + (uint64_t)j * p.p_row_stride);
        const float *const yr = reinterpret_cast<const float *>(p.y + (uint64_t)j * p.y_row_stride);
        const double c = p.center ? p.center[j] : 0.0, s = p.inv_scale ? p.inv_scale[j] : 1.0;
        double acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = 0.0;
        const uint64_t whole = c0 + ((c1 - c0) & ~(uint64_t)3);  // the groups of 4 end here
        for (uint64_t t = c0 + 4 * tid; t < whole; t += 4 * kMomThreads) {
            const casc_f32x4 pv = *reinterpret_cast<const casc_f32x4 *>(pr + t);
            const casc_f32x4 yv = *reinterpret_cast<const casc_f32x4 *>(yr + t);
#pragma unroll
            for (int e = 0; e < 4; ++e) mom_column<D>(acc, pv.v[e], yv.v[e], c, s);
        }
        if (whole + tid < c1) mom_column<D>(acc, pr[whole + tid], yr[whole + tid], c, s);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double v = acc[i];
#pragma unroll
            for (int sh = 32; sh; sh >>= 1) v += __shfl_xor(v, sh);
            if (lane == 0) red[wave][i] = v;
        }
        __syncthreads();
        double *const dst = p.scratch + item * (uint64_t)(N + 1);
        if (tid < N) {
            double v = red[0][tid];
#pragma unroll
            for (uint32_t w = 1; w < kMomThreads / 64; ++w) v += red[w][tid];
            dst[tid + 1] = v;
        } else if (tid == N) {
            dst[0] = (double)(c1 - c0);  // T_0: exact, a run has at most kMomRun columns
        }
        __syncthreads();
    }
}

// element e = (r * k + j) * per + s: its partial sum of the range's run i is scratch[((run_first[r] + i) * k + j) * per + s]
__global__ __launch_bounds__(kMomSumThreads) void k_moments_sum(const double *scratch, MomRanges ranges, uint32_t k, uint32_t per,
                                                                uint32_t elements, double *out, uint32_t accumulate)
{
    for (uint32_t e = blockIdx.x * kMomSumThreads + threadIdx.x; e < elements; e += gridDim.x * kMomSumThreads) {
        const uint32_t rj = e / per, s = e - rj * per, r = rj / k, j = rj - r * k;
        const uint64_t r0 = ranges.run_first[r], r1 = ranges.run_first[r + 1];
        double v = 0.0;  // an empty range has no run: all its sums are zero
#pragma unroll 8
        for (uint64_t run = r0; run < r1; ++run) v += scratch[(run * k + j) * per + s];
        out[e] = accumulate ? out[e] + v : v;
    }
}

struct PolyParams {
    const uint8_t *p;  // float rows, p_row_stride bytes apart
    uint64_t p_row_stride;
    uint32_t k;
    uint64_t cols;
    const float *coef, *center, *inv_scale;  // center, inv_scale NULL: 0 and 1
    uint8_t *out;
    uint64_t out_row_stride;
    uint64_t items;
};

template <int D>
__device__ inline float poly_horner(const float (&cf)[D + 1], float pf, float c, float s)
{
    const float u = (pf - c) * s;
    float a = cf[0];
#pragma unroll
    for (int i = 1; i <= D; ++i) a = fmaf(a, u, cf[i]);
    return a;
}

template <int D>
__global__ __launch_bounds__(kPolyThreads) void k_polyval(PolyParams p)
{
    const uint32_t tid = threadIdx.x;
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint64_t tile = item / p.k;
        const uint32_t j = (uint32_t)(item - tile * p.k);
        const float *const pr = reinterpret_cast<const float *>(p.p + (uint64_t)j * p.p_row_stride);
        float *const orow = reinterpret_cast<float *>(p.out + (uint64_t)j * p.out_row_stride);
        float cf[D + 1];
#pragma unroll
        for (int i = 0; i <= D; ++i) cf[i] = p.coef[j * (D + 1) + i];
        const float c = p.center ? p.center[j] : 0.f, s = p.inv_scale ? p.inv_scale[j] : 1.f;
        const uint64_t t = tile * kPolyTile + 4 * tid;
        if (t + 4 <= p.cols) {
            casc_f32x4 v = *reinterpret_cast<const casc_f32x4 *>(pr + t);
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = poly_horner<D>(cf, v.v[e], c, s);
            *reinterpret_cast<casc_f32x4 *>(orow + t) = v;
        } else {
            for (uint64_t i = t; i < p.cols; ++i) orow[i] = poly_horner<D>(cf, pr[i], c, s);
        }
    }
}

}  // namespace mh
