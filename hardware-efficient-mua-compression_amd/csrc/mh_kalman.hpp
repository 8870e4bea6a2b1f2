// mh_kalman.hpp -- the kernels of mhk_project and mhk_scan (include/muahuff_kalman.h).  What a workgroup owns, the tiles, the
// scratch and the grids are mh_kalman_layout.hpp's; DESIGN.md section 4 has the reasoning.
//
// k_project<K>: lanes lie along time.  Thread t of a workgroup owns 4 consecutive columns of the tile and keeps their K
// outputs in 4 K float64 accumulators that start at m0[j].  It walks the channels in ascending order, kProjUnroll at a
// time: the dwords of all of them are loaded before the first is used, then every byte is clipped, converted and
// multiplied into the K accumulators of its column with one fma each.  m[j][c] is the same for the whole wave (scalar
// loads).  A wave's load of one channel is 256 consecutive bytes; the row of a channel starts at any byte, so a thread
// takes its 4 bytes from the two aligned dwords that hold them and falls back to byte loads where one of those would
// reach outside the row (the first and the last thread of a row at most).  Every output is one chain: m0, then the
// channels ascending.
//
// k_scan_local<K> (kernel 1): a thread owns a tile of steps; it runs the recurrence from a zero state and multiplies the
// tile's maps together, F of the last step leftmost.  k_scan_carry<K> (kernel 2): one wave per range; lane l folds the
// tiles [l per, (l + 1) per) of the range into one affine map, the 64 maps are applied one after the other starting from
// init (every lane does all 64, reading lane l's map by v_readlane, and keeps the state in front of its own), then lane l
// walks its tiles again and writes the carry of each.  k_scan_apply<K> (kernel 3): a thread runs its tile's recurrence
// from the carry and writes every column.  No workgroup waits for another inside a launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_kalman_layout.hpp"

namespace mh {

struct ProjectParams {
    const uint8_t *x;
    uint64_t x_row_stride;
    uint32_t rows;
    uint64_t cols;
    uint32_t clip;
    const double *m, *m0;
    uint8_t *v;  // float64 rows, v_row_stride bytes apart
    uint64_t v_row_stride, tiles;
};

template <int K>
__device__ inline void proj_add(double (&acc)[K][4], uint32_t d, uint32_t clip, const double *m, uint32_t rows, uint32_t c)
{
    double mc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) mc[j] = m[(uint64_t)j * rows + c];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t u = (d >> (8 * b)) & 255u;
        const double xv = (double)(u < clip ? u : clip);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j][b] = fma(mc[j], xv, acc[j][b]);
    }
}

template <int K>
__global__ __launch_bounds__(kProjThreads) void k_project(ProjectParams p)
{
    constexpr uint32_t U = kProjUnroll;
    for (uint64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const uint64_t t = tile * kProjTileCols + (uint64_t)kProjGroup * threadIdx.x;
        if (t >= p.cols) continue;
        double acc[K][4];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double b0 = p.m0 ? p.m0[j] : 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[j][b] = b0;
        }
        uint32_t c = 0;
        for (; c + U <= p.rows; c += U) {
            uint32_t d[U];
#pragma unroll
            for (uint32_t i = 0; i < U; ++i) d[i] = load4(p.x + (uint64_t)(c + i) * p.x_row_stride, t, p.cols);
#pragma unroll
            for (uint32_t i = 0; i < U; ++i) proj_add<K>(acc, d[i], p.clip, p.m, p.rows, c + i);
        }
        for (; c < p.rows; ++c) proj_add<K>(acc, load4(p.x + (uint64_t)c * p.x_row_stride, t, p.cols), p.clip, p.m, p.rows, c);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double *const o = reinterpret_cast<double *>(p.v + (uint64_t)j * p.v_row_stride) + t;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (t + b < p.cols) o[b] = acc[j][b];
        }
    }
}

struct ScanParams {
    const uint8_t *v;  // float64 rows, v_row_stride bytes apart
    uint64_t v_row_stride;
    const double *f, *b;  // [n_gain][k][k]
    uint32_t n_gain;
    const double *init;   // [n_ranges][k]
    uint8_t *out;
    uint64_t out_row_stride;
    double *scratch;
    ScanLayout L;
};

// s = F s + B x, row by row: B's terms in ascending column order first, then F's
template <int K>
__device__ inline void scan_step(double (&s)[K], const double (&F)[K][K], const double (&B)[K][K], const double (&x)[K])
{
    double n[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double a = B[i][0] * x[0];
#pragma unroll
        for (int j = 1; j < K; ++j) a = fma(B[i][j], x[j], a);
#pragma unroll
        for (int j = 0; j < K; ++j) a = fma(F[i][j], s[j], a);
        n[i] = a;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] = n[i];
}

// P = F P, column by column, the terms of an entry in ascending order
template <int K>
__device__ inline void scan_compose(double (&P)[K][K], const double (&F)[K][K])
{
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double n[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double a = F[i][0] * P[0][c];
#pragma unroll
            for (int j = 1; j < K; ++j) a = fma(F[i][j], P[j][c], a);
            n[i] = a;
        }
#pragma unroll
        for (int i = 0; i < K; ++i) P[i][c] = n[i];
    }
}

// s = P s + e
template <int K>
__device__ inline void scan_affine(double (&s)[K], const double (&P)[K][K], const double (&e)[K])
{
    double n[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double a = e[i];
#pragma unroll
        for (int j = 0; j < K; ++j) a = fma(P[i][j], s[j], a);
        n[i] = a;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] = n[i];
}

template <int K>
__device__ inline void scan_load_gain(double (&F)[K][K], double (&B)[K][K], const ScanParams &p, uint32_t g)
{
    const double *const f = p.f + (uint64_t)g * (K * K), *const b = p.b + (uint64_t)g * (K * K);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) F[i][j] = f[i * K + j], B[i][j] = b[i * K + j];
}

// LOCAL: from a zero state, with the composite map, into scratch; otherwise from the carry, every column into out
template <int K, bool LOCAL>
__device__ inline void scan_tile(const ScanParams &p, uint64_t tile)
{
    const uint32_t r = scan_tile_range(tile, p.L.tile_base, p.L.n_ranges);
    const uint64_t a = p.L.a[r], b = p.L.b[r];
    uint64_t i0, i1;
    scan_tile_steps(tile - p.L.tile_base[r], a, b, &i0, &i1);
    double *const rec = p.scratch + tile * scan_per_tile(K);
    double s[K], P[K][K], F[K][K], B[K][K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        s[i] = LOCAL ? 0.0 : rec[K * K + K + i];
#pragma unroll
        for (int j = 0; j < K; ++j) P[i][j] = i == j ? 1.0 : 0.0;
    }
    uint32_t g = (uint32_t)(i0 < p.n_gain - 1 ? i0 : p.n_gain - 1);
    scan_load_gain<K>(F, B, p, g);
    for (uint64_t i = i0; i < i1; ++i) {
        const uint32_t gi = (uint32_t)(i < p.n_gain - 1 ? i : p.n_gain - 1);
        if (gi != g) {
            g = gi;
            scan_load_gain<K>(F, B, p, g);
        }
        const uint64_t t = a + 1 + i;
        double x[K];
#pragma unroll
        for (int j = 0; j < K; ++j) x[j] = reinterpret_cast<const double *>(p.v + (uint64_t)j * p.v_row_stride)[t];
        scan_step<K>(s, F, B, x);
        if (LOCAL) {
            scan_compose<K>(P, F);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) reinterpret_cast<double *>(p.out + (uint64_t)j * p.out_row_stride)[t] = s[j];
        }
    }
    if (LOCAL) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
            for (int j = 0; j < K; ++j) rec[i * K + j] = P[i][j];
            rec[K * K + i] = s[i];
        }
    }
}

template <int K>
__global__ __launch_bounds__(kScanThreads) void k_scan_local(ScanParams p)
{
    for (uint64_t tile = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x; tile < p.L.tiles; tile += (uint64_t)gridDim.x * kScanThreads)
        scan_tile<K, true>(p, tile);
}

template <int K>
__global__ __launch_bounds__(kScanThreads) void k_scan_apply(ScanParams p)
{
    for (uint64_t tile = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x; tile < p.L.tiles; tile += (uint64_t)gridDim.x * kScanThreads)
        scan_tile<K, false>(p, tile);
}

// lane `l`'s value of x in every lane; l is the same in all of them
__device__ inline double scan_lane(double x, uint32_t l)
{
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), (int)l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <int K>
__device__ inline void scan_load_tile(double (&P)[K][K], double (&e)[K], const double *rec)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j < K; ++j) P[i][j] = rec[i * K + j];
        e[i] = rec[K * K + i];
    }
}

template <int K>
__global__ __launch_bounds__(kScanThreads) void k_scan_carry(ScanParams p)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t a = p.L.a[r], b = p.L.b[r];
    if (b == a) return;
    const double *const init = p.init + (uint64_t)r * K;
    if (lane < (uint32_t)K) reinterpret_cast<double *>(p.out + (uint64_t)lane * p.out_row_stride)[a] = init[lane];
    const uint64_t n = scan_range_tiles(a, b);
    if (n == 0) return;
    const uint64_t per = (n + kScanThreads - 1) / kScanThreads;
    const uint64_t q0 = lane * per < n ? lane * per : n, q1 = q0 + per < n ? q0 + per : n;
    double *const rec0 = p.scratch + p.L.tile_base[r] * scan_per_tile(K);
    // this lane's tiles as one map
    double P[K][K], u[K], T[K][K], e[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        u[i] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) P[i][j] = i == j ? 1.0 : 0.0;
    }
    for (uint64_t q = q0; q < q1; ++q) {
        scan_load_tile<K>(T, e, rec0 + q * scan_per_tile(K));
        scan_affine<K>(u, T, e);
        scan_compose<K>(P, T);
    }
    // the 64 maps, one after the other
    double s[K], mine[K];
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] = init[i], mine[i] = 0.0;
    for (uint32_t l = 0; l < kScanThreads; ++l) {
        if (lane == l) {
#pragma unroll
            for (int i = 0; i < K; ++i) mine[i] = s[i];
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {
            e[i] = scan_lane(u[i], l);
#pragma unroll
            for (int j = 0; j < K; ++j) T[i][j] = scan_lane(P[i][j], l);
        }
        scan_affine<K>(s, T, e);
    }
    // the carry of each of this lane's tiles
    for (uint64_t q = q0; q < q1; ++q) {
        double *const rec = rec0 + q * scan_per_tile(K);
#pragma unroll
        for (int i = 0; i < K; ++i) rec[K * K + K + i] = mine[i];
        scan_load_tile<K>(T, e, rec);
        scan_affine<K>(mine, T, e);
    }
}

}  // namespace mh
