// mh_windows.hpp -- the kernels of mhi_windows (include/muahuff_ingest.h): the same window [win_off[k], win_off[k] + W)
// of every row of a uint8 matrix for many k, re-binned by r from the window's own first sample, stacked per window or
// summed over the windows (with the sum of squares of the per-window bin values).  The forms, the tiles and the grid
// are mh_windows_layout.hpp's; this file is what runs on them.
//
// Every output element has ONE owner -- a lane (kWinLane, kWinStage) or a wave (kWinWave) -- and in the SUM form the
// owner walks the windows itself with its accumulators in registers and stores once: no atomics touch the result, and
// it is the same from run to run.  A window is short and starts at any byte, so the loads are the unaligned 16-byte
// ones of mh_device.hpp, kWinUnroll windows of them in flight per owner; a ragged end is read byte by byte, so that no
// byte outside [win_off[k], win_off[k] + W) of a row is read.
// win_off and win_idx are untrusted: a window is compared with cols (subtractively) and its slot with n_out before any
// address is formed; a refused window is skipped and counted in bad by the owner of (row 0, tile 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_device.hpp"
#include "mh_windows_layout.hpp"

namespace mh {

constexpr int kWinUnroll = 4;  // windows whose loads a SUM owner issues before it adds any of them

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct WinParams {
    const uint8_t *in;
    uint64_t row_stride, rows, cols;
    const uint64_t *win_off, *win_idx;
    uint64_t n_out;
    uint32_t n_win, W, r, nb, tile_bins, tiles;
    uint64_t items;
    uint8_t *out;
    uint64_t out_win_stride, out_row_stride;
    uint8_t *sumsq;
    uint64_t sq_row_stride;
    uint32_t accumulate;
    unsigned long long *bad;
};

// window k's first column, or false: it does not lie inside [0, cols)
__device__ __forceinline__ bool win_start(const WinParams &p, uint64_t k, uint64_t &off)
{
    off = p.win_off[k];
    return p.W <= p.cols && off <= p.cols - p.W;
}

__device__ __forceinline__ void win_refuse(const WinParams &p, uint64_t k)
{
    atomicAdd(p.bad, 1ull);
    atomicMin(p.bad + 1, (unsigned long long)k);
}

// item -> (tile, row, k): 32-bit divisions where everything fits them
__device__ __forceinline__ void win_split(const WinParams &p, uint64_t item, uint32_t &tile, uint64_t &row, uint32_t &k)
{
    if (((item | p.rows) >> 32) == 0) {
        const uint32_t i = (uint32_t)item, q = i / p.tiles, kk = q / (uint32_t)p.rows;
        tile = i - q * p.tiles, row = q - kk * (uint32_t)p.rows, k = kk;
    } else {
        const uint64_t q = item / p.tiles, kk = q / p.rows;
        tile = (uint32_t)(item - q * p.tiles), row = q - kk * p.rows, k = (uint32_t)kk;
    }
}

// n <= 16 bytes at any address, zero padded: one 16-byte load, or byte by byte at a ragged end
__device__ __forceinline__ u32x4 win_load(const uint8_t *src, uint32_t n)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n >= 16) {
        v = *reinterpret_cast<const u32x4_u *>(src);
    } else {
        for (uint32_t j = 0; j < n; ++j) v[j >> 2] |= (uint32_t)src[j] << (8 * (j & 3));
    }
    return v;
}

__device__ __forceinline__ uint32_t win_byte(const u32x4 &v, int j) { return (v[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

__device__ __forceinline__ uint32_t win_sum16(const u32x4 &v, uint32_t acc)
{
    acc = __builtin_amdgcn_sad_u8(v[0], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v[1], 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v[2], 0u, acc);
    return __builtin_amdgcn_sad_u8(v[3], 0u, acc);
}

template <bool OUT32>
__device__ __forceinline__ void win_put(uint8_t *row, uint32_t b, uint32_t s)
{
    if (OUT32)
        reinterpret_cast<uint32_t *>(row)[b] = s;
    else
        row[b] = (uint8_t)(s > 255u ? 255u : s);
}

// the SUM form's one store of element (row, b)
template <bool SQ>
__device__ __forceinline__ void win_store_sum(const WinParams &p, uint64_t row, uint32_t b, uint32_t acc, uint64_t sq)
{
    uint32_t *const o = reinterpret_cast<uint32_t *>(p.out + row * p.out_row_stride) + b;
    *o = p.accumulate ? *o + acc : acc;
    if (SQ) {
        uint64_t *const q = reinterpret_cast<uint64_t *>(p.sumsq + row * p.sq_row_stride) + b;
        *q = p.accumulate ? *q + sq : sq;
    }
}

// ---- r == 1, STACK: a lane copies its 16 samples of one window
template <bool OUT32>
__global__ __launch_bounds__(kWinThreads) void k_win_lane_stack(const WinParams p)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWinThreads;
    for (uint64_t item = (uint64_t)blockIdx.x * kWinThreads + threadIdx.x; item < p.items; item += stride) {
        uint32_t tile, k;
        uint64_t row, off;
        win_split(p, item, tile, row, k);
        const uint64_t slot = p.win_idx ? p.win_idx[k] : k;
        if (!win_start(p, k, off) || slot >= p.n_out) {
            if (tile == 0 && row == 0) win_refuse(p, k);
            continue;
        }
        const uint32_t c0 = tile * kWinLaneBytes, n = p.W - c0 < kWinLaneBytes ? p.W - c0 : kWinLaneBytes;
        const u32x4 v = win_load(p.in + row * p.row_stride + off + c0, n);
        uint8_t *const dst = p.out + slot * p.out_win_stride + row * p.out_row_stride + (uint64_t)c0 * (OUT32 ? 4 : 1);
        if (n == kWinLaneBytes) {
            if (OUT32) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const u32x4 w = {v[q] & 0xFFu, (v[q] >> 8) & 0xFFu, (v[q] >> 16) & 0xFFu, v[q] >> 24};
                    reinterpret_cast<u32x4_a4 *>(dst)[q] = w;
                }
            } else {
                *reinterpret_cast<u32x4_u *>(dst) = v;
            }
        } else {
            for (uint32_t j = 0; j < n; ++j) win_put<OUT32>(dst, j, (v[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        }
    }
}

// ---- r == 1, SUM: a lane owns 16 samples of a row and walks the windows
template <bool SQ>
__global__ __launch_bounds__(kWinThreads) void k_win_lane_sum(const WinParams p)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWinThreads;
    for (uint64_t item = (uint64_t)blockIdx.x * kWinThreads + threadIdx.x; item < p.items; item += stride) {
        uint32_t tile, k_unused;
        uint64_t row;
        win_split(p, item, tile, row, k_unused);
        const uint32_t c0 = tile * kWinLaneBytes, n = p.W - c0 < kWinLaneBytes ? p.W - c0 : kWinLaneBytes;
        const uint8_t *const src = p.in + row * p.row_stride + c0;
        uint32_t acc[16];
        uint64_t sq[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0, sq[j] = 0;
        for (uint64_t k0 = 0; k0 < p.n_win; k0 += kWinUnroll) {
            u32x4 v[kWinUnroll];
#pragma unroll
            for (int u = 0; u < kWinUnroll; ++u) {
                const uint64_t k = k0 + u;
                uint64_t off;
                v[u] = u32x4{0u, 0u, 0u, 0u};
                if (k < p.n_win) {
                    if (win_start(p, k, off))
                        v[u] = win_load(src + off, n);
                    else if (item == 0)
                        win_refuse(p, k);
                }
            }
#pragma unroll
            for (int u = 0; u < kWinUnroll; ++u) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t x = win_byte(v[u], j);
                    acc[j] += x;
                    if (SQ) sq[j] += (uint64_t)(x * x);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((uint32_t)j < n) win_store_sum<SQ>(p, row, c0 + j, acc[j], sq[j]);
    }
}

// bytes [lo, hi) of a staged tile, hi > lo: dword reads, one v_sad_u8 each, masks at the two edges
__device__ __forceinline__ uint32_t win_lds_sum(const uint32_t *t, uint32_t lo, uint32_t hi)
{
    uint32_t d = lo >> 2;
    const uint32_t last = (hi - 1) >> 2;
    uint32_t w = t[d], acc = 0;
    w &= 0xFFFFFFFFu << (8 * (lo & 3));
    while (d < last) {
        acc = __builtin_amdgcn_sad_u8(w, 0u, acc);
        w = t[++d];
    }
    w &= 0xFFFFFFFFu >> (8 * (3 - ((hi - 1) & 3)));
    return __builtin_amdgcn_sad_u8(w, 0u, acc);
}

// a wave's 16-byte pieces into its own LDS tile, then every lane's bins lane, lane + 64, ... out of it into s[].  LDS
// instructions of one wave execute in order, so the wave needs no barrier of the hardware's: the fences only keep the
// compiler from moving the reads over the store (or the next store over the reads).
__device__ __forceinline__ void win_stage_sums(uint32_t *t, int lane, const u32x4 &v, uint32_t r, uint32_t nbins,
                                               uint32_t (&s)[kWinStageLaneBins])
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    reinterpret_cast<u32x4 *>(t)[lane] = v;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (uint32_t j = 0; j < kWinStageLaneBins; ++j) {
        const uint32_t b = (uint32_t)lane + 64u * j;
        s[j] = b < nbins ? win_lds_sum(t, b * r, b * r + r) : 0u;
    }
}

// ---- 2 <= r <= 64: a wave stages a tile of the window, lane l owns the bins l, l + 64, ... of the tile.  The tile is
// zero padded behind the window's end, so the cut last bin needs no bound of its own.
template <bool SUM, bool OUT32, bool SQ>
__global__ __launch_bounds__(kWinThreads) void k_win_stage(const WinParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kWinWaves][kWinStageBytes / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const t = lds[wave];
    const uint64_t stride = (uint64_t)gridDim.x * kWinWaves;
    for (uint64_t item = (uint64_t)blockIdx.x * kWinWaves + wave; item < p.items; item += stride) {
        uint32_t tile, k;
        uint64_t row, off;
        win_split(p, item, tile, row, k);
        const uint32_t b0 = tile * p.tile_bins, nbins = p.nb - b0 < p.tile_bins ? p.nb - b0 : p.tile_bins;
        const uint32_t byte0 = b0 * p.r, tbytes = p.W - byte0 < p.tile_bins * p.r ? p.W - byte0 : p.tile_bins * p.r;
        const uint32_t o = (uint32_t)lane * 16, n = o < tbytes ? (tbytes - o < 16 ? tbytes - o : 16) : 0;
        const uint8_t *const src = p.in + row * p.row_stride + byte0 + o;
        uint32_t s[kWinStageLaneBins];
        if (!SUM) {
            const uint64_t slot = p.win_idx ? p.win_idx[k] : k;
            if (!win_start(p, k, off) || slot >= p.n_out) {  // wave-uniform
                if (tile == 0 && row == 0 && lane == 0) win_refuse(p, k);
                continue;
            }
            win_stage_sums(t, lane, win_load(src + off, n), p.r, nbins, s);
            uint8_t *const dst = p.out + slot * p.out_win_stride + row * p.out_row_stride;
#pragma unroll
            for (uint32_t j = 0; j < kWinStageLaneBins; ++j)
                if ((uint32_t)lane + 64u * j < nbins) win_put<OUT32>(dst, b0 + lane + 64u * j, s[j]);
        } else {
            uint32_t acc[kWinStageLaneBins];
            uint64_t sq[kWinStageLaneBins];
#pragma unroll
            for (uint32_t j = 0; j < kWinStageLaneBins; ++j) acc[j] = 0, sq[j] = 0;
            for (uint64_t k0 = 0; k0 < p.n_win; k0 += kWinUnroll) {
                u32x4 v[kWinUnroll];
#pragma unroll
                for (int u = 0; u < kWinUnroll; ++u) {
                    const uint64_t kk = k0 + u;
                    v[u] = u32x4{0u, 0u, 0u, 0u};
                    if (kk < p.n_win) {
                        if (win_start(p, kk, off))
                            v[u] = win_load(src + off, n);
                        else if (item == 0 && lane == 0)
                            win_refuse(p, kk);
                    }
                }
#pragma unroll
                for (int u = 0; u < kWinUnroll; ++u) {
                    win_stage_sums(t, lane, v[u], p.r, nbins, s);
#pragma unroll
                    for (uint32_t j = 0; j < kWinStageLaneBins; ++j) {
                        acc[j] += s[j];
                        if (SQ) sq[j] += (uint64_t)s[j] * s[j];
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < kWinStageLaneBins; ++j)
                if ((uint32_t)lane + 64u * j < nbins) win_store_sum<SQ>(p, row, b0 + lane + 64u * j, acc[j], sq[j]);
        }
    }
}

// a lane's share of the bin [src, src + len): 16-byte pieces lane, lane + 64, ...
__device__ __forceinline__ uint32_t win_lane_share(const uint8_t *src, uint32_t len, int lane)
{
    uint32_t s = 0;
    for (uint64_t o = (uint64_t)lane * 16; o < len; o += 64 * 16) {
        const uint32_t left = len - (uint32_t)o;
        s = win_sum16(win_load(src + o, left < 16 ? left : 16), s);
    }
    return s;
}

// ---- r > 64: a wave owns a bin
template <bool SUM, bool OUT32, bool SQ>
__global__ __launch_bounds__(kWinThreads) void k_win_wave(const WinParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * kWinWaves;
    for (uint64_t item = (uint64_t)blockIdx.x * kWinWaves + wave; item < p.items; item += stride) {
        uint32_t b, k;
        uint64_t row, off;
        win_split(p, item, b, row, k);
        const uint32_t lo = b * p.r, len = p.W - lo < p.r ? p.W - lo : p.r;  // b < nb: b * r < W
        const uint8_t *const src = p.in + row * p.row_stride + lo;
        if (!SUM) {
            const uint64_t slot = p.win_idx ? p.win_idx[k] : k;
            if (!win_start(p, k, off) || slot >= p.n_out) {  // wave-uniform
                if (b == 0 && row == 0 && lane == 0) win_refuse(p, k);
                continue;
            }
            const uint32_t s = wave_sum_u32(win_lane_share(src + off, len, lane));
            if (lane == 0) win_put<OUT32>(p.out + slot * p.out_win_stride + row * p.out_row_stride, b, s);
        } else {
            uint32_t acc = 0;
            uint64_t sq = 0;
            for (uint32_t kk = 0; kk < p.n_win; ++kk) {
                if (!win_start(p, kk, off)) {  // wave-uniform
                    if (item == 0 && lane == 0) win_refuse(p, kk);
                    continue;
                }
                const uint32_t s = win_lane_share(src + off, len, lane);
                if (SQ) {  // the square is of the window's whole bin: join the lanes per window
                    const uint32_t whole = wave_sum_u32(s);
                    acc += whole;
                    sq += (uint64_t)whole * whole;
                } else {
                    acc += s;  // ... the plain sum joins them once, at the end
                }
            }
            if (!SQ) acc = wave_sum_u32(acc);
            if (lane == 0) win_store_sum<SQ>(p, row, b, acc, sq);
        }
    }
}

}  // namespace mh
