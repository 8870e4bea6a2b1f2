// mh_windows_layout.hpp -- the argument rules, the form and tile choice and the launch grid of mhi_windows
// (include/muahuff_ingest.h): many windows [win_off[k], win_off[k] + W) of every row of a uint8 matrix, re-binned by r on
// each window's own grid, stacked or summed over the windows.  Pure C++ (no HIP, no device, no global state), as
// mh_excess_layout.hpp: mh_ingest.hip checks with windows_check(), launches what windows_layout() returns, and
// tests/windows_check.cpp prints both under -fsanitize=address,undefined.
//
// nb = ceil(W / r) bins per window and row; the last one may be cut.  A TILE is the run of bins one owner handles:
//   kWinLane   r == 1         a lane owns 16 consecutive samples (one unaligned 16-byte load per window):
//                             tile_bins = 16, tiles = ceil(W / 16), an item is a lane.
//   kWinStage  2 <= r <= 64   a wave stages tile_bins * r <= 1024 bytes of the window in LDS with one 16-byte load per
//                             lane, and lane l owns the bins l, l + 64, ... of the tile (at most kWinStageLaneBins):
//                             tile_bins = 1024 / r (16 .. 512), an item is a wave.
//   kWinWave   r > 64         a wave owns one bin; its lanes sum 16-byte pieces and a DPP ladder joins them:
//                             tile_bins = 1, tiles = nb, an item is a wave.
// STACK: items = n_win * rows * tiles, item = (k * rows + row) * tiles + tile.  SUM: items = rows * tiles (the owner walks
// the windows itself), item = row * tiles + tile.
// The grid: workgroups of 256 threads -- 256 lane items or 4 wave items -- capped at kWinMaxBlocks; the kernels stride
// item += gridDim.x * (256 or 4).
#pragma once
#include <stdint.h>

#include "mh_msg.hpp"
#include "muahuff.h"

namespace mh {

constexpr uint32_t kWinStack = 0;  // == MHI_WIN_STACK
constexpr uint32_t kWinSum = 1;    // == MHI_WIN_SUM
constexpr uint32_t kWinLane = 0, kWinStage = 1, kWinWave = 2;  // the forms
constexpr uint32_t kWinLaneBytes = 16;     // samples of a lane (r == 1)
constexpr uint32_t kWinStageBytes = 1024;  // bytes a wave stages: 64 lanes x 16
constexpr uint32_t kWinStageMaxR = 64;     // the largest r of the staged form: its tiles still hold 16 bins
constexpr uint32_t kWinStageLaneBins = 8;  // bins of a tile one lane owns at most: r = 2 puts 512 bins into a tile
static_assert(kWinStageBytes / 2 <= 64 * kWinStageLaneBins && kWinStageBytes / kWinStageMaxR >= 16, "the staged form's tiles");
constexpr uint32_t kWinThreads = 256;      // threads of a workgroup, every form
constexpr uint32_t kWinWaves = kWinThreads / 64;
constexpr uint32_t kWinMaxBlocks = 4096;   // the grid is capped; the kernels stride
constexpr uint64_t kWinMax32 = 1ull << 32; // W, r and n_win are below this

// mhi_windows' arguments, pointers as plain addresses: nothing here reads through them
struct WinArgs {
    uint64_t in, row_stride, rows, cols;
    uint64_t win_off, win_idx, n_win, n_out, W, r;
    uint32_t mode;
    uint64_t out;
    uint32_t out_bits;
    uint64_t out_win_stride, out_row_stride;
    uint64_t sumsq, sq_row_stride;
    uint32_t accumulate;
    uint64_t bad;
};

struct WinLayout {
    uint32_t form;       // kWinLane / kWinStage / kWinWave
    uint32_t nb;         // ceil(W / r)
    uint32_t tile_bins;  // bins of a tile
    uint32_t tiles;      // ceil(nb / tile_bins)
    uint64_t items;      // lanes (kWinLane) or waves that own a tile
    uint32_t per_block;  // items of a workgroup: 256 or 4
    uint32_t grid;       // min(ceil(items / per_block), kWinMaxBlocks); 0 when there are no items
};

inline uint64_t win_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int windows_check(Msg &m, const WinArgs &a)
{
    if (!a.in || !a.out || !a.bad || (a.n_win && !a.win_off)) return m.set(MH_ERR_ARG, "mhi_windows: NULL pointer");
    if (a.mode != kWinStack && a.mode != kWinSum)
        return m.set(MH_ERR_ARG, "mhi_windows: mode=%u (MHI_WIN_STACK or MHI_WIN_SUM)", a.mode);
    if (a.mode == kWinStack) {
        if (a.out_bits != 8 && a.out_bits != 32)
            return m.set(MH_ERR_ARG, "mhi_windows: out_bits=%u (8 or 32 in the STACK form)", a.out_bits);
        if (a.sumsq || a.accumulate)
            return m.set(MH_ERR_ARG, "mhi_windows: the STACK form takes no sumsq and no accumulate");
    } else {
        if (a.out_bits != 32) return m.set(MH_ERR_ARG, "mhi_windows: out_bits=%u (32 in the SUM form)", a.out_bits);
        if (a.accumulate > 1) return m.set(MH_ERR_ARG, "mhi_windows: accumulate=%u (0 or 1)", a.accumulate);
    }
    if (a.rows == 0 || a.cols == 0 || a.W == 0 || a.r == 0)
        return m.set(MH_ERR_ARG, "mhi_windows: rows=%llu, cols=%llu, W=%llu, r=%llu (each at least 1)", (unsigned long long)a.rows,
                     (unsigned long long)a.cols, (unsigned long long)a.W, (unsigned long long)a.r);
    if (a.W >= kWinMax32 || a.r >= kWinMax32 || a.n_win >= kWinMax32)
        return m.set(MH_ERR_ARG, "mhi_windows: W=%llu, r=%llu, n_win=%llu (each below 2^32)", (unsigned long long)a.W,
                     (unsigned long long)a.r, (unsigned long long)a.n_win);
    if (a.rows > 1 && a.row_stride < a.cols)
        return m.set(MH_ERR_ARG, "mhi_windows: row_stride=%llu is below cols=%llu", (unsigned long long)a.row_stride,
                     (unsigned long long)a.cols);
    if (a.out_bits == 32 && (a.out % 4 || a.out_row_stride % 4 || (a.mode == kWinStack && a.out_win_stride % 4)))
        return m.set(MH_ERR_ARG, "mhi_windows: out_bits=32 needs out and its strides to be multiples of 4");
    if (a.sumsq && (a.sumsq % 8 || a.sq_row_stride % 8))
        return m.set(MH_ERR_ARG, "mhi_windows: sumsq and sq_row_stride must be multiples of 8");
    if (a.mode == kWinSum && !a.accumulate && (unsigned __int128)a.n_win * 255 * win_min(a.r, a.W) >= kWinMax32)
        return m.set(MH_ERR_ARG, "mhi_windows: n_win=%llu windows of bins of %llu samples can exceed 32 bits",
                     (unsigned long long)a.n_win, (unsigned long long)win_min(a.r, a.W));
    const uint64_t tiles = a.r == 1 ? (a.W + kWinLaneBytes - 1) / kWinLaneBytes : (a.W + a.r - 1) / a.r;  // an upper bound
    const unsigned __int128 items = (unsigned __int128)(a.mode == kWinStack && a.n_win ? a.n_win : 1) * a.rows * tiles;
    if (items >= ((unsigned __int128)1 << 63)) return m.set(MH_ERR_ARG, "mhi_windows: rows=%llu is too large", (unsigned long long)a.rows);
    return MH_OK;
}

// the form and the tile of (W, r); the caller has checked 1 <= W, r < 2^32
inline void windows_tile(uint64_t W, uint64_t r, WinLayout *L)
{
    L->nb = (uint32_t)((W + r - 1) / r);
    if (r == 1) {
        L->form = kWinLane, L->tile_bins = kWinLaneBytes;
    } else if (r <= kWinStageMaxR) {
        L->form = kWinStage, L->tile_bins = kWinStageBytes / (uint32_t)r;
    } else {
        L->form = kWinWave, L->tile_bins = 1;
    }
    L->tiles = (uint32_t)(((uint64_t)L->nb + L->tile_bins - 1) / L->tile_bins);  // (nb + 15 does not fit 32 bits at W = 2^32 - 1)
}

// the whole layout; the caller has passed windows_check.  STACK with n_win == 0 has no items and no grid.
inline void windows_layout(uint32_t mode, uint64_t rows, uint64_t W, uint64_t r, uint64_t n_win, WinLayout *L)
{
    windows_tile(W, r, L);
    L->items = (mode == kWinStack ? n_win : 1) * rows * L->tiles;
    L->per_block = L->form == kWinLane ? kWinThreads : kWinWaves;
    const uint64_t blocks = (L->items + L->per_block - 1) / L->per_block;
    L->grid = (uint32_t)(blocks < kWinMaxBlocks ? blocks : kWinMaxBlocks);
}

}  // namespace mh
