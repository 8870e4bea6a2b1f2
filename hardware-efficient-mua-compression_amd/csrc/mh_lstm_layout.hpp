// mh_lstm_layout.hpp -- the argument rules, the tiles, the scratch and the launch grids of mhl_inproj and mhl_windows
// (include/muahuff_lstm.h): the input half of an LSTM's gate pre-activations, once per bin, and the recurrence over every
// window of `lags` bins.  Pure C++ (no HIP, no device, no global state), as mh_kalman_layout.hpp: mh_lstm.hip checks with
// inproj_check() / windows_check(), launches what inproj_layout() / windows_layout() return, the kernels of mh_lstm.hpp
// find their work with the same functions, and tests/lstm_check.cpp walks all of it under -fsanitize=address,undefined.
//
// mhl_inproj.  p[t][g] is a [cols, 4U] x [rows] product on v_mfma_f32_32x32x2_f32 with TIME as the M dimension.  The
// columns are cut into TILES of kInTileCols = 4 waves x 128; a lane owns 4 consecutive columns (one dword of every
// channel, taken from aligned dwords where both lie inside the row: dwords_ok of mh_rows.hpp, byte by byte otherwise).  The 4U
// pre-activations are cut into G-TILES of 32 (the N dimension).  An ITEM is (tile, g-tile); the grid is capped at
// kInMaxBlocks, workgroup b starts at item b and strides by the grid.  The scratch matrix p holds inproj_bytes(cols,
// units) = cols * 4U * 4 bytes.
//
// mhl_windows.  The cols - lags + 1 windows are cut into TILES of kWinTile = 32 consecutive windows, the N dimension of
// the recurrent product.  The 4U rows of Wh are permuted into BLOCKS of 32: block q holds the four gates of the units
// 8q .. 8q+7, row (r & 3) + 8 (r >> 2) + 4 h of the MFMA's C layout being gate r >> 2 of unit 8q + 4h + (r & 3), so that
// a lane owns all four gates of its units.  Wave w of the kWinThreads / 64 = 8 owns the blocks w and w + 8 (the second
// only where U > 64: WinLayout::per_wave).  The reduction over the previous h runs in ksteps pairs of units, rounded up
// to a multiple of kWinKGroup (the kernel is instantiated per group); the pad multiplies zeros.  The grid is capped at
// kWinMaxBlocks; workgroup b starts at tile b and strides by the grid.
#pragma once
#include <stdint.h>

#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kLstmMaxUnits = 128;
constexpr uint32_t kLstmMaxLags = 32;
constexpr uint32_t kLstmMaxK = 8;
constexpr uint64_t kLstmMaxRows = 65536;

constexpr uint32_t kInThreads = 256;             // 4 waves
constexpr uint32_t kInWaveCols = 128;            // 32 lanes x 4 bytes of a dword
constexpr uint32_t kInTileCols = kInWaveCols * (kInThreads / 64);
constexpr uint32_t kInGTile = 32;                // pre-activations of a g-tile: the MFMA's N
constexpr uint32_t kInMaxBlocks = 8192;          // the grid is capped; the kernel strides

constexpr uint32_t kWinThreads = 512;            // 8 waves
constexpr uint32_t kWinWaves = kWinThreads / 64;
constexpr uint32_t kWinTile = 32;                // windows of a tile: the MFMA's N
constexpr uint32_t kWinBlockUnits = 8;           // units of a block of 32 permuted rows
constexpr uint32_t kWinKGroup = 8;               // k-steps (pairs of units) come in groups of this
constexpr uint32_t kWinMaxBlocks = 4096;         // the grid is capped; the kernel strides

// the arguments, pointers as plain addresses: nothing here reads through them
struct InprojArgs {
    uint64_t x, x_row_stride, rows, cols;
    uint32_t clip;
    uint64_t wx, bias;
    uint32_t units;
    uint64_t p;
};

struct WindowsArgs {
    uint64_t p, cols;
    uint32_t lags, units;
    uint64_t wh, wd, bd;
    uint32_t k;
    uint64_t out, out_row_stride;
};

struct InprojLayout {
    uint64_t tiles;   // ceil(cols / kInTileCols)
    uint32_t gtiles;  // ceil(4 units / kInGTile)
    uint64_t items;   // tiles * gtiles
    uint32_t grid;
};

struct WinLayout {
    uint64_t windows;   // cols - lags + 1
    uint64_t tiles;     // ceil(windows / kWinTile)
    uint32_t blocks;    // ceil(units / kWinBlockUnits), at most 2 * kWinWaves
    uint32_t per_wave;  // 1 or 2: blocks a wave may own
    uint32_t ksteps;    // ceil(units / 2) rounded up to a multiple of kWinKGroup
    uint32_t grid;
};

MH_HD inline uint64_t inproj_bytes(uint64_t cols, uint32_t units) { return cols * 16ull * units; }  // below 2^51

// ---- mhl_inproj -------------------------------------------------------------------------------------------------------------
inline void inproj_layout(uint64_t cols, uint32_t units, InprojLayout *L)
{
    L->tiles = (cols + kInTileCols - 1) / kInTileCols;  // below 2^31
    L->gtiles = (4 * units + kInGTile - 1) / kInGTile;  // at most 16
    L->items = L->tiles * L->gtiles;
    L->grid = (uint32_t)(L->items < kInMaxBlocks ? L->items : kInMaxBlocks);
}

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int inproj_check(Msg &m, const InprojArgs &a)
{
    if (!a.x || !a.wx || !a.bias || !a.p) return m.set(MH_ERR_ARG, "mhl_inproj: NULL pointer");
    if (a.units < 1 || a.units > kLstmMaxUnits) return m.set(MH_ERR_ARG, "mhl_inproj: units=%u outside 1..%u", a.units, kLstmMaxUnits);
    if (int rc = rows_rule(m, "mhl_inproj", a.rows, kLstmMaxRows)) return rc;
    if (int rc = cols_rule(m, "mhl_inproj", a.cols)) return rc;
    if (int rc = clip_rule(m, "mhl_inproj", a.clip)) return rc;
    if (a.wx % 4 || a.bias % 4 || a.p % 4) return m.set(MH_ERR_ARG, "mhl_inproj: wx, bias and p must be multiples of 4");
    if (a.rows > 1 && (a.x_row_stride < a.cols || a.x_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhl_inproj: x_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.x_row_stride, (unsigned long long)a.cols);
    const uint64_t x_end = strided_end(a.x, a.rows, a.x_row_stride, a.cols);
    const uint64_t p_end = a.p + inproj_bytes(a.cols, a.units);
    if (ranges_overlap(a.p, p_end, a.x, x_end) || ranges_overlap(a.p, p_end, a.wx, a.wx + 16ull * a.units * a.rows) ||
        ranges_overlap(a.p, p_end, a.bias, a.bias + 16ull * a.units))
        return m.set(MH_ERR_ARG, "mhl_inproj: p overlaps x, wx or bias");
    return MH_OK;
}

// ---- mhl_windows ------------------------------------------------------------------------------------------------------------
inline void windows_layout(uint64_t cols, uint32_t lags, uint32_t units, WinLayout *L)
{
    L->windows = cols - lags + 1;
    L->tiles = (L->windows + kWinTile - 1) / kWinTile;  // below 2^35
    L->blocks = (units + kWinBlockUnits - 1) / kWinBlockUnits;
    L->per_wave = L->blocks > kWinWaves ? 2 : 1;
    L->ksteps = ((units + 1) / 2 + kWinKGroup - 1) / kWinKGroup * kWinKGroup;
    L->grid = (uint32_t)(L->tiles < kWinMaxBlocks ? L->tiles : kWinMaxBlocks);
}

// the unit and the gate of register r (0..15) of lane half h (0..1) in block q
MH_HD inline uint32_t win_unit(uint32_t q, uint32_t h, uint32_t r) { return q * kWinBlockUnits + 4 * h + (r & 3); }
MH_HD inline uint32_t win_gate(uint32_t r) { return r >> 2; }
// the permuted row m (0..31) of block q as a row g = gate * units + unit of Wh; units <= unit: a row of zeros
MH_HD inline uint32_t win_row_unit(uint32_t q, uint32_t m) { return q * kWinBlockUnits + (m & 7); }
MH_HD inline uint32_t win_row_gate(uint32_t m) { return m >> 3; }

inline int windows_check(Msg &m, const WindowsArgs &a)
{
    if (!a.p || !a.wh || !a.wd || !a.bd || !a.out) return m.set(MH_ERR_ARG, "mhl_windows: NULL pointer");
    if (a.units < 1 || a.units > kLstmMaxUnits) return m.set(MH_ERR_ARG, "mhl_windows: units=%u outside 1..%u", a.units, kLstmMaxUnits);
    if (a.lags < 1 || a.lags > kLstmMaxLags) return m.set(MH_ERR_ARG, "mhl_windows: lags=%u outside 1..%u", a.lags, kLstmMaxLags);
    if (int rc = k_rule(m, "mhl_windows", a.k, kLstmMaxK)) return rc;
    if (a.cols < a.lags || a.cols >= kMaxCols)
        return m.set(MH_ERR_ARG, "mhl_windows: cols=%llu outside lags=%u..2^40-1", (unsigned long long)a.cols, a.lags);
    if (a.p % 4 || a.wh % 4 || a.wd % 4 || a.bd % 4 || a.out % 4 || a.out_row_stride % 4)
        return m.set(MH_ERR_ARG, "mhl_windows: p, wh, wd, bd, out and out_row_stride must be multiples of 4");
    const uint64_t row = 4 * (a.cols - a.lags + 1);
    if (a.k > 1 && (a.out_row_stride < row || a.out_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhl_windows: out_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.out_row_stride, (unsigned long long)row);
    const uint64_t out_end = strided_end(a.out, a.k, a.out_row_stride, row);
    const uint64_t uu = 4ull * a.units;
    if (ranges_overlap(a.out, out_end, a.p, a.p + inproj_bytes(a.cols, a.units)) || ranges_overlap(a.out, out_end, a.wh, a.wh + 4 * uu * a.units) ||
        ranges_overlap(a.out, out_end, a.wd, a.wd + uu * a.k) || ranges_overlap(a.out, out_end, a.bd, a.bd + 4ull * a.k))
        return m.set(MH_ERR_ARG, "mhl_windows: out overlaps p, wh, wd or bd");
    return MH_OK;
}

}  // namespace mh
