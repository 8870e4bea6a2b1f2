// mh_wiener_layout.hpp -- the argument rules, the runs, the tiles and the launch grids of mhw_xty and mhw_fir
// (include/muahuff_wiener.h): a lagged linear decoder on uint8 counts, its cross products with float covariates and its
// prediction.  Pure C++ (no HIP, no device, no global state), as mh_gram_layout.hpp: mh_wiener.hip checks with
// xty_check() / fir_check(), launches what xty_layout() / fir_layout() return, the kernels of mh_wiener.hpp find their
// work with the same functions, and tests/wiener_check.cpp walks all of it under -fsanitize=address,undefined.
//
// mhw_xty.  The columns are cut into RUNS of kXtyRun; an ITEM is one (run, channel): item = run * rows + channel, so the
// items next to each other read the same columns of y.  A workgroup takes an item at a time, walks the lags in blocks of
// kXtyLagBlock (the accumulators of a block live in registers) and stores the item's lags * k partial sums at
// scratch[item * lags * k + l * k + j].  The grid is capped at kXtyMaxBlocks; workgroup b starts at item b and strides
// by the grid.  The second kernel has one thread per (channel, lag, covariate) ELEMENT, which adds that element's runs
// in run order; its grid is capped at kXtySumMaxBlocks and strides too.
//
// mhw_fir.  A P COLUMN is a column of x (cols + lags - 1 of them); output i is the diagonal sum over the P columns
// i .. i + lags - 1.  A wave owns kFirWaveCols P columns, the kFirWaves waves of a workgroup consecutive ones, so a
// WORKGROUP TILE is kFirTileCols P columns and yields fir_tile_outputs(lags) = kFirTileCols - (lags - 1) outputs:
// consecutive tiles overlap by lags - 1 P columns and every output has one owner.  An M-TILE is the 32 rows of the
// matrix instruction: floor(32 / lags) whole outputs of lags rows each, the remaining rows zero.  An ITEM is one
// (workgroup tile, M-tile): item = tile * mtiles + mtile, so the M-tiles of one tile -- which read the same bytes of x --
// run next to each other.  The grid is capped at kFirMaxBlocks and strides.
#pragma once
#include <stdint.h>

#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kWienerMaxLags = 32;
constexpr uint32_t kWienerMaxK = 8;
constexpr uint64_t kWienerMaxRows = 65536;

constexpr uint32_t kXtyThreads = 256;       // 4 waves
constexpr uint32_t kXtyRun = 32768;         // columns of a run
constexpr uint32_t kXtyLagBlock = 8;        // lags a pass over the run keeps in registers
constexpr uint32_t kXtyMaxBlocks = 4096;    // the grid is capped; the kernel strides
constexpr uint32_t kXtySumThreads = 256;
constexpr uint32_t kXtySumMaxBlocks = 4096;
static_assert(kXtyRun % kXtyThreads == 0, "every thread of a workgroup walks the same number of columns of a full run");

constexpr uint32_t kFirWaves = 4;
constexpr uint32_t kFirThreads = 64 * kFirWaves;
constexpr uint32_t kFirWaveCols = 128;      // 32 columns of the matrix instruction x 4 byte positions of a dword
constexpr uint32_t kFirTileCols = kFirWaveCols * kFirWaves;
constexpr uint32_t kFirMRows = 32;          // rows of v_mfma_f32_32x32x2_f32
constexpr uint32_t kFirMaxBlocks = 4096;    // the grid is capped; the kernel strides
static_assert(kWienerMaxLags <= kFirMRows && kWienerMaxLags <= kFirTileCols, "an output's lags fit one M-tile and one tile");

// the arguments, pointers as plain addresses: nothing here reads through them
struct XtyArgs {
    uint64_t x, x_row_stride, rows, cols;
    uint32_t lags, clip;
    uint64_t y, y_row_stride;
    uint32_t k;
    uint64_t out;
    uint32_t accumulate;
    uint64_t scratch, scratch_bytes;
};

struct FirArgs {
    uint64_t x, x_row_stride, rows, cols;
    uint32_t lags, clip;
    uint64_t w, bias;
    uint32_t k;
    uint64_t out, out_row_stride;
};

struct XtyLayout {
    uint64_t runs;       // ceil(cols / kXtyRun)
    uint64_t items;      // runs * rows
    uint32_t per_item;   // lags * k partial sums
    uint64_t scratch_bytes;
    uint32_t grid;       // of the first kernel
    uint64_t elements;   // rows * lags * k
    uint32_t sum_grid;   // of the second
};

struct FirLayout {
    uint32_t tile_outputs;  // outputs of a workgroup tile
    uint64_t tiles;         // ceil(cols / tile_outputs)
    uint32_t per_mtile;     // whole outputs of an M-tile
    uint32_t mtiles;        // ceil(k / per_mtile)
    uint64_t items;         // tiles * mtiles
    uint32_t grid;
};

// the limits the two calls and the scratch size share; `fn` names the call
inline int wiener_shape_check(Msg &m, const char *fn, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k)
{
    if (lags < 1 || lags > kWienerMaxLags) return m.set(MH_ERR_ARG, "%s: lags=%u outside 1..%u", fn, lags, kWienerMaxLags);
    if (int rc = k_rule(m, fn, k, kWienerMaxK)) return rc;
    if (int rc = rows_rule(m, fn, rows, kWienerMaxRows)) return rc;
    return cols_rule(m, fn, cols);
}

// the whole layout of mhw_xty; the shape has passed wiener_shape_check
inline void xty_layout(uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, XtyLayout *L)
{
    L->runs = (cols + kXtyRun - 1) / kXtyRun;
    L->items = L->runs * rows;  // below 2^25 * 2^16
    L->per_item = lags * k;
    L->scratch_bytes = L->items * L->per_item * 8;  // below 2^41 * 2^8 * 2^3
    L->grid = (uint32_t)(L->items < kXtyMaxBlocks ? L->items : kXtyMaxBlocks);
    L->elements = rows * L->per_item;
    const uint64_t blocks = (L->elements + kXtySumThreads - 1) / kXtySumThreads;
    L->sum_grid = (uint32_t)(blocks < kXtySumMaxBlocks ? blocks : kXtySumMaxBlocks);
}

// the columns [c0, c1) of a run
MH_HD inline void xty_run_cols(uint64_t run, uint64_t cols, uint64_t *c0, uint64_t *c1)
{
    *c0 = run * kXtyRun;
    *c1 = cols - *c0 < kXtyRun ? cols : *c0 + kXtyRun;
}

inline int xty_scratch_check(Msg &m, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint64_t bytes_ptr)
{
    if (int rc = wiener_shape_check(m, "mhw_xty_scratch_bytes", rows, cols, lags, k)) return rc;
    if (!bytes_ptr) return m.set(MH_ERR_ARG, "mhw_xty_scratch_bytes: NULL pointer");
    return MH_OK;
}

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int xty_check(Msg &m, const XtyArgs &a)
{
    if (!a.x || !a.y || !a.out || !a.scratch) return m.set(MH_ERR_ARG, "mhw_xty: NULL pointer");
    if (int rc = wiener_shape_check(m, "mhw_xty", a.rows, a.cols, a.lags, a.k)) return rc;
    if (int rc = clip_rule(m, "mhw_xty", a.clip)) return rc;
    if (a.accumulate > 1) return m.set(MH_ERR_ARG, "mhw_xty: accumulate=%u (0 or 1)", a.accumulate);
    if (a.out % 8 || a.scratch % 8) return m.set(MH_ERR_ARG, "mhw_xty: out and scratch must be multiples of 8");
    if (a.y % 4 || a.y_row_stride % 4) return m.set(MH_ERR_ARG, "mhw_xty: y and y_row_stride must be multiples of 4");
    if (a.rows > 1 && a.x_row_stride < a.cols + a.lags - 1)
        return m.set(MH_ERR_ARG, "mhw_xty: x_row_stride=%llu is below the cols + lags - 1 = %llu bytes of a row",
                     (unsigned long long)a.x_row_stride, (unsigned long long)(a.cols + a.lags - 1));
    if (a.k > 1 && a.y_row_stride < 4 * a.cols)
        return m.set(MH_ERR_ARG, "mhw_xty: y_row_stride=%llu is below the %llu bytes of a row", (unsigned long long)a.y_row_stride,
                     (unsigned long long)(4 * a.cols));
    XtyLayout L;
    xty_layout(a.rows, a.cols, a.lags, a.k, &L);
    if (a.scratch_bytes < L.scratch_bytes)
        return m.set(MH_ERR_ARG, "mhw_xty: scratch_bytes=%llu is below the %llu that mhw_xty_scratch_bytes asks for",
                     (unsigned long long)a.scratch_bytes, (unsigned long long)L.scratch_bytes);
    return MH_OK;
}

MH_HD inline uint32_t fir_tile_outputs(uint32_t lags) { return kFirTileCols - (lags - 1); }
MH_HD inline uint32_t fir_per_mtile(uint32_t lags) { return kFirMRows / lags; }

// the whole layout of mhw_fir; the shape has passed wiener_shape_check
inline void fir_layout(uint64_t cols, uint32_t lags, uint32_t k, FirLayout *L)
{
    L->tile_outputs = fir_tile_outputs(lags);
    L->tiles = (cols + L->tile_outputs - 1) / L->tile_outputs;
    L->per_mtile = fir_per_mtile(lags);
    L->mtiles = (k + L->per_mtile - 1) / L->per_mtile;
    L->items = L->tiles * L->mtiles;  // below 2^32 * 2^3
    L->grid = (uint32_t)(L->items < kFirMaxBlocks ? L->items : kFirMaxBlocks);
}

inline int fir_check(Msg &m, const FirArgs &a)
{
    if (!a.x || !a.w || !a.bias || !a.out) return m.set(MH_ERR_ARG, "mhw_fir: NULL pointer");
    if (int rc = wiener_shape_check(m, "mhw_fir", a.rows, a.cols, a.lags, a.k)) return rc;
    if (int rc = clip_rule(m, "mhw_fir", a.clip)) return rc;
    if (a.w % 4 || a.bias % 4) return m.set(MH_ERR_ARG, "mhw_fir: w and bias must be multiples of 4");
    if (a.out % 4 || a.out_row_stride % 4) return m.set(MH_ERR_ARG, "mhw_fir: out and out_row_stride must be multiples of 4");
    if (a.rows > 1 && a.x_row_stride < a.cols + a.lags - 1)
        return m.set(MH_ERR_ARG, "mhw_fir: x_row_stride=%llu is below the cols + lags - 1 = %llu bytes of a row",
                     (unsigned long long)a.x_row_stride, (unsigned long long)(a.cols + a.lags - 1));
    if (a.k > 1 && a.out_row_stride < 4 * a.cols)
        return m.set(MH_ERR_ARG, "mhw_fir: out_row_stride=%llu is below the %llu bytes of a row", (unsigned long long)a.out_row_stride,
                     (unsigned long long)(4 * a.cols));
    return MH_OK;
}

}  // namespace mh
