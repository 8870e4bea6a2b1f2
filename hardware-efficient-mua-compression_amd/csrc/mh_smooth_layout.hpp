// mh_smooth_layout.hpp -- the argument rules, the tiles, the halos and the launch grids of mhs_box and mhs_box_f32
// (include/muahuff_smooth.h): the box sums of clipped counts as byte planes and the trailing box sum of a float
// prediction.  Pure C++ (no HIP, no device, no global state), as mh_wiener_layout.hpp: mh_smooth.hip checks with
// box_check() / boxf_check(), launches what box_layout() / boxf_layout() return, the kernels of mh_smooth.hpp find their
// work with the same functions, and tests/box_check.cpp walks all of it under -fsanitize=address,undefined.
//
// mhs_box.  The output columns of a row are cut into TILES of kBoxTileCols; an ITEM is one (channel, tile):
// item = channel * tiles + tile, so the items next to each other stream along one row.  A tile of n outputs reads the
// n + window - 1 bytes from its first column on (the last window - 1 are its HALO, which the next tile reads again).
// The workgroup loads them as the aligned 16-byte GROUPS that hold them, thread t the group at SPAN position 16 t, where
// position 0 is the tile's first byte rounded down to a multiple of 16 (`shift` = 0..15 bytes in front of it): the span
// of kBoxSpan = 16 * kBoxThreads positions covers shift + kBoxTileCols + kBoxMaxWindow - 1.  Of a group only the dwords
// that hold a byte of the row are loaded (box_dword_ok), a whole group at once where all four do.  Output o of the tile
// is P[shift + o + window] - P[shift + o] of the exclusive prefix sums P over the span, kept modulo 2^16.  The grid is
// capped at kBoxMaxBlocks; workgroup b starts at item b and strides by the grid.
//
// mhs_box_f32.  The columns are cut into TILES of kBoxfTile, one thread per column; an ITEM is one (tile, output):
// item = tile * k + j.  The grid is capped at kBoxfMaxBlocks and strides.
#pragma once
#include <stdint.h>

#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kBoxMaxWindow = 256;
constexpr uint64_t kBoxMaxRows = 65536;

constexpr uint32_t kBoxThreads = 256;           // 4 waves
constexpr uint32_t kBoxGroup = 16;              // bytes a thread loads
constexpr uint32_t kBoxSpan = kBoxGroup * kBoxThreads;
constexpr uint32_t kBoxTileCols = 3824;         // output columns of a tile: a multiple of 16, so every tile's stores are aligned
constexpr uint32_t kBoxMaxBlocks = 2048;        // the grid is capped; the kernel strides
static_assert(kBoxTileCols % kBoxGroup == 0, "a tile starts on a 16-byte boundary of the output rows");
static_assert(kBoxGroup - 1 + kBoxTileCols + kBoxMaxWindow - 1 <= kBoxSpan, "the span holds the shift, the tile and the halo");

constexpr uint32_t kBoxfMaxK = 8;
constexpr uint32_t kBoxfThreads = 256;
constexpr uint32_t kBoxfTile = kBoxfThreads;    // columns of a tile: one per thread
constexpr uint32_t kBoxfMaxBlocks = 4096;

// the arguments, pointers as plain addresses: nothing here reads through them
struct BoxArgs {
    uint64_t x, x_row_stride, rows, cols;
    uint32_t window, clip;
    uint64_t lo, hi, out_row_stride;
};

struct BoxfArgs {
    uint64_t in, in_row_stride;
    uint32_t k;
    uint64_t cols;
    uint32_t window;
    uint64_t bias, out, out_row_stride;
};

struct BoxLayout {
    uint64_t tiles;   // ceil(cols / kBoxTileCols), per row
    uint64_t items;   // rows * tiles
    uint32_t planes;  // 1 (hi is NULL) or 2
    uint32_t grid;
};

struct BoxfLayout {
    uint64_t tiles;  // ceil(cols / kBoxfTile)
    uint64_t items;  // tiles * k
    uint32_t grid;
};

// the whole layout of mhs_box; the shape has passed box_check
inline void box_layout(uint64_t rows, uint64_t cols, bool two_planes, BoxLayout *L)
{
    L->tiles = (cols + kBoxTileCols - 1) / kBoxTileCols;
    L->items = rows * L->tiles;  // below 2^16 * 2^29
    L->planes = two_planes ? 2 : 1;
    L->grid = (uint32_t)(L->items < kBoxMaxBlocks ? L->items : kBoxMaxBlocks);
}

// the channel and the tile of an item
MH_HD inline void box_item(uint64_t item, uint64_t tiles, uint64_t *c, uint64_t *tile)
{
    *c = item / tiles;
    *tile = item - *c * tiles;
}

// the first output column i0 of a tile and its number of outputs; it reads the columns [i0, i0 + n + window - 1) of x
MH_HD inline uint32_t box_tile_outputs(uint64_t tile, uint64_t cols, uint64_t *i0)
{
    *i0 = tile * kBoxTileCols;
    return cols - *i0 < kBoxTileCols ? (uint32_t)(cols - *i0) : kBoxTileCols;
}

// May the aligned dword at address a be loaded?  Only if it holds a byte of the row [row, row_end) and a byte the tile
// needs, [row, need_end) with need_end <= row_end: so no dword without a byte of the row is ever touched.
MH_HD inline bool box_dword_ok(uint64_t a, uint64_t row, uint64_t need_end) { return a + 4 > row && a < need_end; }

// Do two planes of `rows` rows of `cols` bytes, both `stride` apart, share a byte?  Row by row, not as two ranges: planes
// whose rows interleave (hi's rows in the gaps of lo's pitch) are apart.  stride >= cols where rows > 1.
inline bool planes_overlap(uint64_t a, uint64_t b, uint64_t rows, uint64_t stride, uint64_t cols)
{
    const uint64_t d = a < b ? b - a : a - b;
    if (rows == 1) return d < cols;
    const uint64_t q = d / stride, r = d - q * stride;  // the later plane's row 0 starts r bytes into the other's row q
    return (q < rows && r < cols) || (q + 1 < rows && stride - r < cols);
}

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int box_check(Msg &m, const BoxArgs &a)
{
    if (!a.x || !a.lo) return m.set(MH_ERR_ARG, "mhs_box: NULL pointer");
    if (a.window < 1 || a.window > kBoxMaxWindow) return m.set(MH_ERR_ARG, "mhs_box: window=%u outside 1..%u", a.window, kBoxMaxWindow);
    if (int rc = clip_rule(m, "mhs_box", a.clip)) return rc;
    if (int rc = rows_rule(m, "mhs_box", a.rows, kBoxMaxRows)) return rc;
    if (int rc = cols_rule(m, "mhs_box", a.cols)) return rc;
    if (!a.hi && a.window * a.clip > 255)
        return m.set(MH_ERR_ARG, "mhs_box: hi is NULL and window * clip = %u is above 255", a.window * a.clip);
    if (a.lo % 16 || a.hi % 16 || a.out_row_stride % 16) return m.set(MH_ERR_ARG, "mhs_box: lo, hi and out_row_stride must be multiples of 16");
    const uint64_t in_row = a.cols + a.window - 1;
    if (a.rows > 1 && (a.x_row_stride < in_row || a.x_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhs_box: x_row_stride=%llu is below the cols + window - 1 = %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.x_row_stride, (unsigned long long)in_row);
    if (a.rows > 1 && (a.out_row_stride < a.cols || a.out_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhs_box: out_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.out_row_stride, (unsigned long long)a.cols);
    const uint64_t x_end = strided_end(a.x, a.rows, a.x_row_stride, in_row);
    const uint64_t out_len = strided_end(0, a.rows, a.out_row_stride, a.cols);
    if (ranges_overlap(a.lo, a.lo + out_len, a.x, x_end) || (a.hi && ranges_overlap(a.hi, a.hi + out_len, a.x, x_end)))
        return m.set(MH_ERR_ARG, "mhs_box: lo or hi overlaps x");
    if (a.hi && planes_overlap(a.lo, a.hi, a.rows, a.out_row_stride, a.cols)) return m.set(MH_ERR_ARG, "mhs_box: lo and hi overlap");
    return MH_OK;
}

// the whole layout of mhs_box_f32; the shape has passed boxf_check
inline void boxf_layout(uint64_t cols, uint32_t k, BoxfLayout *L)
{
    L->tiles = (cols + kBoxfTile - 1) / kBoxfTile;
    L->items = L->tiles * k;  // below 2^32 * 2^3
    L->grid = (uint32_t)(L->items < kBoxfMaxBlocks ? L->items : kBoxfMaxBlocks);
}

inline int boxf_check(Msg &m, const BoxfArgs &a)
{
    if (!a.in || !a.bias || !a.out) return m.set(MH_ERR_ARG, "mhs_box_f32: NULL pointer");
    if (int rc = k_rule(m, "mhs_box_f32", a.k, kBoxfMaxK)) return rc;
    if (int rc = cols_rule(m, "mhs_box_f32", a.cols)) return rc;
    if (a.window < 1 || a.window > kBoxMaxWindow)
        return m.set(MH_ERR_ARG, "mhs_box_f32: window=%u outside 1..%u", a.window, kBoxMaxWindow);
    if (a.in % 4 || a.in_row_stride % 4 || a.out % 4 || a.out_row_stride % 4)
        return m.set(MH_ERR_ARG, "mhs_box_f32: in, out and their row strides must be multiples of 4");
    if (a.bias % 4) return m.set(MH_ERR_ARG, "mhs_box_f32: bias must be a multiple of 4");
    const uint64_t row = 4 * a.cols;
    if (a.k > 1 && (a.in_row_stride < row || a.out_row_stride < row || a.in_row_stride >= kMaxStride || a.out_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhs_box_f32: in_row_stride=%llu or out_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.in_row_stride, (unsigned long long)a.out_row_stride, (unsigned long long)row);
    const uint64_t in_end = strided_end(a.in, a.k, a.in_row_stride, row);
    const uint64_t out_end = strided_end(a.out, a.k, a.out_row_stride, row);
    if (ranges_overlap(a.out, out_end, a.in, in_end)) return m.set(MH_ERR_ARG, "mhs_box_f32: out overlaps in");
    if (ranges_overlap(a.out, out_end, a.bias, a.bias + 4ull * a.k)) return m.set(MH_ERR_ARG, "mhs_box_f32: out overlaps bias");
    return MH_OK;
}

}  // namespace mh
