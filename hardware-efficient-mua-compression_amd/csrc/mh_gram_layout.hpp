// mh_gram_layout.hpp -- the argument rules, the tiles, the K slices and the launch grid of mhi_gram
// (include/muahuff_ingest.h): gram[i][j] = sum over t of a[i][t] * b[j][t] on uint8 counts, exact in int64, on the int8
// matrix cores.  Pure C++ (no HIP, no device, no global state), as mh_windows_layout.hpp: mh_ingest.hip checks with
// gram_check(), launches what gram_layout() returns, the kernel of mh_gram.hpp finds its work with gram_owner(), and
// tests/gram_check.cpp walks all of it under -fsanitize=address,undefined.
//
// A TILE is kGramTile x kGramTile elements of the result: tile (ti, tj) holds the rows [128 ti, 128 ti + 128) of a
// against those of b.  The symmetric form (b == a) has only the tiles with tj >= ti, numbered row by row; their owner
// stores the mirror image too.  The columns are cut into SLICES of kGramSlice; a RUN is run_slices <= kGramRunSlices
// consecutive slices, so a run is at most kGramRunCols = 65536 columns.  That is the int32 bound: a product of two
// operands (x XOR 0x80 as int8) is at most 16384 in magnitude, an int32 accumulator holds 131071 of them, and a run is
// all an accumulator ever sums before it is widened to int64 and added to the result.
// An ITEM is one (run, tile): item = run * tiles + tile -- slice-major, so that the items next to each other are the
// tiles of ONE run, which read the same columns of every row block.  Short inputs get shorter runs (down to one slice),
// so that there are about kGramTargetItems items to spread over the device.  The grid is capped at kGramMaxBlocks and a
// multiple of 8; workgroup `block` starts at item (block % 8) * (grid / 8) + block / 8 -- each XCD (workgroups go to the 8
// XCDs round robin) gets a contiguous range of items, i.e. whole runs, whose re-reads then hit that XCD's L2 -- and strides
// by grid.
#pragma once
#include <stdint.h>

#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kGramTile = 128;        // rows of a and of b in a tile
constexpr uint32_t kGramThreads = 256;     // 4 waves, 2 x 2, each 64 x 64 of the tile
constexpr uint32_t kGramStep = 64;         // columns of one MFMA (i32_16x16x64_i8)
constexpr uint32_t kGramSlice = 4096;      // columns of a slice
constexpr uint32_t kGramRunSlices = 16;    // slices of a run at most
constexpr uint32_t kGramRunCols = kGramSlice * kGramRunSlices;
constexpr uint32_t kGramInt32Cols = 131071;  // floor((2^31 - 1) / 16384)
static_assert(kGramRunCols <= kGramInt32Cols && kGramSlice % kGramStep == 0, "a run fits an int32 accumulator");
static_assert((uint64_t)255 * 16 * (kGramRunCols / kGramStep) < (1ull << 32), "a lane's row sum of a run fits 32 bits");
constexpr uint32_t kGramXcds = 8;
constexpr uint32_t kGramMaxBlocks = 2048;  // the grid is capped; the kernel strides
constexpr uint32_t kGramTargetItems = 4096;
static_assert(kGramMaxBlocks % kGramXcds == 0, "every XCD takes the same share of the grid");
constexpr uint64_t kGramMaxCols = kMaxCols;
constexpr uint64_t kGramMaxRows = 1ull << 31;  // a_rows and b_rows are at most this

// mhi_gram's arguments, pointers as plain addresses: nothing here reads through them
struct GramArgs {
    uint64_t a, a_row_stride, a_rows;
    uint64_t b, b_row_stride, b_rows, cols;
    uint64_t gram, gram_row_stride;
    uint64_t sum_a, sum_b;
    uint32_t accumulate;
};

struct GramLayout {
    uint32_t symmetric;   // b == NULL
    uint32_t nta, ntb;    // tiles along a's and b's rows
    uint64_t tiles;       // nta * ntb, or nta * (nta + 1) / 2 in the symmetric form
    uint64_t slices;      // ceil(cols / kGramSlice)
    uint32_t run_slices;  // slices of a run, 1 .. kGramRunSlices
    uint64_t runs;        // ceil(slices / run_slices)
    uint64_t items;       // runs * tiles
    uint32_t grid;        // workgroups: a multiple of 8, at most kGramMaxBlocks
    uint64_t cols;
};

struct GramItem {
    uint32_t ti, tj;  // the tile
    uint64_t k0, k1;  // the columns [k0, k1)
};

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int gram_check(Msg &m, const GramArgs &g)
{
    if (!g.a || !g.gram) return m.set(MH_ERR_ARG, "mhi_gram: NULL pointer");
    const uint64_t b_rows = g.b ? g.b_rows : g.a_rows;
    if (g.a_rows == 0 || b_rows == 0 || g.cols == 0)
        return m.set(MH_ERR_ARG, "mhi_gram: a_rows=%llu, b_rows=%llu, cols=%llu (each at least 1)", (unsigned long long)g.a_rows,
                     (unsigned long long)b_rows, (unsigned long long)g.cols);
    if (g.cols >= kGramMaxCols) return m.set(MH_ERR_ARG, "mhi_gram: cols=%llu (below 2^40)", (unsigned long long)g.cols);
    if (g.a_rows > kGramMaxRows || b_rows > kGramMaxRows)
        return m.set(MH_ERR_ARG, "mhi_gram: a_rows=%llu, b_rows=%llu (each at most 2^31)", (unsigned long long)g.a_rows,
                     (unsigned long long)b_rows);
    if (g.a_rows > 1 && g.a_row_stride < g.cols)
        return m.set(MH_ERR_ARG, "mhi_gram: a_row_stride=%llu is below cols=%llu", (unsigned long long)g.a_row_stride,
                     (unsigned long long)g.cols);
    if (g.b && g.b_rows > 1 && g.b_row_stride < g.cols)
        return m.set(MH_ERR_ARG, "mhi_gram: b_row_stride=%llu is below cols=%llu", (unsigned long long)g.b_row_stride,
                     (unsigned long long)g.cols);
    if (g.accumulate > 1) return m.set(MH_ERR_ARG, "mhi_gram: accumulate=%u (0 or 1)", g.accumulate);
    if (g.gram % 8 || g.gram_row_stride % 8)
        return m.set(MH_ERR_ARG, "mhi_gram: gram and gram_row_stride must be multiples of 8");
    if (g.a_rows > 1 && g.gram_row_stride < 8 * b_rows)
        return m.set(MH_ERR_ARG, "mhi_gram: gram_row_stride=%llu is below the %llu bytes of a row", (unsigned long long)g.gram_row_stride,
                     (unsigned long long)(8 * b_rows));
    if (g.sum_a % 8 || g.sum_b % 8) return m.set(MH_ERR_ARG, "mhi_gram: sum_a and sum_b must be multiples of 8");
    const uint64_t nta = (g.a_rows + kGramTile - 1) / kGramTile, ntb = (b_rows + kGramTile - 1) / kGramTile;
    const unsigned __int128 items = (unsigned __int128)nta * ntb * ((g.cols + kGramSlice - 1) / kGramSlice);  // an upper bound
    if (items >= ((unsigned __int128)1 << 62))
        return m.set(MH_ERR_ARG, "mhi_gram: a_rows=%llu, b_rows=%llu are too large for cols=%llu", (unsigned long long)g.a_rows,
                     (unsigned long long)b_rows, (unsigned long long)g.cols);
    return MH_OK;
}

// the whole layout; the caller has passed gram_check
inline void gram_layout(uint64_t a_rows, uint64_t b_rows, uint64_t cols, bool symmetric, GramLayout *L)
{
    L->symmetric = symmetric;
    L->nta = (uint32_t)((a_rows + kGramTile - 1) / kGramTile);
    L->ntb = symmetric ? L->nta : (uint32_t)((b_rows + kGramTile - 1) / kGramTile);
    L->tiles = symmetric ? (uint64_t)L->nta * (L->nta + 1) / 2 : (uint64_t)L->nta * L->ntb;
    L->cols = cols;
    L->slices = (cols + kGramSlice - 1) / kGramSlice;
    // as long as a run may be, but no longer than leaves about kGramTargetItems items
    const unsigned __int128 all = (unsigned __int128)L->tiles * L->slices;
    const unsigned __int128 want = (all + kGramTargetItems - 1) / kGramTargetItems;
    L->run_slices = want < 1 ? 1u : want > kGramRunSlices ? kGramRunSlices : (uint32_t)want;
    L->runs = (L->slices + L->run_slices - 1) / L->run_slices;
    L->items = L->runs * L->tiles;  // (below 2^62: gram_check)
    const uint64_t blocks = L->items < kGramMaxBlocks ? L->items : kGramMaxBlocks;
    L->grid = (uint32_t)((blocks + kGramXcds - 1) / kGramXcds * kGramXcds);
}

// the first item of workgroup `block`; it goes on with item += grid while item < items
MH_HD inline uint64_t gram_first_item(uint32_t block, uint32_t grid)
{
    return (uint64_t)(block % kGramXcds) * (grid / kGramXcds) + block / kGramXcds;
}

// item -> its tile and its columns
MH_HD inline GramItem gram_owner(uint32_t symmetric, uint32_t nta, uint32_t ntb, uint64_t tiles, uint32_t run_slices,
                                      uint64_t cols, uint64_t item)
{
    GramItem it;
    const uint64_t run = item / tiles;
    uint64_t t = item - run * tiles;
    if (symmetric) {  // row ti of the upper triangle holds nta - ti tiles
        uint32_t ti = 0;
        while (t >= nta - ti) t -= nta - ti, ++ti;
        it.ti = ti, it.tj = ti + (uint32_t)t;
    } else {
        it.ti = (uint32_t)(t / ntb), it.tj = (uint32_t)(t - (uint64_t)it.ti * ntb);
    }
    const uint64_t run_cols = (uint64_t)run_slices * kGramSlice;
    it.k0 = run * run_cols;
    it.k1 = cols - it.k0 < run_cols ? cols : it.k0 + run_cols;
    return it;
}

}  // namespace mh
