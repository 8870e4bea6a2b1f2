// mh_unbin_layout.hpp -- the tile rule and the scratch layout of mhi_unbin_count / mhi_unbin_emit
// (include/muahuff_ingest.h): how a matrix of uint8 counts is cut into tiles, one per wave, and where the tile sums, the
// tiles' output bases and the scan's partials sit in the caller's scratch.  Pure C++ (no HIP, no device), as
// mh_aer_layout.hpp: mh_ingest.hip launches from it, mhi_unbin_scratch_bytes IS unbin_layout().bytes, and
// tests/unbin_layout_check.cpp prints it under -fsanitize=address,undefined.  Everything is a function of
// (form, rows, cols).
//
//   wave row  1 KiB: what a wave reads with one 16-byte load per lane.
//   tile      16 wave rows = 16 KiB of ONE contiguous span of the input, owned by one wave in the count and in the emit
//             kernel.  A tile never holds bytes of two rows of the CSR form -- a row's bytes are all the caller vouches
//             for -- so there row i is cut into ceil(cols / 16384) tiles, the last one short:
//               tile t = row t / tiles_per_row, bytes [k * 16384, min(cols, (k + 1) * 16384)), k = t % tiles_per_row.
//             The AER form is one contiguous block, cut flat: tile t = bytes [t * 16384, min(rows * cols, ...)); the
//             (time step, channel) of a byte comes from one division per wave and a small one per event.
//             A tile's sum is at most 16384 * 255 < 2^22.
//   group     1024 consecutive tiles: the scan sums a group's tiles (< 2^32, so 32-bit), scans the group sums in 64
//             bits, and walks each group again to turn the sums into 64-bit output bases.
// Tiles are counted in 32 bits (a grid dimension, and the divisions by tiles_per_row): more than 2^32 - 1 are refused.
#pragma once
#include <stdint.h>

namespace mh {

constexpr uint32_t kUnbinCsr = 0;  // == MHI_UNBIN_CSR: rows are channels, columns are bins
constexpr uint32_t kUnbinAer = 1;  // == MHI_UNBIN_AER: rows are time steps, columns are channels
constexpr uint32_t kUnbinRowBytes = 1024;
constexpr uint32_t kUnbinTileRows = 16;
constexpr uint32_t kUnbinTile = kUnbinRowBytes * kUnbinTileRows;
constexpr uint32_t kUnbinWaves = 4;      // tiles per workgroup
constexpr uint32_t kUnbinGroup = 1024;   // tiles per group of the scan
constexpr uint32_t kUnbinStage = 2048;   // events a wave stages in LDS before it stores them (16-bit entries)
constexpr uint64_t kUnbinMaxTiles = 0xFFFFFFFFull;
constexpr uint64_t kUnbinMaxAerCols = 1ull << 32;  // a channel number fits 32 bits

static_assert((uint64_t)kUnbinTile * 255 * kUnbinGroup < (1ull << 32), "a group's sum is 32-bit");
static_assert(kUnbinTile <= 65536, "an element's place in its tile is staged in 16 bits");

struct UnbinLayout {
    uint64_t tiles_per_row;  // CSR form; 0 in the AER form
    uint64_t tiles;
    uint64_t groups;         // ceil(tiles / 1024)
    uint64_t off_sum;        // u32[tiles]
    uint64_t off_base;       // u64[tiles]
    uint64_t off_partial;    // u64[groups + 1]: the entry behind the groups holds the total
    uint64_t bytes;          // == mhi_unbin_scratch_bytes (a multiple of 16, never 0)
};

// 0, or -1: unknown form, rows == 0, cols == 0, AER cols above 2^32; -2: more than kUnbinMaxTiles tiles
inline int unbin_layout(uint32_t form, uint64_t rows, uint64_t cols, UnbinLayout *L)
{
    if ((form != kUnbinCsr && form != kUnbinAer) || rows == 0 || cols == 0) return -1;
    if (form == kUnbinAer && cols > kUnbinMaxAerCols) return -1;
    unsigned __int128 tiles;
    if (form == kUnbinCsr) {
        L->tiles_per_row = cols / kUnbinTile + (cols % kUnbinTile ? 1 : 0);
        tiles = (unsigned __int128)rows * L->tiles_per_row;
    } else {
        L->tiles_per_row = 0;
        tiles = ((unsigned __int128)rows * cols + (kUnbinTile - 1)) / kUnbinTile;
    }
    if (tiles > kUnbinMaxTiles) return -2;
    L->tiles = (uint64_t)tiles;
    L->groups = (L->tiles + kUnbinGroup - 1) / kUnbinGroup;
    const auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    L->off_sum = 0;
    L->off_base = up16(L->tiles * 4);
    L->off_partial = L->off_base + up16(L->tiles * 8);
    L->bytes = L->off_partial + up16((L->groups + 1) * 8);
    return 0;
}

}  // namespace mh
