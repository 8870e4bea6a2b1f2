// mh_excess_layout.hpp -- the tile rule and the scratch layout of mhi_excess_count / mhi_excess_emit
// (include/muahuff_ingest.h): how a matrix of uint8 counts is cut into the pieces whose entries -- the elements above
// the threshold -- are counted, scanned and then emitted at their base.  Pure C++ (no HIP, no device), as
// mh_unbin_layout.hpp: mh_ingest.hip launches from it, mhi_excess_scratch_bytes IS excess_layout().bytes, and
// tests/excess_layout_check.cpp prints it under -fsanitize=address,undefined.  Everything is a function of
// (form, rows, cols).
//
//   ROWS form  rows are channels.  Row i is cut as the CSR form of mh_unbin_layout.hpp cuts it: ceil(cols / 16384)
//              tiles of 16 wave rows of 1 KiB, one wave per tile; a tile examines the columns of its span that lie in
//              the row's window [lo, hi), and a tile outside the window costs its wave two loads.
//              piece t = row t / per_channel, tile t % per_channel.
//   COLS form  one time-major [rows = T, cols = C] block.  A lane owns kExcessLaneCh adjacent channels, so that a wave
//              reads a STRIP of 64 * 4 = 256 channels with one dword per lane and time step -- a coalesced run of the
//              matrix -- and walks a time tile of kExcessTileT steps of it.  The piece is the CELL (time tile, channel):
//              piece t = channel t / per_channel, time tile t % per_channel -- channel-major, which is the order of the
//              list, so that one scan over the pieces gives every cell's base and no cross-lane reduction is needed.
//   group      1024 consecutive pieces, as in mh_unbin_layout.hpp: the scan kernels of mh_unbin.hpp run on the pieces
//              unchanged (a piece holds at most 16384 entries).
// A position inside a channel is 32-bit: channel lengths (ROWS cols, COLS rows) of 2^32 and more are refused, and so
// are more than 2^32 - 1 pieces.
#pragma once
#include <stdint.h>

#include "mh_unbin_layout.hpp"

namespace mh {

constexpr uint32_t kExcessRows = 0;  // == MHI_EXCESS_ROWS
constexpr uint32_t kExcessCols = 1;  // == MHI_EXCESS_COLS
constexpr uint32_t kExcessLaneCh = 4;                    // adjacent channels of one lane: one dword per time step
constexpr uint32_t kExcessStrip = 64 * kExcessLaneCh;    // channels of one wave
constexpr uint32_t kExcessTileT = 512;                   // time steps of one cell
constexpr uint32_t kExcessWaves = 4;                     // waves per workgroup, both forms
constexpr uint64_t kExcessMaxLen = 1ull << 32;           // a channel is shorter than this
constexpr uint64_t kExcessMaxPieces = kUnbinMaxTiles;

static_assert(kExcessTileT <= 65535, "a lane counts a cell in 16 bits");
static_assert(kExcessTileT <= kUnbinTile, "a piece's count fits the scan's 32-bit group sums");

struct ExcessLayout {
    uint64_t channels;     // ROWS: rows; COLS: cols -- exc_off has channels + 1 entries
    uint64_t length;       // ROWS: cols; COLS: rows -- the samples of a channel
    uint64_t per_channel;  // pieces of one channel
    uint64_t pieces;
    uint64_t groups;       // ceil(pieces / 1024)
    uint64_t strips;       // COLS: ceil(cols / 256); 0 in the ROWS form
    uint64_t off_sum;      // u32[pieces]
    uint64_t off_base;     // u64[pieces]
    uint64_t off_partial;  // u64[groups + 1]: the entry behind the groups holds the total
    uint64_t bytes;        // == mhi_excess_scratch_bytes (a multiple of 16, never 0)
};

// 0, or -1: unknown form, rows == 0, cols == 0, a channel of 2^32 samples or more, COLS cols >= 2^32;
// -2: more than kExcessMaxPieces pieces
inline int excess_layout(uint32_t form, uint64_t rows, uint64_t cols, ExcessLayout *L)
{
    if ((form != kExcessRows && form != kExcessCols) || rows == 0 || cols == 0) return -1;
    if (cols >= kExcessMaxLen) return -1;  // ROWS: the channel length; COLS: a channel number is 32-bit too
    if (form == kExcessCols && rows >= kExcessMaxLen) return -1;
    if (form == kExcessRows) {
        L->channels = rows, L->length = cols;
        L->per_channel = cols / kUnbinTile + (cols % kUnbinTile ? 1 : 0);
        L->strips = 0;
    } else {
        L->channels = cols, L->length = rows;
        L->per_channel = rows / kExcessTileT + (rows % kExcessTileT ? 1 : 0);
        L->strips = cols / kExcessStrip + (cols % kExcessStrip ? 1 : 0);
    }
    const unsigned __int128 pieces = (unsigned __int128)L->channels * L->per_channel;
    if (pieces > kExcessMaxPieces) return -2;
    L->pieces = (uint64_t)pieces;
    L->groups = (L->pieces + kUnbinGroup - 1) / kUnbinGroup;
    const auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    L->off_sum = 0;
    L->off_base = up16(L->pieces * 4);
    L->off_partial = L->off_base + up16(L->pieces * 8);
    L->bytes = L->off_partial + up16((L->groups + 1) * 8);
    return 0;
}

// mhi_excess_apply: an output row is cut into runs of kApplyRun elements, one thread each (r > 1)
constexpr uint32_t kApplyRun = 32;
constexpr uint32_t kApplyThreads = 256;
constexpr uint64_t kApplyMaxBlocks = 1u << 20;  // the grid is capped; the kernels stride

// elements of an output row: ceil((stop - start + lead) / r); the caller has checked start <= stop <= 2^32, r >= 1
inline uint64_t apply_elements(uint64_t start, uint64_t stop, uint64_t r, uint64_t lead)
{
    const uint64_t n = stop - start + lead;
    return n / r + (n % r ? 1 : 0);
}

}  // namespace mh
