// mh_excess_layout.hpp -- the tile rule and the scratch layout of mhi_excess_count / mhi_excess_emit
// (include/muahuff_ingest.h): how a matrix of uint8 counts is cut into the pieces whose entries -- the elements above
// the threshold -- are counted, scanned and then emitted at their base.  Pure C++ (no HIP, no device), as
// mh_unbin_layout.hpp: mh_ingest.hip checks with excess_scratch_check() / excess_count_check() / excess_emit_check() /
// excess_apply_check() and launches what they return, mhi_excess_scratch_bytes IS excess_layout().bytes, and
// tests/excess_layout_check.cpp prints the layout and the checks' verdicts under -fsanitize=address,undefined.  The
// layout is a function of (form, rows, cols).
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
    uint64_t waves;        // COLS: strips * per_channel, a wave per (strip, time tile); 0 in the ROWS form
    uint32_t grid;         // k_excess_*_count, k_excess_*_emit: ceil(pieces (ROWS) or waves (COLS) / kExcessWaves);
                           //   not capped: pieces fit 32 bits, and there are never more waves than pieces
    uint32_t grid_scan;    // k_unbin_group_sum, k_unbin_bases: groups; not capped: pieces fit 32 bits
};

// what mhi_excess_count and mhi_excess_emit share, pointers as plain addresses: nothing here reads through them
struct ExcessArgs {
    uint32_t form;
    uint64_t in, row_off, lo, hi, rows, cols;
    uint32_t threshold;
    uint64_t scratch, scratch_bytes;
};
struct ExcessCountArgs {
    ExcessArgs s;
    uint64_t exc_off, total;
};
struct ExcessEmitArgs {
    ExcessArgs s;
    uint64_t pos, val, capacity, over;
};
// mhi_excess_apply's arguments
struct ApplyArgs {
    uint64_t pos, val, n_entries, first, last, n_rows, start, stop, r, lead, out;
    uint32_t out_bits;
    uint64_t row_stride, col_stride;
};
// what excess_apply_check works out on the way; both 0: nothing to add (no rows, no entries or an empty range), nothing
// to launch
struct ApplyLayout {
    uint64_t elements;  // of an output row
    uint64_t runs;      // ceil(elements / kApplyRun): the jobs of a row (r > 1)
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
    L->waves = L->strips * L->per_channel;
    L->grid = (uint32_t)(((form == kExcessRows ? L->pieces : L->waves) + kExcessWaves - 1) / kExcessWaves);
    L->grid_scan = (uint32_t)L->groups;
    return 0;
}

// mhi_excess_scratch_bytes: MH_OK and the layout, or MH_ERR_ARG with the text in m; `bytes` is the address of the result
inline int excess_scratch_check(Msg &m, uint32_t form, uint64_t rows, uint64_t cols, uint64_t bytes, ExcessLayout *L)
{
    if (!bytes) return m.set(MH_ERR_ARG, "mhi_excess_scratch_bytes: NULL pointer");
    const int rc = excess_layout(form, rows, cols, L);
    if (rc == -1)
        return m.set(MH_ERR_ARG, "mhi_excess_scratch_bytes: form=%u, rows=%llu, cols=%llu (a known form, each at least 1, cols below 2^32; COLS form: rows below 2^32)",
                     form, (unsigned long long)rows, (unsigned long long)cols);
    if (rc)
        return m.set(MH_ERR_ARG, "mhi_excess_scratch_bytes: rows=%llu, cols=%llu make more than 2^32 - 1 pieces",
                     (unsigned long long)rows, (unsigned long long)cols);
    return MH_OK;
}

// what mhi_excess_count and mhi_excess_emit share: the form, the shape, the threshold and the scratch.  `fn` names the
// caller.
inline int excess_shared_check(Msg &m, const char *fn, const ExcessArgs &a, ExcessLayout *L)
{
    if (a.form != kExcessRows && a.form != kExcessCols)
        return m.set(MH_ERR_ARG, "%s: form=%u (MHI_EXCESS_ROWS or MHI_EXCESS_COLS)", fn, a.form);
    if (!a.in || !a.scratch) return m.set(MH_ERR_ARG, "%s: NULL pointer", fn);
    if (a.form == kExcessRows && !a.row_off) return m.set(MH_ERR_ARG, "%s: the ROWS form needs row_off", fn);
    if (a.form == kExcessCols && (a.row_off || a.lo || a.hi))
        return m.set(MH_ERR_ARG, "%s: the COLS form is one contiguous block, every column whole: row_off, lo and hi must be NULL", fn);
    if (a.threshold < 1 || a.threshold > 254) return m.set(MH_ERR_ARG, "%s: threshold=%u (1 .. 254)", fn, a.threshold);
    const int rc = excess_layout(a.form, a.rows, a.cols, L);
    if (rc == -1)
        return m.set(MH_ERR_ARG, "%s: rows=%llu, cols=%llu (each at least 1, cols below 2^32; COLS form: rows below 2^32)", fn,
                     (unsigned long long)a.rows, (unsigned long long)a.cols);
    if (rc)
        return m.set(MH_ERR_ARG, "%s: rows=%llu, cols=%llu make more than 2^32 - 1 pieces", fn, (unsigned long long)a.rows,
                     (unsigned long long)a.cols);
    if (a.scratch_bytes < L->bytes)
        return m.set(MH_ERR_ARG, "%s: scratch_bytes=%llu, mhi_excess_scratch_bytes asks for %llu", fn,
                     (unsigned long long)a.scratch_bytes, (unsigned long long)L->bytes);
    if (a.scratch % 16) return m.set(MH_ERR_ARG, "%s: scratch is not 16-byte aligned", fn);
    return MH_OK;
}

// mhi_excess_count / mhi_excess_emit: MH_OK and the layout, or MH_ERR_ARG with the text in m, before any device work
inline int excess_count_check(Msg &m, const ExcessCountArgs &a, ExcessLayout *L)
{
    if (int rc = excess_shared_check(m, "mhi_excess_count", a.s, L)) return rc;
    if (!a.exc_off || !a.total) return m.set(MH_ERR_ARG, "mhi_excess_count: NULL pointer");
    return MH_OK;
}

inline int excess_emit_check(Msg &m, const ExcessEmitArgs &a, ExcessLayout *L)
{
    if (int rc = excess_shared_check(m, "mhi_excess_emit", a.s, L)) return rc;
    if (!a.pos || !a.val || !a.over) return m.set(MH_ERR_ARG, "mhi_excess_emit: NULL pointer");
    if (a.pos % 4) return m.set(MH_ERR_ARG, "mhi_excess_emit: pos is not 4-byte aligned");
    return MH_OK;
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

// mhi_excess_apply: MH_OK and the row's elements and runs (0 and 0: nothing to add), or MH_ERR_ARG with the text in m
inline int excess_apply_check(Msg &m, const ApplyArgs &a, ApplyLayout *L)
{
    L->elements = L->runs = 0;
    if (!a.first || !a.last || !a.out || (a.n_entries && (!a.pos || !a.val))) return m.set(MH_ERR_ARG, "mhi_excess_apply: NULL pointer");
    if (a.out_bits != 8 && a.out_bits != 32) return m.set(MH_ERR_ARG, "mhi_excess_apply: out_bits=%u (8 or 32)", a.out_bits);
    if (a.r == 0 || a.r > kExcessMaxLen || a.lead >= kExcessMaxLen)
        return m.set(MH_ERR_ARG, "mhi_excess_apply: r=%llu, lead=%llu (r 1 .. 2^32, lead below 2^32)", (unsigned long long)a.r,
                     (unsigned long long)a.lead);
    if (a.start > a.stop || a.stop > kExcessMaxLen)
        return m.set(MH_ERR_ARG, "mhi_excess_apply: start=%llu, stop=%llu (start <= stop <= 2^32)", (unsigned long long)a.start,
                     (unsigned long long)a.stop);
    if (a.out_bits == 32 && (a.out % 4 || a.row_stride % 4 || a.col_stride % 4))
        return m.set(MH_ERR_ARG, "mhi_excess_apply: out_bits=32 needs out and both strides to be multiples of 4");
    if (a.pos % 4) return m.set(MH_ERR_ARG, "mhi_excess_apply: pos is not 4-byte aligned");
    if (a.n_rows == 0 || a.n_entries == 0 || a.start == a.stop) return MH_OK;  // nothing to add
    const uint64_t elements = apply_elements(a.start, a.stop, a.r, a.lead);
    const uint64_t runs = (elements + kApplyRun - 1) / kApplyRun;
    if ((unsigned __int128)a.n_rows * runs >= ((unsigned __int128)1 << 63))
        return m.set(MH_ERR_ARG, "mhi_excess_apply: n_rows=%llu is too large", (unsigned long long)a.n_rows);
    L->elements = elements, L->runs = runs;
    return MH_OK;
}

}  // namespace mh
