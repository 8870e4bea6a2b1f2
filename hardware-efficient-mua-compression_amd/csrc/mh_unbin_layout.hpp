// mh_unbin_layout.hpp -- the tile rule and the scratch layout of mhi_unbin_count / mhi_unbin_emit
// (include/muahuff_ingest.h): how a matrix of uint8 counts is cut into tiles, one per wave, and where the tile sums, the
// tiles' output bases and the scan's partials sit in the caller's scratch.  Pure C++ (no HIP, no device), as
// mh_aer_layout.hpp: mh_ingest.hip checks with unbin_scratch_check() / unbin_count_check() / unbin_emit_check() and
// launches what they return, mhi_unbin_scratch_bytes IS unbin_layout().bytes, and tests/unbin_layout_check.cpp prints the
// layout and the checks' verdicts under -fsanitize=address,undefined.  The layout is a function of (form, rows, cols).
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

#include "../../include/muahuff.h"  // MH_OK, MH_ERR_ARG; by its place: the check programs are built with -I csrc alone
#include "mh_msg.hpp"

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
    uint32_t grid;           // k_unbin_count, k_unbin_emit: ceil(tiles / kUnbinWaves); not capped: tiles fit 32 bits
    uint32_t grid_scan;      // k_unbin_group_sum, k_unbin_bases: groups; not capped: tiles fit 32 bits
};

// what mhi_unbin_count and mhi_unbin_emit share, pointers as plain addresses: nothing here reads through them
struct UnbinArgs {
    uint32_t form;
    uint64_t in, row_off, rows, cols;
    uint64_t scratch, scratch_bytes;
};
struct UnbinCountArgs {
    UnbinArgs s;
    uint64_t ev_off, total;
};
struct UnbinEmitArgs {
    UnbinArgs s;
    uint64_t origin, period, phase;
    uint64_t out_ticks, out_ch;
    uint32_t ch_bits;
    uint64_t capacity, over;
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
    L->grid = (uint32_t)((L->tiles + kUnbinWaves - 1) / kUnbinWaves);
    L->grid_scan = (uint32_t)L->groups;
    return 0;
}

// mhi_unbin_scratch_bytes: MH_OK and the layout, or MH_ERR_ARG with the text in m; `bytes` is the address of the result
inline int unbin_scratch_check(Msg &m, uint32_t form, uint64_t rows, uint64_t cols, uint64_t bytes, UnbinLayout *L)
{
    if (!bytes) return m.set(MH_ERR_ARG, "mhi_unbin_scratch_bytes: NULL pointer");
    const int rc = unbin_layout(form, rows, cols, L);
    if (rc == -1)
        return m.set(MH_ERR_ARG, "mhi_unbin_scratch_bytes: form=%u, rows=%llu, cols=%llu (a known form, each at least 1; AER form: cols <= 2^32)",
                     form, (unsigned long long)rows, (unsigned long long)cols);
    if (rc)
        return m.set(MH_ERR_ARG, "mhi_unbin_scratch_bytes: rows=%llu, cols=%llu make more than 2^32 - 1 tiles",
                     (unsigned long long)rows, (unsigned long long)cols);
    return MH_OK;
}

// what mhi_unbin_count and mhi_unbin_emit share: the form, the shape and the scratch.  `fn` names the caller.
inline int unbin_shared_check(Msg &m, const char *fn, const UnbinArgs &a, UnbinLayout *L)
{
    if (a.form != kUnbinCsr && a.form != kUnbinAer)
        return m.set(MH_ERR_ARG, "%s: form=%u (MHI_UNBIN_CSR or MHI_UNBIN_AER)", fn, a.form);
    if (!a.in || !a.scratch) return m.set(MH_ERR_ARG, "%s: NULL pointer", fn);
    if (a.form == kUnbinCsr && !a.row_off) return m.set(MH_ERR_ARG, "%s: the CSR form needs row_off", fn);
    if (a.form == kUnbinAer && a.row_off)
        return m.set(MH_ERR_ARG, "%s: the AER form is one contiguous block: row_off must be NULL", fn);
    const int rc = unbin_layout(a.form, a.rows, a.cols, L);
    if (rc == -1)
        return m.set(MH_ERR_ARG, "%s: rows=%llu, cols=%llu (each at least 1; AER form: cols <= 2^32)", fn,
                     (unsigned long long)a.rows, (unsigned long long)a.cols);
    if (rc)
        return m.set(MH_ERR_ARG, "%s: rows=%llu, cols=%llu make more than 2^32 - 1 tiles", fn, (unsigned long long)a.rows,
                     (unsigned long long)a.cols);
    if (a.scratch_bytes < L->bytes)
        return m.set(MH_ERR_ARG, "%s: scratch_bytes=%llu, mhi_unbin_scratch_bytes asks for %llu", fn,
                     (unsigned long long)a.scratch_bytes, (unsigned long long)L->bytes);
    if (a.scratch % 16) return m.set(MH_ERR_ARG, "%s: scratch is not 16-byte aligned", fn);
    return MH_OK;
}

// mhi_unbin_count: MH_OK and the layout, or MH_ERR_ARG with the text in m, before any device work
inline int unbin_count_check(Msg &m, const UnbinCountArgs &a, UnbinLayout *L)
{
    if (int rc = unbin_shared_check(m, "mhi_unbin_count", a.s, L)) return rc;
    if (!a.total) return m.set(MH_ERR_ARG, "mhi_unbin_count: NULL pointer");
    if (a.s.form == kUnbinCsr && !a.ev_off) return m.set(MH_ERR_ARG, "mhi_unbin_count: the CSR form needs ev_off");
    return MH_OK;
}

// mhi_unbin_emit: the same, with the 2^63 bound of the ticks and out_ticks against the input
inline int unbin_emit_check(Msg &m, const UnbinEmitArgs &a, UnbinLayout *L)
{
    if (int rc = unbin_shared_check(m, "mhi_unbin_emit", a.s, L)) return rc;
    if (!a.out_ticks || !a.over) return m.set(MH_ERR_ARG, "mhi_unbin_emit: NULL pointer");
    if (a.period == 0 || a.phase >= a.period)
        return m.set(MH_ERR_ARG, "mhi_unbin_emit: period=%llu, phase=%llu (period at least 1, phase below it)",
                     (unsigned long long)a.period, (unsigned long long)a.phase);
    const uint64_t steps = a.s.form == kUnbinCsr ? a.s.cols : a.s.rows;
    const unsigned __int128 last = (unsigned __int128)a.origin + (unsigned __int128)(steps - 1) * a.period + a.phase;
    if (last >= ((unsigned __int128)1 << 63))
        return m.set(MH_ERR_ARG, "mhi_unbin_emit: the largest tick reaches 2^63 (origin=%llu, period=%llu, phase=%llu, %llu steps)",
                     (unsigned long long)a.origin, (unsigned long long)a.period, (unsigned long long)a.phase,
                     (unsigned long long)steps);
    if (a.s.form == kUnbinAer) {
        if (!a.out_ch) return m.set(MH_ERR_ARG, "mhi_unbin_emit: the AER form needs out_ch");
        if (a.ch_bits != 16 && a.ch_bits != 32) return m.set(MH_ERR_ARG, "mhi_unbin_emit: ch_bits=%u (16 or 32)", a.ch_bits);
        if (a.ch_bits == 16 && a.s.cols > 65536)
            return m.set(MH_ERR_ARG, "mhi_unbin_emit: cols=%llu does not fit 16-bit channels", (unsigned long long)a.s.cols);
    }
    // out_ticks[0 .. capacity) against the input: the whole block in the AER form, where its extent is known here
    const unsigned __int128 in = a.s.in, out = a.out_ticks;
    const unsigned __int128 n_in = a.s.form == kUnbinAer ? (unsigned __int128)a.s.rows * a.s.cols : 1;
    const unsigned __int128 n_out = (unsigned __int128)a.capacity * 8;
    if (n_out && in < out + n_out && out < in + n_in) return m.set(MH_ERR_ARG, "mhi_unbin_emit: out_ticks overlaps the input");
    return MH_OK;
}

}  // namespace mh
