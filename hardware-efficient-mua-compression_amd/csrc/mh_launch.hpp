// mh_launch.hpp -- the launch geometry of every grid the two libraries cap below what the problem size asks for: one
// small function per capped launch, next to the constant that caps it, returning the grid and the kernel arguments
// derived with it.  Pure C++ (no HIP, no device, no global state): muahuff.hip and mh_ingest.hip launch what these
// return; tests/planner_check.cpp --geometry prints them under -fsanitize=address,undefined and
// tests/test_host_launch_geometry.py compares them with each rule restated in Python.  DESIGN.md ("Capped launch
// grids") lists what covers the part of the problem a capped grid does not reach.
//
// Tile and group sizes that the kernels fix are restated here as kGeo* constants (this header cannot include a kernel
// header): the .hip files static_assert that they agree.
#pragma once
#include <stdint.h>

#include "mh_msg.hpp"
#include "muahuff.h"

namespace mh {

// chunk_stride of `bits`-bit pieces: 0 (contiguous), or packed pieces only, a multiple of 16, at least one chunk
inline bool chunk_stride_ok(uint64_t chunk_stride, uint32_t bits)
{
    return !chunk_stride || (bits != 8 && chunk_stride % 16 == 0 && chunk_stride >= (uint64_t)MH_CHUNK * bits / 8);
}

struct GridXY {
    uint32_t x, y;
};

inline uint64_t grid_ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b ? 1 : 0); }
inline uint64_t clamp_grid(uint64_t n, uint64_t cap) { return n < 1 ? 1 : n < cap ? n : cap; }

// ---- one grid row per channel: the kernels loop ch += gridDim.y
constexpr uint32_t kGridMaxY = 65535;  // what HIP allows in y
inline uint32_t channel_rows(uint32_t C) { return C > kGridMaxY ? kGridMaxY : C; }

// ---- mh_synth_poisson (k_synth): x over the longest channel in workgroups of 256 threads x 16 samples, pc += gridDim.x * 256
constexpr uint32_t kSynthMaxX = 4096;
inline GridXY synth_grid(uint64_t max_len, uint32_t C)
{
    return {(uint32_t)clamp_grid(grid_ceil_div(max_len, 256 * 16), kSynthMaxX), channel_rows(C)};
}

// ---- mh_rebin
constexpr uint32_t kGeoRebinTileBytes = 32768;  // mh_layout.hpp: kRebinTileBytes
// r < 4 (k_rebin2): x over the longest channel's bins in tiles of kRebinTileBytes / r bins, b0 += gridDim.x * bins_per_tile
constexpr uint32_t kRebin2MaxX = 4096;
inline GridXY rebin2_grid(uint64_t max_len, uint32_t C, uint32_t r)
{
    const uint64_t bins_per_tile = kGeoRebinTileBytes / r;
    return {(uint32_t)clamp_grid(grid_ceil_div(grid_ceil_div(max_len, r), bins_per_tile), kRebin2MaxX), channel_rows(C)};
}
// r >= 4 (k_rebin3): unit = g bins = u whole dwords; tile = upt units (<= 32 KiB, whole passes of 256 threads when there
// are that many); a workgroup walks tpw consecutive tiles of a channel, tile0 += gridDim.x * tpw
constexpr uint32_t kRebin3MaxX = 65535;
struct Rebin3Launch {
    GridXY grid;
    uint32_t g, u, upt, tpw;
};
inline Rebin3Launch rebin3_launch(uint64_t max_len, uint32_t C, uint32_t r)
{
    Rebin3Launch l;
    l.g = r % 4 == 0 ? 1u : r % 2 == 0 ? 2u : 4u;
    l.u = l.g * r / 4;
    l.upt = kGeoRebinTileBytes / 4 / l.u;
    if (l.upt >= 256) l.upt -= l.upt % 256;
    l.tpw = 4;
    const uint64_t tile_bytes = (uint64_t)l.upt * l.u * 4;
    l.grid = {(uint32_t)clamp_grid(grid_ceil_div(grid_ceil_div(max_len, tile_bytes), l.tpw), kRebin3MaxX), channel_rows(C)};
    return l;
}

// ---- the zero fills of mh_decode_range / mh_decode_rebin (k_range_fill, k_rebin_fill): y = the records of one launch,
// the next launch takes the next kFillMaxRecords; the workgroups of x stride over the longest record (per_block
// elements per workgroup and pass, i += gridDim.x * 256)
constexpr uint32_t kFillMaxX = 1024;
constexpr uint32_t kFillMaxRecords = 65535;
inline uint32_t fill_grid_x(uint64_t max_fill, uint64_t per_block) { return (uint32_t)clamp_grid(grid_ceil_div(max_fill, per_block), kFillMaxX); }
inline uint32_t fill_grid_y(uint64_t nfill, uint64_t first) { return (uint32_t)(nfill - first < kFillMaxRecords ? nfill - first : kFillMaxRecords); }

// ---- mh_deinterleave, mh_deinterleave_packed, mh_interleave, mh_interleave_packed over T x C (C >= 1) with tpw tiles
// of a strip per workgroup visit: strips of kTr2C channels times visits, in ONE grid dimension (strip fastest); more
// strips than kTransposedMaxStrips are refused, the visits are capped so that the product fits kGridMaxX
// (tile0 += gx * tpw covers the rest).  `who` names the call.
constexpr uint64_t kGridMaxX = 0x7FFFFFFFull;  // what HIP allows in x
constexpr uint32_t kTransposedMaxStrips = 65535;
constexpr uint32_t kGeoTr2T = 256, kGeoTr2C = 128;  // mh_layout.hpp: kTr2T, kTr2C
inline int transposed_grid(Msg &m, const char *who, uint64_t T, uint32_t C, uint32_t tpw, uint32_t *grid)
{
    const uint32_t strips = (uint32_t)grid_ceil_div(C, kGeoTr2C);
    if (strips > kTransposedMaxStrips) return m.set(MH_ERR_ARG, "%s: C=%u too large", who, C);
    uint64_t visits = grid_ceil_div(grid_ceil_div(T, kGeoTr2T), tpw);
    if (visits > kGridMaxX / strips) visits = kGridMaxX / strips;
    *grid = (uint32_t)(visits * strips);
    return MH_OK;
}

// ---- mh_power_draws, mh_reduce_rows: one thread per item (`items`: what the message calls them), no loop in the kernel
inline int per_item_grid(Msg &m, const char *who, const char *items, uint64_t n, uint32_t *grid)
{
    if (n > kGridMaxX * 256) return m.set(MH_ERR_ARG, "%s: too many %s for one launch", who, items);
    *grid = (uint32_t)grid_ceil_div(n, 256);
    return MH_OK;
}

// ---- mh_compact (not capped: a plan has fewer than 2^32 segments): the blocks of kScanBlock segments that
// k_scan_block_sums / k_scan_apply take (up to one, every wave of k_compact scans for itself and they are not
// launched), and k_compact's workgroups of kCompactSegs segments
constexpr uint32_t kGeoScanBlock = 2048, kGeoCompactSegs = 4;  // mh_kernels.hpp: kScanBlock, kCompactSegs
inline uint32_t compact_scan_blocks(uint64_t nseg) { return (uint32_t)grid_ceil_div(nseg, kGeoScanBlock); }
inline uint32_t compact_groups(uint64_t nseg) { return (uint32_t)clamp_grid(grid_ceil_div(nseg, kGeoCompactSegs), ~0u); }

// ---- mhi_bin_events (k_bin_events): C x nspans workgroups in one dimension, a workgroup walks `span` chunks.  8 chunks
// amortise the start search and keep the event list streaming; fewer when that would leave the device short of
// workgroups (kBinMinGroups), more when the grid would not fit kGridMaxX.  C beyond kGridMaxX fits at no span.
constexpr uint64_t kBinMinGroups = 4096;
struct BinLaunch {
    uint64_t nchunks, span, nspans;
    uint32_t div_mode;  // how the kernel divides by the period: 0 not at all, 1 in 32 bits, 2 in 64
    uint32_t grid;
};
inline int bin_events_launch(Msg &m, uint32_t C, uint64_t T, uint64_t period, BinLaunch *l)
{
    if (C > kGridMaxX) return m.set(MH_ERR_ARG, "mhi_bin_events: C=%u does not fit one grid", C);
    l->nchunks = grid_ceil_div(T, MH_CHUNK);
    uint64_t span = 8;
    while (span > 1 && (unsigned __int128)C * grid_ceil_div(l->nchunks, span) < kBinMinGroups) span >>= 1;
    while ((unsigned __int128)C * grid_ceil_div(l->nchunks, span) > kGridMaxX) span <<= 1;  // (ends: C itself fits)
    l->span = span;
    l->nspans = grid_ceil_div(l->nchunks, span);
    l->div_mode = period == 1 ? 0u : period < (1ull << 18) ? 1u : 2u;
    l->grid = (uint32_t)(C * l->nspans);
    return MH_OK;
}

// ---- mhi_seg_crc32 (k_seg_crc32): workgroups of kCrcWaves segments, j += gridDim.x * kCrcWaves over a longer list
constexpr uint32_t kGeoCrcWaves = 4, kCrcMaxX = 2048;  // mh_crc.hpp: kCrcWaves, kCrcMaxGroups (8 workgroups per CU)
inline uint32_t seg_crc_grid(uint64_t n_list) { return (uint32_t)clamp_grid(grid_ceil_div(n_list, kGeoCrcWaves), kCrcMaxX); }

// ---- mhi_excess_apply: workgroups of kGeoApplyThreads threads
constexpr uint32_t kGeoApplyThreads = 256;           // mh_excess_layout.hpp: kApplyThreads
constexpr uint64_t kGeoApplyMaxBlocks = 1u << 20;    // mh_excess_layout.hpp: kApplyMaxBlocks
// r == 1 (k_excess_apply1): one grid row per output row, i += gridDim.y; a row's entries are few against its samples,
// so at most kApply1MaxX workgroups stride them, e += gridDim.x * 256 (x is sized by the whole list: no row has more)
constexpr uint32_t kApply1MaxX = 64;
inline GridXY excess_apply1_grid(uint64_t n_entries, uint64_t n_rows)
{
    return {(uint32_t)clamp_grid(grid_ceil_div(n_entries, kGeoApplyThreads), kApply1MaxX), (uint32_t)clamp_grid(n_rows, kGridMaxY)};
}
// r > 1 (k_excess_apply): a thread per run of a row, n_rows * runs jobs (below 2^63: the call refuses more) in one
// dimension, job += gridDim.x * 256
inline uint32_t excess_apply_grid(uint64_t n_rows, uint64_t runs)
{
    return (uint32_t)clamp_grid(grid_ceil_div(n_rows * runs, kGeoApplyThreads), kGeoApplyMaxBlocks);
}

}  // namespace mh
