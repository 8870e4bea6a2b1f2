// mh_aer_layout.hpp -- the tile rule and the scratch layout of mhi_aer_to_csr (include/muahuff_ingest.h): how a list of
// n (tick, channel) pairs over C channels is cut into wave sub-runs and tiles, and where the count matrix, the scan's
// partials and the per-row drop counts sit in the caller's scratch.  Pure C++ (no HIP, no device), as mh_planner.hpp
// and mh_worklist.hpp: mh_ingest.hip checks with aer_scratch_check() / aer_check() and launches what they return,
// mhi_aer_scratch_bytes IS aer_layout().bytes, and tests/aer_layout_check.cpp prints the layout and the checks' verdicts
// under -fsanitize=address,undefined.  The layout is a function of (n, C).
//
//   sub-run  W consecutive pairs, owned by ONE wave in the count and in the scatter kernel; row r of the count matrix
//            belongs to pairs [r * W, (r + 1) * W).  W is a multiple of 64:
//              n <= 2048 * 1024          W = 1024                               (rows = ceil(n / 1024) <= 2048)
//              else                      W = min(roundup64(ceil(n / 2048)), Wmax(C))    (about 2048 rows, then more)
//            Wmax = 16 * C rounded up to a power of two, within 4096 .. 65536: a row of the matrix costs 4 * C bytes
//            and is moved five times (count, group sums, bases, bases again, scatter), 20 C bytes against the 22 W
//            bytes of the row's pairs -- at most a sixth at W = 4 C ... a twentieth at W = 16 C.
//   tile     the sub-runs of one workgroup: waves * W pairs.  Every wave keeps C 32-bit counters / cursors in LDS, and
//            a workgroup stays within 64 KiB of it: 4 waves up to 4096 channels, 2 up to 8192, 1 up to 16384 = the
//            published limit MHI_AER_MAX_CHANNELS.
//   group    64 consecutive rows: the scan sums a group's rows per channel (partials), scans the partials, and walks
//            each group again to turn counts into output positions.
// Output positions are 32-bit in the matrix and in LDS, hence n < 2^32.
// The scratch sections are sized by rows_alloc >= rows, which -- unlike rows -- never falls when n rises, so that
// mhi_aer_scratch_bytes is non-decreasing in n: a scratch that served n pairs serves any shorter list.
#pragma once
#include <stdint.h>

#include "../../include/muahuff.h"  // MH_OK, MH_ERR_ARG; by its place: the check programs are built with -I csrc alone
#include "mh_msg.hpp"

namespace mh {

constexpr uint32_t kAerMaxChannels = 16384;     // == MHI_AER_MAX_CHANNELS
constexpr uint64_t kAerMaxPairs = 0xFFFFFFFFull;
constexpr uint32_t kAerMinRun = 1024;
constexpr uint32_t kAerRowsTarget = 2048;
constexpr uint32_t kAerGroupRows = 64;
constexpr uint32_t kAerLayoutColThreads = 256;  // mh_aer.hpp: kAerColThreads (mh_ingest.hip asserts that they agree)

struct AerLayout {
    uint32_t run;          // W: pairs per wave sub-run
    uint32_t waves;        // waves per workgroup
    uint32_t tile;         // waves * run
    uint32_t nbits;        // ceil(log2 C): ballots per 64-pair step
    uint32_t lds_bytes;    // per workgroup: waves * C * 4
    uint64_t rows;         // ceil(n / run)
    uint64_t groups;       // ceil(rows / 64)
    uint64_t rows_alloc;   // what the sections are sized by
    uint64_t groups_alloc;
    uint64_t off_matrix;   // u32[rows][C]
    uint64_t off_partial;  // u32[groups + 1][C]: the row behind the partials holds the channels' totals
    uint64_t off_drop;     // u32[rows]
    uint64_t bytes;        // == mhi_aer_scratch_bytes (a multiple of 16, never 0)
    uint32_t grid_tiles;   // k_aer_count, k_aer_scatter: ceil(rows / waves) workgroups; not capped: n is below 2^32
    uint32_t grid_cols_x;  // k_aer_group_sum, k_aer_bases: ceil(C / 256) by groups workgroups; not capped: C <= 16384,
    uint32_t grid_cols_y;  //   and n below 2^32 makes fewer than 65536 groups
};

// mhi_aer_to_csr's arguments, pointers as plain addresses: nothing here reads through them
struct AerArgs {
    uint64_t ticks, channels;
    uint32_t ch_bits;
    uint64_t n;
    uint32_t C;
    uint64_t out_ticks, ev_off, dropped, scratch, scratch_bytes;
};

inline uint32_t aer_run_max(uint32_t C)
{
    uint32_t w = 4096;
    while (w < 65536u && w < 16u * C) w <<= 1;
    return w;
}

inline uint32_t aer_waves(uint32_t C) { return C <= 4096u ? 4u : C <= 8192u ? 2u : 1u; }

// 0, or -1: C == 0 or above kAerMaxChannels; -2: n above kAerMaxPairs
inline int aer_layout(uint64_t n, uint32_t C, AerLayout *L)
{
    if (C == 0 || C > kAerMaxChannels) return -1;
    if (n > kAerMaxPairs) return -2;
    const uint64_t wmax = aer_run_max(C);
    const uint64_t knee = (uint64_t)kAerRowsTarget * kAerMinRun;
    uint64_t w = kAerMinRun;
    if (n > knee) {
        w = ((n + kAerRowsTarget - 1) / kAerRowsTarget + 63) & ~63ull;
        if (w > wmax) w = wmax;
    }
    L->run = (uint32_t)w;
    L->waves = aer_waves(C);
    L->tile = L->waves * L->run;
    L->nbits = 0;
    while (L->nbits < 32 && (1ull << L->nbits) < C) ++L->nbits;
    L->lds_bytes = L->waves * C * 4u;
    L->rows = (n + w - 1) / w;
    L->groups = (L->rows + kAerGroupRows - 1) / kAerGroupRows;
    const uint64_t by_max = (n + wmax - 1) / wmax;
    L->rows_alloc = n <= knee ? (n + kAerMinRun - 1) / kAerMinRun : by_max > kAerRowsTarget ? by_max : kAerRowsTarget;
    L->groups_alloc = (L->rows_alloc + kAerGroupRows - 1) / kAerGroupRows;
    const auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    L->off_matrix = 0;
    L->off_partial = up16(L->rows_alloc * C * 4);
    L->off_drop = L->off_partial + up16((L->groups_alloc + 1) * C * 4);
    L->bytes = L->off_drop + up16(L->rows_alloc * 4) + 16;
    L->grid_tiles = (uint32_t)((L->rows + L->waves - 1) / L->waves);
    L->grid_cols_x = (C + kAerLayoutColThreads - 1) / kAerLayoutColThreads;
    L->grid_cols_y = (uint32_t)L->groups;
    return 0;
}

// aer_layout with its refusals as text; `fn` names the entry point
inline int aer_shape_check(Msg &m, const char *fn, uint64_t n, uint32_t C, AerLayout *L)
{
    const int rc = aer_layout(n, C, L);
    if (rc == -1) return m.set(MH_ERR_ARG, "%s: C=%u (1 .. MHI_AER_MAX_CHANNELS = %u)", fn, C, kAerMaxChannels);
    if (rc) return m.set(MH_ERR_ARG, "%s: n=%llu (below 2^32: positions are 32-bit)", fn, (unsigned long long)n);
    return MH_OK;
}

// mhi_aer_scratch_bytes: MH_OK and the layout, or MH_ERR_ARG with the text in m; `bytes` is the address of the result
inline int aer_scratch_check(Msg &m, uint64_t n, uint32_t C, uint64_t bytes, AerLayout *L)
{
    if (!bytes) return m.set(MH_ERR_ARG, "mhi_aer_scratch_bytes: NULL pointer");
    return aer_shape_check(m, "mhi_aer_scratch_bytes", n, C, L);
}

// mhi_aer_to_csr: MH_OK and the layout, or MH_ERR_ARG with the text in m, before any device work
inline int aer_check(Msg &m, const AerArgs &a, AerLayout *L)
{
    if (!a.ticks || !a.channels || !a.out_ticks || !a.ev_off || !a.dropped || !a.scratch)
        return m.set(MH_ERR_ARG, "mhi_aer_to_csr: NULL pointer");
    if (a.ch_bits != 16 && a.ch_bits != 32) return m.set(MH_ERR_ARG, "mhi_aer_to_csr: ch_bits=%u (16 or 32)", a.ch_bits);
    if (int rc = aer_shape_check(m, "mhi_aer_to_csr", a.n, a.C, L)) return rc;
    if (a.scratch_bytes < L->bytes)
        return m.set(MH_ERR_ARG, "mhi_aer_to_csr: scratch_bytes=%llu, mhi_aer_scratch_bytes asks for %llu",
                     (unsigned long long)a.scratch_bytes, (unsigned long long)L->bytes);
    // (n is below 2^32 here; the sums wrap as pointer arithmetic does)
    if (a.n && a.ticks < a.out_ticks + a.n * 8 && a.out_ticks < a.ticks + a.n * 8)
        return m.set(MH_ERR_ARG, "mhi_aer_to_csr: out_ticks overlaps ticks");
    if (a.scratch % 16) return m.set(MH_ERR_ARG, "mhi_aer_to_csr: scratch is not 16-byte aligned");
    return MH_OK;
}

}  // namespace mh
