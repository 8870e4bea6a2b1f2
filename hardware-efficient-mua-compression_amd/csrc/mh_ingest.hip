// mh_ingest.hip -- the C ABI of include/muahuff_ingest.h over the kernels of mh_ingest.hpp, mh_aer.hpp, mh_crc.hpp,
// mh_unbin.hpp, mh_excess.hpp, mh_windows.hpp and mh_gram.hpp.  Every entry point builds its argument struct, asks the
// check of its host-only header (mh_*_layout.hpp, mh_ingest_check.hpp) for a verdict and the layout, and launches what
// came back: no argument rule and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no
// CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_aer.hpp"
#include "mh_aer_layout.hpp"
#include "mh_crc.hpp"
#include "mh_excess.hpp"
#include "mh_excess_layout.hpp"
#include "mh_gram.hpp"
#include "mh_gram_layout.hpp"
#include "mh_ingest.hpp"
#include "mh_ingest_check.hpp"
#include "mh_launch.hpp"
#include "mh_unbin.hpp"
#include "mh_unbin_layout.hpp"
#include "mh_windows.hpp"
#include "mh_windows_layout.hpp"
// built with -fvisibility=hidden: the mhi_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_ingest.h"
#pragma GCC visibility pop

namespace {

static_assert(mh::kGeoCrcWaves == mh::kCrcWaves && mh::kCrcMaxX == mh::kCrcMaxGroups, "mh_launch.hpp sizes the grid by mh_crc.hpp's constants");
static_assert(mh::kGeoApplyThreads == mh::kApplyThreads && mh::kGeoApplyMaxBlocks == mh::kApplyMaxBlocks,
              "mh_launch.hpp sizes the apply grids by mh_excess_layout.hpp's constants");
static_assert(mh::kAerLayoutColThreads == mh::kAerColThreads, "mh_aer_layout.hpp sizes the column grid by mh_aer.hpp's constant");
static_assert(mh::kAerMaxChannels == MHI_AER_MAX_CHANNELS, "the header publishes the layout's limit");
static_assert(mh::kUnbinCsr == MHI_UNBIN_CSR && mh::kUnbinAer == MHI_UNBIN_AER, "the header publishes the forms");
static_assert(mh::kExcessRows == MHI_EXCESS_ROWS && mh::kExcessCols == MHI_EXCESS_COLS, "the header publishes the forms");
static_assert(mh::kWinStack == MHI_WIN_STACK && mh::kWinSum == MHI_WIN_SUM, "the header publishes the forms");

// Where does a table live?  Only a query of the runtime's allocation records: nothing is enqueued, nothing waits.
uint32_t where_is(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // not an allocation the runtime knows (or no runtime at all): plain host memory
        return mh::kWhereHostOnly;
    }
    if (a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged) return mh::kWhereBoth;
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) return mh::kWhereDevice;
    return mh::kWhereHostOnly;
}

template <typename CH>
void aer_launch(const uint64_t *ticks, const void *channels, uint64_t n, uint32_t C, const mh::AerLayout &L, uint8_t *scratch,
                uint64_t *out_ticks, uint64_t *ev_off, uint64_t *dropped, hipStream_t st)
{
    uint32_t *const matrix = reinterpret_cast<uint32_t *>(scratch + L.off_matrix);
    uint32_t *const partial = reinterpret_cast<uint32_t *>(scratch + L.off_partial);
    uint32_t *const drop = reinterpret_cast<uint32_t *>(scratch + L.off_drop);
    const CH *const ch = static_cast<const CH *>(channels);
    const dim3 tiles(L.grid_tiles), waves(64u * L.waves);
    const dim3 cols(L.grid_cols_x, L.grid_cols_y), col(mh::kAerColThreads);
    if (L.rows) {
        hipLaunchKernelGGL(mh::k_aer_count<CH>, tiles, waves, L.lds_bytes, st, ch, n, C, L.run, L.rows, matrix, drop);
        hipLaunchKernelGGL(mh::k_aer_group_sum, cols, col, 0, st, matrix, C, L.rows, mh::kAerGroupRows, partial);
    }
    hipLaunchKernelGGL(mh::k_aer_scan, dim3(1), dim3(mh::kAerScanThreads), 0, st, partial, drop, C, L.rows, L.groups, ev_off,
                       dropped);
    if (L.rows) {
        hipLaunchKernelGGL(mh::k_aer_bases, cols, col, 0, st, matrix, partial, ev_off, C, L.rows, mh::kAerGroupRows);
        hipLaunchKernelGGL(mh::k_aer_scatter<CH>, tiles, waves, L.lds_bytes, st, ticks, ch, n, C, L.nbits, L.run, L.rows, matrix,
                           out_ticks);
    }
}

template <uint32_t FORM, typename CH>
void unbin_emit_launch(const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols, const mh::UnbinLayout &L,
                       uint64_t first_tick, uint64_t period, const uint64_t *base, uint64_t *out_ticks, void *out_ch,
                       uint64_t capacity, uint64_t *over, hipStream_t st)
{
    const dim3 grid(L.grid), block(64u * mh::kUnbinWaves);
    hipLaunchKernelGGL((mh::k_unbin_emit<FORM, CH>), grid, block, 0, st, in, row_off, cols, (uint32_t)L.tiles_per_row,
                       rows * cols, (uint32_t)L.tiles, first_tick, period, base, out_ticks, static_cast<CH *>(out_ch), capacity,
                       reinterpret_cast<unsigned long long *>(over));
}

// The scan mhi_unbin_count and mhi_excess_count end in, over the three regions of their scratch (u32 sums[pieces], u64
// base[pieces], u64 partial[groups + 1]): the pieces' sums become their 64-bit bases, *total the sum of all, and -- where
// `offs` is given -- offs[0 .. n_rows] the base of every row's first piece (`per` pieces to a row) and the total.
void scan_launch(uint8_t *scratch, uint64_t off_sum, uint64_t off_base, uint64_t off_partial, uint32_t pieces, uint32_t per,
                 uint64_t groups, uint32_t grid_scan, uint64_t *total, uint64_t *offs, uint64_t n_rows, hipStream_t st)
{
    uint32_t *const sums = reinterpret_cast<uint32_t *>(scratch + off_sum);
    uint64_t *const base = reinterpret_cast<uint64_t *>(scratch + off_base);
    uint64_t *const partial = reinterpret_cast<uint64_t *>(scratch + off_partial);
    const dim3 grid(grid_scan), per_group(mh::kUnbinBaseThreads);
    hipLaunchKernelGGL(mh::k_unbin_group_sum, grid, per_group, 0, st, sums, pieces, partial);
    hipLaunchKernelGGL(mh::k_unbin_scan, dim3(1), dim3(mh::kUnbinScanThreads), 0, st, partial, groups, total, offs, n_rows);
    hipLaunchKernelGGL(mh::k_unbin_bases, grid, per_group, 0, st, sums, pieces, partial, base, per, offs);
}

}  // namespace

extern "C" {

int mhi_version(void) { return MH_VERSION; }

const char *mhi_last_error(void) { return g_err; }

int mhi_bin_events(const uint64_t *ticks, const uint64_t *ev_off, uint32_t C, uint64_t origin, uint64_t period,
                   uint64_t T, uint32_t bits, uint8_t *out, const uint64_t *out_off, uint64_t chunk_stride,
                   void *stream)
{
    const mh::BinArgs a = {(uintptr_t)ticks, (uintptr_t)ev_off, C, origin, period, T, bits, (uintptr_t)out, (uintptr_t)out_off,
                           chunk_stride};
    mh::Msg m;
    mh::BinLaunch l;  // chunks per workgroup and the grid (mh_launch.hpp)
    if (int rc = mh::bin_events_check(m, a)) return fail(rc, m);
    // a packed call's out_off is walked where the host can read it: the runtime is asked only once the rest holds
    if (int rc = mh::bin_events_table_check(m, a, bits != 8 ? where_is(out_off) : mh::kWhereDevice, &l)) return fail(rc, m);
    const dim3 grid(l.grid), block(mh::kBinThreads);
    hipStream_t st = (hipStream_t)stream;
    if (bits == 8)
        hipLaunchKernelGGL(mh::k_bin_events<8>, grid, block, 0, st, ticks, ev_off, origin, period, T, l.nchunks, l.span, l.nspans,
                           l.div_mode, out, out_off, chunk_stride);
    else if (bits == 4)
        hipLaunchKernelGGL(mh::k_bin_events<4>, grid, block, 0, st, ticks, ev_off, origin, period, T, l.nchunks, l.span, l.nspans,
                           l.div_mode, out, out_off, chunk_stride);
    else
        hipLaunchKernelGGL(mh::k_bin_events<2>, grid, block, 0, st, ticks, ev_off, origin, period, T, l.nchunks, l.span, l.nspans,
                           l.div_mode, out, out_off, chunk_stride);
    return launched("mhi_bin_events");
}

int mhi_aer_scratch_bytes(uint64_t n, uint32_t C, uint64_t *bytes)
{
    mh::Msg m;
    mh::AerLayout L;
    if (int rc = mh::aer_scratch_check(m, n, C, (uintptr_t)bytes, &L)) return fail(rc, m);
    *bytes = L.bytes;
    return MH_OK;
}

int mhi_aer_to_csr(const uint64_t *ticks, const void *channels, uint32_t ch_bits, uint64_t n, uint32_t C,
                   uint64_t *out_ticks, uint64_t *ev_off, uint64_t *dropped, void *scratch, uint64_t scratch_bytes,
                   void *stream)
{
    const mh::AerArgs a = {(uintptr_t)ticks, (uintptr_t)channels, ch_bits, n, C, (uintptr_t)out_ticks, (uintptr_t)ev_off,
                           (uintptr_t)dropped, (uintptr_t)scratch, scratch_bytes};
    mh::Msg m;
    mh::AerLayout L;  // the sub-runs, the scratch sections and the grids (mh_aer_layout.hpp)
    if (int rc = mh::aer_check(m, a, &L)) return fail(rc, m);
    hipStream_t st = (hipStream_t)stream;
    if (ch_bits == 16)
        aer_launch<uint16_t>(ticks, channels, n, C, L, (uint8_t *)scratch, out_ticks, ev_off, dropped, st);
    else
        aer_launch<uint32_t>(ticks, channels, n, C, L, (uint8_t *)scratch, out_ticks, ev_off, dropped, st);
    return launched("mhi_aer_to_csr");
}

int mhi_seg_crc32(const void *payload, uint64_t payload_words, const uint64_t *seg_off, const uint64_t *seg_words,
                  uint64_t n_segments, const uint64_t *seg_idx, uint64_t n_idx, uint32_t *crc, const uint32_t *expect,
                  uint64_t *bad, void *stream)
{
    const mh::CrcArgs a = {(uintptr_t)payload, payload_words, (uintptr_t)seg_off, (uintptr_t)seg_words, n_segments,
                           (uintptr_t)seg_idx, n_idx, (uintptr_t)crc, (uintptr_t)expect, (uintptr_t)bad};
    mh::Msg m;
    mh::CrcLaunch l;  // the length of the list and the capped grid (mh_launch.hpp)
    if (int rc = mh::seg_crc_check(m, a, &l)) return fail(rc, m);
    if (l.n_list == 0) return MH_OK;
    const dim3 grid(l.grid), block(64u * mh::kCrcWaves);
    hipLaunchKernelGGL(mh::k_seg_crc32, grid, block, 0, (hipStream_t)stream, static_cast<const uint32_t *>(payload),
                       payload_words, seg_off, seg_words, n_segments, seg_idx, l.n_list, crc, expect,
                       reinterpret_cast<unsigned long long *>(bad));
    return launched("mhi_seg_crc32");
}

int mhi_unbin_scratch_bytes(uint32_t form, uint64_t rows, uint64_t cols, uint64_t *bytes)
{
    mh::Msg m;
    mh::UnbinLayout L;
    if (int rc = mh::unbin_scratch_check(m, form, rows, cols, (uintptr_t)bytes, &L)) return fail(rc, m);
    *bytes = L.bytes;
    return MH_OK;
}

int mhi_unbin_count(uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
                    uint64_t *ev_off, uint64_t *total, void *scratch, uint64_t scratch_bytes, void *stream)
{
    const mh::UnbinCountArgs a = {{form, (uintptr_t)in, (uintptr_t)row_off, rows, cols, (uintptr_t)scratch, scratch_bytes},
                                  (uintptr_t)ev_off, (uintptr_t)total};
    mh::Msg m;
    mh::UnbinLayout L;  // the tiles, the scratch sections and the grids (mh_unbin_layout.hpp)
    if (int rc = mh::unbin_count_check(m, a, &L)) return fail(rc, m);
    uint8_t *const s8 = static_cast<uint8_t *>(scratch);
    uint32_t *const sums = reinterpret_cast<uint32_t *>(s8 + L.off_sum);
    const uint32_t tiles = (uint32_t)L.tiles, tpr = (uint32_t)L.tiles_per_row;
    const dim3 grid(L.grid), block(64u * mh::kUnbinWaves);
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kUnbinCsr)
        hipLaunchKernelGGL(mh::k_unbin_count<mh::kUnbinCsr>, grid, block, 0, st, in, row_off, cols, tpr, rows * cols, tiles, sums);
    else
        hipLaunchKernelGGL(mh::k_unbin_count<mh::kUnbinAer>, grid, block, 0, st, in, row_off, cols, tpr, rows * cols, tiles, sums);
    scan_launch(s8, L.off_sum, L.off_base, L.off_partial, tiles, tpr, L.groups, L.grid_scan, total,
                form == mh::kUnbinCsr ? ev_off : nullptr, rows, st);
    return launched("mhi_unbin_count");
}

int mhi_unbin_emit(uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
                   uint64_t origin, uint64_t period, uint64_t phase, uint64_t *out_ticks, void *out_ch, uint32_t ch_bits,
                   uint64_t capacity, uint64_t *over, void *scratch, uint64_t scratch_bytes, void *stream)
{
    const mh::UnbinEmitArgs a = {{form, (uintptr_t)in, (uintptr_t)row_off, rows, cols, (uintptr_t)scratch, scratch_bytes},
                                 origin, period, phase, (uintptr_t)out_ticks, (uintptr_t)out_ch, ch_bits, capacity,
                                 (uintptr_t)over};
    mh::Msg m;
    mh::UnbinLayout L;
    if (int rc = mh::unbin_emit_check(m, a, &L)) return fail(rc, m);
    const uint8_t *const s8 = static_cast<const uint8_t *>(scratch);
    const uint64_t *const base = reinterpret_cast<const uint64_t *>(s8 + L.off_base);
    const uint64_t first_tick = origin + phase;
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kUnbinCsr)
        unbin_emit_launch<mh::kUnbinCsr, uint32_t>(in, row_off, rows, cols, L, first_tick, period, base, out_ticks, nullptr, capacity,
                                                   over, st);
    else if (ch_bits == 16)
        unbin_emit_launch<mh::kUnbinAer, uint16_t>(in, row_off, rows, cols, L, first_tick, period, base, out_ticks, out_ch, capacity,
                                                   over, st);
    else
        unbin_emit_launch<mh::kUnbinAer, uint32_t>(in, row_off, rows, cols, L, first_tick, period, base, out_ticks, out_ch, capacity,
                                                   over, st);
    return launched("mhi_unbin_emit");
}

int mhi_excess_scratch_bytes(uint32_t form, uint64_t rows, uint64_t cols, uint64_t *bytes)
{
    mh::Msg m;
    mh::ExcessLayout L;
    if (int rc = mh::excess_scratch_check(m, form, rows, cols, (uintptr_t)bytes, &L)) return fail(rc, m);
    *bytes = L.bytes;
    return MH_OK;
}

int mhi_excess_count(uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo, const uint64_t *hi,
                     uint64_t rows, uint64_t cols, uint32_t threshold, uint64_t *exc_off, uint64_t *total, void *scratch,
                     uint64_t scratch_bytes, void *stream)
{
    const mh::ExcessCountArgs a = {{form, (uintptr_t)in, (uintptr_t)row_off, (uintptr_t)lo, (uintptr_t)hi, rows, cols, threshold,
                                    (uintptr_t)scratch, scratch_bytes},
                                   (uintptr_t)exc_off, (uintptr_t)total};
    mh::Msg m;
    mh::ExcessLayout L;  // the pieces, the scratch sections and the grids (mh_excess_layout.hpp)
    if (int rc = mh::excess_count_check(m, a, &L)) return fail(rc, m);
    uint8_t *const s8 = static_cast<uint8_t *>(scratch);
    uint32_t *const sums = reinterpret_cast<uint32_t *>(s8 + L.off_sum);
    const uint32_t pieces = (uint32_t)L.pieces, per = (uint32_t)L.per_channel, k = (255u - threshold) * 0x01010101u;
    const dim3 grid(L.grid), block(64u * mh::kExcessWaves);
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kExcessRows)
        hipLaunchKernelGGL(mh::k_excess_rows_count, grid, block, 0, st, in, row_off, lo, hi, cols, per, pieces, k, sums);
    else
        hipLaunchKernelGGL(mh::k_excess_cols_count, grid, block, 0, st, in, rows, cols, per, L.waves, k, sums);
    scan_launch(s8, L.off_sum, L.off_base, L.off_partial, pieces, per, L.groups, L.grid_scan, total, exc_off, L.channels, st);
    return launched("mhi_excess_count");
}

int mhi_excess_emit(uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo, const uint64_t *hi,
                    uint64_t rows, uint64_t cols, uint32_t threshold, uint32_t *pos, uint8_t *val, uint64_t capacity,
                    uint64_t *over, void *scratch, uint64_t scratch_bytes, void *stream)
{
    const mh::ExcessEmitArgs a = {{form, (uintptr_t)in, (uintptr_t)row_off, (uintptr_t)lo, (uintptr_t)hi, rows, cols, threshold,
                                   (uintptr_t)scratch, scratch_bytes},
                                  (uintptr_t)pos, (uintptr_t)val, capacity, (uintptr_t)over};
    mh::Msg m;
    mh::ExcessLayout L;
    if (int rc = mh::excess_emit_check(m, a, &L)) return fail(rc, m);
    const uint8_t *const s8 = static_cast<const uint8_t *>(scratch);
    const uint64_t *const base = reinterpret_cast<const uint64_t *>(s8 + L.off_base);
    const uint32_t pieces = (uint32_t)L.pieces, per = (uint32_t)L.per_channel, k = (255u - threshold) * 0x01010101u;
    const dim3 grid(L.grid), block(64u * mh::kExcessWaves);
    unsigned long long *const ov = reinterpret_cast<unsigned long long *>(over);
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kExcessRows)
        hipLaunchKernelGGL(mh::k_excess_rows_emit, grid, block, 0, st, in, row_off, lo, hi, cols, per, pieces, k, threshold, base,
                           pos, val, capacity, ov);
    else
        hipLaunchKernelGGL(mh::k_excess_cols_emit, grid, block, 0, st, in, rows, cols, per, L.waves, k, threshold, base, pos, val,
                           capacity, ov);
    return launched("mhi_excess_emit");
}

int mhi_excess_apply(const uint32_t *pos, const uint8_t *val, uint64_t n_entries, const uint64_t *first, const uint64_t *last,
                     uint64_t n_rows, uint64_t start, uint64_t stop, uint64_t r, uint64_t lead, void *out, uint32_t out_bits,
                     uint64_t row_stride, uint64_t col_stride, void *stream)
{
    const mh::ApplyArgs a = {(uintptr_t)pos, (uintptr_t)val, n_entries, (uintptr_t)first, (uintptr_t)last, n_rows, start, stop, r,
                             lead, (uintptr_t)out, out_bits, row_stride, col_stride};
    mh::Msg m;
    mh::ApplyLayout L;  // a row's elements and its runs of kApplyRun (mh_excess_layout.hpp)
    if (int rc = mh::excess_apply_check(m, a, &L)) return fail(rc, m);
    if (L.runs == 0) return MH_OK;  // nothing to add
    uint8_t *const o8 = static_cast<uint8_t *>(out);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(mh::kApplyThreads);
    if (r == 1) {
        const mh::GridXY g = mh::excess_apply1_grid(n_entries, n_rows);  // capped in x and y (mh_launch.hpp)
        const dim3 grid(g.x, g.y);
        if (out_bits == 8)
            hipLaunchKernelGGL(mh::k_excess_apply1<uint8_t>, grid, block, 0, st, pos, val, n_entries, first, last, n_rows, start,
                               stop, lead, o8, row_stride, col_stride);
        else
            hipLaunchKernelGGL(mh::k_excess_apply1<uint32_t>, grid, block, 0, st, pos, val, n_entries, first, last, n_rows, start,
                               stop, lead, o8, row_stride, col_stride);
    } else {
        const dim3 grid(mh::excess_apply_grid(n_rows, L.runs));  // capped (mh_launch.hpp)
        if (out_bits == 8)
            hipLaunchKernelGGL(mh::k_excess_apply<uint8_t>, grid, block, 0, st, pos, val, n_entries, first, last, n_rows, start,
                               stop, r, lead, L.elements, L.runs, o8, row_stride, col_stride);
        else
            hipLaunchKernelGGL(mh::k_excess_apply<uint32_t>, grid, block, 0, st, pos, val, n_entries, first, last, n_rows, start,
                               stop, r, lead, L.elements, L.runs, o8, row_stride, col_stride);
    }
    return launched("mhi_excess_apply");
}

int mhi_windows(const uint8_t *in, uint64_t row_stride, uint64_t rows, uint64_t cols, const uint64_t *win_off,
                const uint64_t *win_idx, uint64_t n_win, uint64_t n_out, uint64_t W, uint64_t r, uint32_t mode, void *out,
                uint32_t out_bits, uint64_t out_win_stride, uint64_t out_row_stride, uint64_t *sumsq, uint64_t sq_row_stride,
                uint32_t accumulate, uint64_t *bad, void *stream)
{
    const mh::WinArgs a = {(uintptr_t)in, row_stride, rows, cols, (uintptr_t)win_off, (uintptr_t)win_idx, n_win, n_out, W, r, mode,
                           (uintptr_t)out, out_bits, out_win_stride, out_row_stride, (uintptr_t)sumsq, sq_row_stride, accumulate,
                           (uintptr_t)bad};
    mh::Msg m;
    if (int rc = mh::windows_check(m, a)) return fail(rc, m);
    mh::WinLayout L;  // the form, the tiles and the capped grid (mh_windows_layout.hpp)
    mh::windows_layout(mode, rows, W, r, n_win, &L);
    if (L.items == 0) return MH_OK;  // STACK of no windows
    const mh::WinParams p = {in, row_stride, rows, cols, win_off, win_idx, n_out, (uint32_t)n_win, (uint32_t)W, (uint32_t)r, L.nb,
                             L.tile_bins, L.tiles, L.items, static_cast<uint8_t *>(out), out_win_stride, out_row_stride,
                             reinterpret_cast<uint8_t *>(sumsq), sq_row_stride, accumulate,
                             reinterpret_cast<unsigned long long *>(bad)};
    const dim3 grid(L.grid), block(mh::kWinThreads);
    hipStream_t st = (hipStream_t)stream;
    const bool sum = mode == mh::kWinSum, o32 = out_bits == 32, sq = sumsq != nullptr;
#define MH_WIN_GO(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, st, p)
    if (L.form == mh::kWinLane) {
        if (!sum && o32) MH_WIN_GO(mh::k_win_lane_stack<true>);
        else if (!sum) MH_WIN_GO(mh::k_win_lane_stack<false>);
        else if (sq) MH_WIN_GO(mh::k_win_lane_sum<true>);
        else MH_WIN_GO(mh::k_win_lane_sum<false>);
    } else if (L.form == mh::kWinStage) {
        if (!sum && o32) MH_WIN_GO((mh::k_win_stage<false, true, false>));
        else if (!sum) MH_WIN_GO((mh::k_win_stage<false, false, false>));
        else if (sq) MH_WIN_GO((mh::k_win_stage<true, true, true>));
        else MH_WIN_GO((mh::k_win_stage<true, true, false>));
    } else {
        if (!sum && o32) MH_WIN_GO((mh::k_win_wave<false, true, false>));
        else if (!sum) MH_WIN_GO((mh::k_win_wave<false, false, false>));
        else if (sq) MH_WIN_GO((mh::k_win_wave<true, true, true>));
        else MH_WIN_GO((mh::k_win_wave<true, true, false>));
    }
#undef MH_WIN_GO
    return launched("mhi_windows");
}

int mhi_gram(const uint8_t *a, uint64_t a_row_stride, uint64_t a_rows, const uint8_t *b, uint64_t b_row_stride, uint64_t b_rows,
             uint64_t cols, int64_t *gram, uint64_t gram_row_stride, int64_t *sum_a, int64_t *sum_b, uint32_t accumulate,
             void *stream)
{
    const mh::GramArgs g = {(uintptr_t)a, a_row_stride, a_rows, (uintptr_t)b, b_row_stride, b_rows, cols, (uintptr_t)gram,
                            gram_row_stride, (uintptr_t)sum_a, (uintptr_t)sum_b, accumulate};
    mh::Msg m;
    if (int rc = mh::gram_check(m, g)) return fail(rc, m);
    const bool symmetric = b == nullptr;
    if (symmetric) b = a, b_row_stride = a_row_stride, b_rows = a_rows;
    mh::GramLayout L;  // the tiles, the runs of K slices and the capped grid (mh_gram_layout.hpp)
    mh::gram_layout(a_rows, b_rows, cols, symmetric, &L);
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) {
        hipError_t e = a_rows == 1 || gram_row_stride == 8 * b_rows
                           ? hipMemsetAsync(gram, 0, a_rows == 1 ? 8 * b_rows : a_rows * gram_row_stride, st)
                           : hipMemset2DAsync(gram, gram_row_stride, 0, 8 * b_rows, a_rows, st);
        if (e == hipSuccess && sum_a) e = hipMemsetAsync(sum_a, 0, 8 * a_rows, st);
        if (e == hipSuccess && sum_b) e = hipMemsetAsync(sum_b, 0, 8 * b_rows, st);
        if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_gram: zeroing the result failed: %s", hipGetErrorString(e));
    }
    const mh::GramParams p = {a, a_row_stride, a_rows, b, b_row_stride, b_rows, cols, reinterpret_cast<uint8_t *>(gram),
                              gram_row_stride, reinterpret_cast<unsigned long long *>(sum_a),
                              reinterpret_cast<unsigned long long *>(sum_b), L.symmetric, L.nta, L.ntb, L.run_slices, L.tiles,
                              L.items};
    hipLaunchKernelGGL(mh::k_gram, dim3(L.grid), dim3(mh::kGramThreads), 0, st, p);
    return launched("mhi_gram");
}

}  // extern "C"
