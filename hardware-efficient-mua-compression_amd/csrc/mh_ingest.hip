// mh_ingest.hip -- C ABI (include/muahuff_ingest.h) over the binner kernel in mh_ingest.hpp, the pair-list partition
// in mh_aer.hpp, the segment checksum in mh_crc.hpp, the way back from counts to events in mh_unbin.hpp and the side
// list of what the clip at S-1 drops in mh_excess.hpp, the trial-aligned windows of a decoded recording in
// mh_windows.hpp and the channel-by-channel Gram matrix of one in mh_gram.hpp: argument checks and the launches.  A companion of libmuahuff.so, not part of it; there is no CPU
// fallback here either.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "mh_aer.hpp"
#include "mh_aer_layout.hpp"
#include "mh_crc.hpp"
#include "mh_excess.hpp"
#include "mh_excess_layout.hpp"
#include "mh_gram.hpp"
#include "mh_gram_layout.hpp"
#include "mh_ingest.hpp"
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

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static_assert(mh::kGeoCrcWaves == mh::kCrcWaves && mh::kCrcMaxX == mh::kCrcMaxGroups, "mh_launch.hpp sizes the grid by mh_crc.hpp's constants");
static_assert(mh::kGeoApplyThreads == mh::kApplyThreads && mh::kGeoApplyMaxBlocks == mh::kApplyMaxBlocks,
              "mh_launch.hpp sizes the apply grids by mh_excess_layout.hpp's constants");

// Where does a table live?  Only a query of the runtime's allocation records: nothing is enqueued, nothing waits.
enum class Where { kDevice, kBoth, kHostOnly };

Where where_is(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // not an allocation the runtime knows (or no runtime at all): plain host memory
        return Where::kHostOnly;
    }
    if (a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged) return Where::kBoth;
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) return Where::kDevice;
    return Where::kHostOnly;
}

template <typename CH>
void aer_launch(const uint64_t *ticks, const void *channels, uint64_t n, uint32_t C, const mh::AerLayout &L, uint8_t *scratch,
                uint64_t *out_ticks, uint64_t *ev_off, uint64_t *dropped, hipStream_t st)
{
    uint32_t *const matrix = reinterpret_cast<uint32_t *>(scratch + L.off_matrix);
    uint32_t *const partial = reinterpret_cast<uint32_t *>(scratch + L.off_partial);
    uint32_t *const drop = reinterpret_cast<uint32_t *>(scratch + L.off_drop);
    const CH *const ch = static_cast<const CH *>(channels);
    const dim3 tiles((unsigned)((L.rows + L.waves - 1) / L.waves)), waves(64u * L.waves);
    const dim3 cols((C + mh::kAerColThreads - 1) / mh::kAerColThreads, (unsigned)L.groups), col(mh::kAerColThreads);
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

// What mhi_unbin_count and mhi_unbin_emit share: the form, the shape and the scratch.  `fn` names the caller.
int unbin_args(const char *fn, uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
               const void *scratch, uint64_t scratch_bytes, mh::UnbinLayout *L)
{
    if (form != mh::kUnbinCsr && form != mh::kUnbinAer)
        return fail(MH_ERR_ARG, "%s: form=%u (MHI_UNBIN_CSR or MHI_UNBIN_AER)", fn, form);
    if (!in || !scratch) return fail(MH_ERR_ARG, "%s: NULL pointer", fn);
    if (form == mh::kUnbinCsr && !row_off) return fail(MH_ERR_ARG, "%s: the CSR form needs row_off", fn);
    if (form == mh::kUnbinAer && row_off) return fail(MH_ERR_ARG, "%s: the AER form is one contiguous block: row_off must be NULL", fn);
    const int rc = mh::unbin_layout(form, rows, cols, L);
    if (rc == -1)
        return fail(MH_ERR_ARG, "%s: rows=%llu, cols=%llu (each at least 1; AER form: cols <= 2^32)", fn,
                    (unsigned long long)rows, (unsigned long long)cols);
    if (rc) return fail(MH_ERR_ARG, "%s: rows=%llu, cols=%llu make more than 2^32 - 1 tiles", fn, (unsigned long long)rows,
                        (unsigned long long)cols);
    if (scratch_bytes < L->bytes)
        return fail(MH_ERR_ARG, "%s: scratch_bytes=%llu, mhi_unbin_scratch_bytes asks for %llu", fn,
                    (unsigned long long)scratch_bytes, (unsigned long long)L->bytes);
    if ((uintptr_t)scratch % 16) return fail(MH_ERR_ARG, "%s: scratch is not 16-byte aligned", fn);
    return MH_OK;
}

template <uint32_t FORM, typename CH>
void unbin_emit_launch(const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols, const mh::UnbinLayout &L,
                       uint64_t first_tick, uint64_t period, const uint64_t *base, uint64_t *out_ticks, void *out_ch,
                       uint64_t capacity, uint64_t *over, hipStream_t st)
{
    const dim3 grid((unsigned)((L.tiles + mh::kUnbinWaves - 1) / mh::kUnbinWaves)), block(64u * mh::kUnbinWaves);
    hipLaunchKernelGGL((mh::k_unbin_emit<FORM, CH>), grid, block, 0, st, in, row_off, cols, (uint32_t)L.tiles_per_row,
                       rows * cols, (uint32_t)L.tiles, first_tick, period, base, out_ticks, static_cast<CH *>(out_ch), capacity,
                       reinterpret_cast<unsigned long long *>(over));
}

// What mhi_excess_count and mhi_excess_emit share: the form, the shape, the threshold and the scratch.
int excess_args(const char *fn, uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo,
                const uint64_t *hi, uint64_t rows, uint64_t cols, uint32_t threshold, const void *scratch,
                uint64_t scratch_bytes, mh::ExcessLayout *L)
{
    if (form != mh::kExcessRows && form != mh::kExcessCols)
        return fail(MH_ERR_ARG, "%s: form=%u (MHI_EXCESS_ROWS or MHI_EXCESS_COLS)", fn, form);
    if (!in || !scratch) return fail(MH_ERR_ARG, "%s: NULL pointer", fn);
    if (form == mh::kExcessRows && !row_off) return fail(MH_ERR_ARG, "%s: the ROWS form needs row_off", fn);
    if (form == mh::kExcessCols && (row_off || lo || hi))
        return fail(MH_ERR_ARG, "%s: the COLS form is one contiguous block, every column whole: row_off, lo and hi must be NULL", fn);
    if (threshold < 1 || threshold > 254) return fail(MH_ERR_ARG, "%s: threshold=%u (1 .. 254)", fn, threshold);
    const int rc = mh::excess_layout(form, rows, cols, L);
    if (rc == -1)
        return fail(MH_ERR_ARG, "%s: rows=%llu, cols=%llu (each at least 1, cols below 2^32; COLS form: rows below 2^32)", fn,
                    (unsigned long long)rows, (unsigned long long)cols);
    if (rc) return fail(MH_ERR_ARG, "%s: rows=%llu, cols=%llu make more than 2^32 - 1 pieces", fn, (unsigned long long)rows,
                        (unsigned long long)cols);
    if (scratch_bytes < L->bytes)
        return fail(MH_ERR_ARG, "%s: scratch_bytes=%llu, mhi_excess_scratch_bytes asks for %llu", fn,
                    (unsigned long long)scratch_bytes, (unsigned long long)L->bytes);
    if ((uintptr_t)scratch % 16) return fail(MH_ERR_ARG, "%s: scratch is not 16-byte aligned", fn);
    return MH_OK;
}

}  // namespace

extern "C" {

int mhi_version(void) { return MH_VERSION; }

const char *mhi_last_error(void) { return g_err; }

int mhi_bin_events(const uint64_t *ticks, const uint64_t *ev_off, uint32_t C, uint64_t origin, uint64_t period,
                   uint64_t T, uint32_t bits, uint8_t *out, const uint64_t *out_off, uint64_t chunk_stride,
                   void *stream)
{
    if (!ticks || !ev_off || !out || !out_off) return fail(MH_ERR_ARG, "mhi_bin_events: NULL pointer");
    if (C == 0 || T == 0 || period == 0)
        return fail(MH_ERR_ARG, "mhi_bin_events: C=%u, T=%llu, period=%llu (each at least 1)", C, (unsigned long long)T,
                    (unsigned long long)period);
    if (bits != 8 && bits != 4 && bits != 2) return fail(MH_ERR_ARG, "mhi_bin_events: bits=%u (8, 4 or 2)", bits);
    if (!mh::chunk_stride_ok(chunk_stride, bits))
        return fail(MH_ERR_ARG, "mhi_bin_events: chunk_stride=%llu (packed output only, a multiple of 16, at least one chunk)",
                    (unsigned long long)chunk_stride);
    const unsigned __int128 end = (unsigned __int128)origin + (unsigned __int128)T * period;
    if (end > ((unsigned __int128)1 << 63))
        return fail(MH_ERR_ARG, "mhi_bin_events: origin + T*period exceeds 2^63 (origin=%llu, T=%llu, period=%llu)",
                    (unsigned long long)origin, (unsigned long long)T, (unsigned long long)period);
    if (bits != 8) {
        const Where w = where_is(out_off);
        if (w != Where::kDevice)
            for (uint32_t c = 0; c < C; ++c)
                if (out_off[c] % 16)
                    return fail(MH_ERR_ARG, "mhi_bin_events: out_off[%u]=%llu is not a multiple of 16 (packed output)", c,
                                (unsigned long long)out_off[c]);
        if (w == Where::kHostOnly) return fail(MH_ERR_ARG, "mhi_bin_events: out_off is host memory the device cannot read");
    }
    mh::Msg m;
    mh::BinLaunch l;  // chunks per workgroup and the grid (mh_launch.hpp)
    if (int rc = mh::bin_events_launch(m, C, T, period, &l)) return fail(rc, "%s", m.text);
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
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_bin_events: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_aer_scratch_bytes(uint64_t n, uint32_t C, uint64_t *bytes)
{
    static_assert(mh::kAerMaxChannels == MHI_AER_MAX_CHANNELS, "the header publishes the layout's limit");
    if (!bytes) return fail(MH_ERR_ARG, "mhi_aer_scratch_bytes: NULL pointer");
    mh::AerLayout L;
    const int rc = mh::aer_layout(n, C, &L);
    if (rc == -1)
        return fail(MH_ERR_ARG, "mhi_aer_scratch_bytes: C=%u (1 .. MHI_AER_MAX_CHANNELS = %u)", C, mh::kAerMaxChannels);
    if (rc) return fail(MH_ERR_ARG, "mhi_aer_scratch_bytes: n=%llu (below 2^32: positions are 32-bit)", (unsigned long long)n);
    *bytes = L.bytes;
    return MH_OK;
}

int mhi_aer_to_csr(const uint64_t *ticks, const void *channels, uint32_t ch_bits, uint64_t n, uint32_t C,
                   uint64_t *out_ticks, uint64_t *ev_off, uint64_t *dropped, void *scratch, uint64_t scratch_bytes,
                   void *stream)
{
    if (!ticks || !channels || !out_ticks || !ev_off || !dropped || !scratch)
        return fail(MH_ERR_ARG, "mhi_aer_to_csr: NULL pointer");
    if (ch_bits != 16 && ch_bits != 32) return fail(MH_ERR_ARG, "mhi_aer_to_csr: ch_bits=%u (16 or 32)", ch_bits);
    mh::AerLayout L;
    const int rc = mh::aer_layout(n, C, &L);
    if (rc == -1) return fail(MH_ERR_ARG, "mhi_aer_to_csr: C=%u (1 .. MHI_AER_MAX_CHANNELS = %u)", C, mh::kAerMaxChannels);
    if (rc) return fail(MH_ERR_ARG, "mhi_aer_to_csr: n=%llu (below 2^32: positions are 32-bit)", (unsigned long long)n);
    if (scratch_bytes < L.bytes)
        return fail(MH_ERR_ARG, "mhi_aer_to_csr: scratch_bytes=%llu, mhi_aer_scratch_bytes asks for %llu",
                    (unsigned long long)scratch_bytes, (unsigned long long)L.bytes);
    const uintptr_t a = (uintptr_t)ticks, b = (uintptr_t)out_ticks;
    if (n && a < b + n * 8 && b < a + n * 8) return fail(MH_ERR_ARG, "mhi_aer_to_csr: out_ticks overlaps ticks");
    if ((uintptr_t)scratch % 16)
        return fail(MH_ERR_ARG, "mhi_aer_to_csr: scratch is not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (ch_bits == 16)
        aer_launch<uint16_t>(ticks, channels, n, C, L, (uint8_t *)scratch, out_ticks, ev_off, dropped, st);
    else
        aer_launch<uint32_t>(ticks, channels, n, C, L, (uint8_t *)scratch, out_ticks, ev_off, dropped, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_aer_to_csr: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_seg_crc32(const void *payload, uint64_t payload_words, const uint64_t *seg_off, const uint64_t *seg_words,
                  uint64_t n_segments, const uint64_t *seg_idx, uint64_t n_idx, uint32_t *crc, const uint32_t *expect,
                  uint64_t *bad, void *stream)
{
    if (!payload || !seg_off || !seg_words) return fail(MH_ERR_ARG, "mhi_seg_crc32: NULL pointer");
    if (!crc && !expect) return fail(MH_ERR_ARG, "mhi_seg_crc32: neither crc nor expect is given");
    if (expect && !bad) return fail(MH_ERR_ARG, "mhi_seg_crc32: expect is given without bad");
    if ((uintptr_t)payload % 4) return fail(MH_ERR_ARG, "mhi_seg_crc32: payload is not 4-byte aligned");
    const uint64_t n_list = seg_idx ? n_idx : n_segments;
    if (n_list == 0) return MH_OK;
    const dim3 grid(mh::seg_crc_grid(n_list)), block(64u * mh::kCrcWaves);
    hipLaunchKernelGGL(mh::k_seg_crc32, grid, block, 0, (hipStream_t)stream, static_cast<const uint32_t *>(payload),
                       payload_words, seg_off, seg_words, n_segments, seg_idx, n_list, crc, expect,
                       reinterpret_cast<unsigned long long *>(bad));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_seg_crc32: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_unbin_scratch_bytes(uint32_t form, uint64_t rows, uint64_t cols, uint64_t *bytes)
{
    static_assert(mh::kUnbinCsr == MHI_UNBIN_CSR && mh::kUnbinAer == MHI_UNBIN_AER, "the header publishes the forms");
    if (!bytes) return fail(MH_ERR_ARG, "mhi_unbin_scratch_bytes: NULL pointer");
    mh::UnbinLayout L;
    const int rc = mh::unbin_layout(form, rows, cols, &L);
    if (rc == -1)
        return fail(MH_ERR_ARG, "mhi_unbin_scratch_bytes: form=%u, rows=%llu, cols=%llu (a known form, each at least 1; AER form: cols <= 2^32)",
                    form, (unsigned long long)rows, (unsigned long long)cols);
    if (rc)
        return fail(MH_ERR_ARG, "mhi_unbin_scratch_bytes: rows=%llu, cols=%llu make more than 2^32 - 1 tiles",
                    (unsigned long long)rows, (unsigned long long)cols);
    *bytes = L.bytes;
    return MH_OK;
}

int mhi_unbin_count(uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
                    uint64_t *ev_off, uint64_t *total, void *scratch, uint64_t scratch_bytes, void *stream)
{
    mh::UnbinLayout L;
    const int rc = unbin_args("mhi_unbin_count", form, in, row_off, rows, cols, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (!total) return fail(MH_ERR_ARG, "mhi_unbin_count: NULL pointer");
    if (form == mh::kUnbinCsr && !ev_off) return fail(MH_ERR_ARG, "mhi_unbin_count: the CSR form needs ev_off");
    uint8_t *const s8 = static_cast<uint8_t *>(scratch);
    uint32_t *const sums = reinterpret_cast<uint32_t *>(s8 + L.off_sum);
    uint64_t *const base = reinterpret_cast<uint64_t *>(s8 + L.off_base);
    uint64_t *const partial = reinterpret_cast<uint64_t *>(s8 + L.off_partial);
    const uint32_t tiles = (uint32_t)L.tiles, tpr = (uint32_t)L.tiles_per_row;
    const dim3 grid((unsigned)((L.tiles + mh::kUnbinWaves - 1) / mh::kUnbinWaves)), block(64u * mh::kUnbinWaves);
    const dim3 groups((unsigned)L.groups), per_group(mh::kUnbinBaseThreads);
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kUnbinCsr)
        hipLaunchKernelGGL(mh::k_unbin_count<mh::kUnbinCsr>, grid, block, 0, st, in, row_off, cols, tpr, rows * cols, tiles, sums);
    else
        hipLaunchKernelGGL(mh::k_unbin_count<mh::kUnbinAer>, grid, block, 0, st, in, row_off, cols, tpr, rows * cols, tiles, sums);
    hipLaunchKernelGGL(mh::k_unbin_group_sum, groups, per_group, 0, st, sums, tiles, partial);
    uint64_t *const offs = form == mh::kUnbinCsr ? ev_off : nullptr;
    hipLaunchKernelGGL(mh::k_unbin_scan, dim3(1), dim3(mh::kUnbinScanThreads), 0, st, partial, L.groups, total, offs, rows);
    hipLaunchKernelGGL(mh::k_unbin_bases, groups, per_group, 0, st, sums, tiles, partial, base, tpr, offs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_unbin_count: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_unbin_emit(uint32_t form, const uint8_t *in, const uint64_t *row_off, uint64_t rows, uint64_t cols,
                   uint64_t origin, uint64_t period, uint64_t phase, uint64_t *out_ticks, void *out_ch, uint32_t ch_bits,
                   uint64_t capacity, uint64_t *over, void *scratch, uint64_t scratch_bytes, void *stream)
{
    mh::UnbinLayout L;
    const int rc = unbin_args("mhi_unbin_emit", form, in, row_off, rows, cols, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (!out_ticks || !over) return fail(MH_ERR_ARG, "mhi_unbin_emit: NULL pointer");
    if (period == 0 || phase >= period)
        return fail(MH_ERR_ARG, "mhi_unbin_emit: period=%llu, phase=%llu (period at least 1, phase below it)",
                    (unsigned long long)period, (unsigned long long)phase);
    const uint64_t steps = form == mh::kUnbinCsr ? cols : rows;
    const unsigned __int128 last = (unsigned __int128)origin + (unsigned __int128)(steps - 1) * period + phase;
    if (last >= ((unsigned __int128)1 << 63))
        return fail(MH_ERR_ARG, "mhi_unbin_emit: the largest tick reaches 2^63 (origin=%llu, period=%llu, phase=%llu, %llu steps)",
                    (unsigned long long)origin, (unsigned long long)period, (unsigned long long)phase,
                    (unsigned long long)steps);
    if (form == mh::kUnbinAer) {
        if (!out_ch) return fail(MH_ERR_ARG, "mhi_unbin_emit: the AER form needs out_ch");
        if (ch_bits != 16 && ch_bits != 32) return fail(MH_ERR_ARG, "mhi_unbin_emit: ch_bits=%u (16 or 32)", ch_bits);
        if (ch_bits == 16 && cols > 65536)
            return fail(MH_ERR_ARG, "mhi_unbin_emit: cols=%llu does not fit 16-bit channels", (unsigned long long)cols);
    }
    {   // out_ticks[0 .. capacity) against the input: the whole block in the AER form, where its extent is known here
        const unsigned __int128 a = (uintptr_t)in, b = (uintptr_t)out_ticks;
        const unsigned __int128 na = form == mh::kUnbinAer ? (unsigned __int128)rows * cols : 1, nb = (unsigned __int128)capacity * 8;
        if (nb && a < b + nb && b < a + na) return fail(MH_ERR_ARG, "mhi_unbin_emit: out_ticks overlaps the input");
    }
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
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_unbin_emit: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_excess_scratch_bytes(uint32_t form, uint64_t rows, uint64_t cols, uint64_t *bytes)
{
    static_assert(mh::kExcessRows == MHI_EXCESS_ROWS && mh::kExcessCols == MHI_EXCESS_COLS, "the header publishes the forms");
    if (!bytes) return fail(MH_ERR_ARG, "mhi_excess_scratch_bytes: NULL pointer");
    mh::ExcessLayout L;
    const int rc = mh::excess_layout(form, rows, cols, &L);
    if (rc == -1)
        return fail(MH_ERR_ARG, "mhi_excess_scratch_bytes: form=%u, rows=%llu, cols=%llu (a known form, each at least 1, cols below 2^32; COLS form: rows below 2^32)",
                    form, (unsigned long long)rows, (unsigned long long)cols);
    if (rc)
        return fail(MH_ERR_ARG, "mhi_excess_scratch_bytes: rows=%llu, cols=%llu make more than 2^32 - 1 pieces",
                    (unsigned long long)rows, (unsigned long long)cols);
    *bytes = L.bytes;
    return MH_OK;
}

int mhi_excess_count(uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo, const uint64_t *hi,
                     uint64_t rows, uint64_t cols, uint32_t threshold, uint64_t *exc_off, uint64_t *total, void *scratch,
                     uint64_t scratch_bytes, void *stream)
{
    mh::ExcessLayout L;
    const int rc = excess_args("mhi_excess_count", form, in, row_off, lo, hi, rows, cols, threshold, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (!exc_off || !total) return fail(MH_ERR_ARG, "mhi_excess_count: NULL pointer");
    uint8_t *const s8 = static_cast<uint8_t *>(scratch);
    uint32_t *const sums = reinterpret_cast<uint32_t *>(s8 + L.off_sum);
    uint64_t *const base = reinterpret_cast<uint64_t *>(s8 + L.off_base);
    uint64_t *const partial = reinterpret_cast<uint64_t *>(s8 + L.off_partial);
    const uint32_t pieces = (uint32_t)L.pieces, per = (uint32_t)L.per_channel, k = (255u - threshold) * 0x01010101u;
    const dim3 block(64u * mh::kExcessWaves), groups((unsigned)L.groups), per_group(mh::kUnbinBaseThreads);
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kExcessRows) {
        const dim3 grid((unsigned)((L.pieces + mh::kExcessWaves - 1) / mh::kExcessWaves));
        hipLaunchKernelGGL(mh::k_excess_rows_count, grid, block, 0, st, in, row_off, lo, hi, cols, per, pieces, k, sums);
    } else {
        const uint64_t waves = L.strips * L.per_channel;
        const dim3 grid((unsigned)((waves + mh::kExcessWaves - 1) / mh::kExcessWaves));
        hipLaunchKernelGGL(mh::k_excess_cols_count, grid, block, 0, st, in, rows, cols, per, waves, k, sums);
    }
    hipLaunchKernelGGL(mh::k_unbin_group_sum, groups, per_group, 0, st, sums, pieces, partial);
    hipLaunchKernelGGL(mh::k_unbin_scan, dim3(1), dim3(mh::kUnbinScanThreads), 0, st, partial, L.groups, total, exc_off, L.channels);
    hipLaunchKernelGGL(mh::k_unbin_bases, groups, per_group, 0, st, sums, pieces, partial, base, per, exc_off);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_excess_count: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_excess_emit(uint32_t form, const uint8_t *in, const uint64_t *row_off, const uint64_t *lo, const uint64_t *hi,
                    uint64_t rows, uint64_t cols, uint32_t threshold, uint32_t *pos, uint8_t *val, uint64_t capacity,
                    uint64_t *over, void *scratch, uint64_t scratch_bytes, void *stream)
{
    mh::ExcessLayout L;
    const int rc = excess_args("mhi_excess_emit", form, in, row_off, lo, hi, rows, cols, threshold, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (!pos || !val || !over) return fail(MH_ERR_ARG, "mhi_excess_emit: NULL pointer");
    if ((uintptr_t)pos % 4) return fail(MH_ERR_ARG, "mhi_excess_emit: pos is not 4-byte aligned");
    const uint8_t *const s8 = static_cast<const uint8_t *>(scratch);
    const uint64_t *const base = reinterpret_cast<const uint64_t *>(s8 + L.off_base);
    const uint32_t pieces = (uint32_t)L.pieces, per = (uint32_t)L.per_channel, k = (255u - threshold) * 0x01010101u;
    const dim3 block(64u * mh::kExcessWaves);
    unsigned long long *const ov = reinterpret_cast<unsigned long long *>(over);
    hipStream_t st = (hipStream_t)stream;
    if (form == mh::kExcessRows) {
        const dim3 grid((unsigned)((L.pieces + mh::kExcessWaves - 1) / mh::kExcessWaves));
        hipLaunchKernelGGL(mh::k_excess_rows_emit, grid, block, 0, st, in, row_off, lo, hi, cols, per, pieces, k, threshold, base,
                           pos, val, capacity, ov);
    } else {
        const uint64_t waves = L.strips * L.per_channel;
        const dim3 grid((unsigned)((waves + mh::kExcessWaves - 1) / mh::kExcessWaves));
        hipLaunchKernelGGL(mh::k_excess_cols_emit, grid, block, 0, st, in, rows, cols, per, waves, k, threshold, base, pos, val,
                           capacity, ov);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_excess_emit: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_excess_apply(const uint32_t *pos, const uint8_t *val, uint64_t n_entries, const uint64_t *first, const uint64_t *last,
                     uint64_t n_rows, uint64_t start, uint64_t stop, uint64_t r, uint64_t lead, void *out, uint32_t out_bits,
                     uint64_t row_stride, uint64_t col_stride, void *stream)
{
    if (!first || !last || !out || (n_entries && (!pos || !val))) return fail(MH_ERR_ARG, "mhi_excess_apply: NULL pointer");
    if (out_bits != 8 && out_bits != 32) return fail(MH_ERR_ARG, "mhi_excess_apply: out_bits=%u (8 or 32)", out_bits);
    if (r == 0 || r > mh::kExcessMaxLen || lead >= mh::kExcessMaxLen)
        return fail(MH_ERR_ARG, "mhi_excess_apply: r=%llu, lead=%llu (r 1 .. 2^32, lead below 2^32)", (unsigned long long)r,
                    (unsigned long long)lead);
    if (start > stop || stop > mh::kExcessMaxLen)
        return fail(MH_ERR_ARG, "mhi_excess_apply: start=%llu, stop=%llu (start <= stop <= 2^32)", (unsigned long long)start,
                    (unsigned long long)stop);
    if (out_bits == 32 && ((uintptr_t)out % 4 || row_stride % 4 || col_stride % 4))
        return fail(MH_ERR_ARG, "mhi_excess_apply: out_bits=32 needs out and both strides to be multiples of 4");
    if ((uintptr_t)pos % 4) return fail(MH_ERR_ARG, "mhi_excess_apply: pos is not 4-byte aligned");
    if (n_rows == 0 || n_entries == 0 || start == stop) return MH_OK;  // nothing to add
    const uint64_t elements = mh::apply_elements(start, stop, r, lead);
    const uint64_t runs = (elements + mh::kApplyRun - 1) / mh::kApplyRun;
    if ((unsigned __int128)n_rows * runs >= ((unsigned __int128)1 << 63))
        return fail(MH_ERR_ARG, "mhi_excess_apply: n_rows=%llu is too large", (unsigned long long)n_rows);
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
        const dim3 grid(mh::excess_apply_grid(n_rows, runs));  // capped (mh_launch.hpp)
        if (out_bits == 8)
            hipLaunchKernelGGL(mh::k_excess_apply<uint8_t>, grid, block, 0, st, pos, val, n_entries, first, last, n_rows, start,
                               stop, r, lead, elements, runs, o8, row_stride, col_stride);
        else
            hipLaunchKernelGGL(mh::k_excess_apply<uint32_t>, grid, block, 0, st, pos, val, n_entries, first, last, n_rows, start,
                               stop, r, lead, elements, runs, o8, row_stride, col_stride);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_excess_apply: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_windows(const uint8_t *in, uint64_t row_stride, uint64_t rows, uint64_t cols, const uint64_t *win_off,
                const uint64_t *win_idx, uint64_t n_win, uint64_t n_out, uint64_t W, uint64_t r, uint32_t mode, void *out,
                uint32_t out_bits, uint64_t out_win_stride, uint64_t out_row_stride, uint64_t *sumsq, uint64_t sq_row_stride,
                uint32_t accumulate, uint64_t *bad, void *stream)
{
    static_assert(mh::kWinStack == MHI_WIN_STACK && mh::kWinSum == MHI_WIN_SUM, "the header publishes the forms");
    const mh::WinArgs a = {(uintptr_t)in, row_stride, rows, cols, (uintptr_t)win_off, (uintptr_t)win_idx, n_win, n_out, W, r, mode,
                           (uintptr_t)out, out_bits, out_win_stride, out_row_stride, (uintptr_t)sumsq, sq_row_stride, accumulate,
                           (uintptr_t)bad};
    mh::Msg m;
    if (int rc = mh::windows_check(m, a)) return fail(rc, "%s", m.text);
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
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_windows: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

int mhi_gram(const uint8_t *a, uint64_t a_row_stride, uint64_t a_rows, const uint8_t *b, uint64_t b_row_stride, uint64_t b_rows,
             uint64_t cols, int64_t *gram, uint64_t gram_row_stride, int64_t *sum_a, int64_t *sum_b, uint32_t accumulate,
             void *stream)
{
    const mh::GramArgs g = {(uintptr_t)a, a_row_stride, a_rows, (uintptr_t)b, b_row_stride, b_rows, cols, (uintptr_t)gram,
                            gram_row_stride, (uintptr_t)sum_a, (uintptr_t)sum_b, accumulate};
    mh::Msg m;
    if (int rc = mh::gram_check(m, g)) return fail(rc, "%s", m.text);
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
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_gram: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

}  // extern "C"
