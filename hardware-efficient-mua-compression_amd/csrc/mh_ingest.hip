// mh_ingest.hip -- C ABI (include/muahuff_ingest.h) over the binner kernel in mh_ingest.hpp, the pair-list partition
// in mh_aer.hpp and the segment checksum in mh_crc.hpp: argument checks and the launches.  A companion of libmuahuff.so, not part of it; there is no CPU
// fallback here either.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "mh_aer.hpp"
#include "mh_aer_layout.hpp"
#include "mh_crc.hpp"
#include "mh_ingest.hpp"
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
    if (chunk_stride && (bits == 8 || chunk_stride % 16 || chunk_stride < (uint64_t)MH_CHUNK * bits / 8))
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
    const uint64_t nchunks = (T + MH_CHUNK - 1) / MH_CHUNK;
    // chunks per workgroup: 8 amortise the start search and keep the event list streaming; fewer when that would leave
    // the device short of workgroups, more when the grid would not fit one dimension
    uint64_t span = 8;
    while (span > 1 && (unsigned __int128)C * ((nchunks + span - 1) / span) < 4096) span >>= 1;
    while ((unsigned __int128)C * ((nchunks + span - 1) / span) > 0x7FFFFFFFull) span <<= 1;
    const uint64_t nspans = (nchunks + span - 1) / span;
    const uint32_t div_mode = period == 1 ? 0u : period < (1ull << 18) ? 1u : 2u;
    const dim3 grid((unsigned)(C * nspans)), block(mh::kBinThreads);
    hipStream_t st = (hipStream_t)stream;
    if (bits == 8)
        hipLaunchKernelGGL(mh::k_bin_events<8>, grid, block, 0, st, ticks, ev_off, origin, period, T, nchunks, span, nspans,
                           div_mode, out, out_off, chunk_stride);
    else if (bits == 4)
        hipLaunchKernelGGL(mh::k_bin_events<4>, grid, block, 0, st, ticks, ev_off, origin, period, T, nchunks, span, nspans,
                           div_mode, out, out_off, chunk_stride);
    else
        hipLaunchKernelGGL(mh::k_bin_events<2>, grid, block, 0, st, ticks, ev_off, origin, period, T, nchunks, span, nspans,
                           div_mode, out, out_off, chunk_stride);
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
    const uint64_t groups = (n_list + mh::kCrcWaves - 1) / mh::kCrcWaves;
    const dim3 grid((unsigned)(groups < mh::kCrcMaxGroups ? groups : mh::kCrcMaxGroups)), block(64u * mh::kCrcWaves);
    hipLaunchKernelGGL(mh::k_seg_crc32, grid, block, 0, (hipStream_t)stream, static_cast<const uint32_t *>(payload),
                       payload_words, seg_off, seg_words, n_segments, seg_idx, n_list, crc, expect,
                       reinterpret_cast<unsigned long long *>(bad));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "mhi_seg_crc32: launch failed: %s", hipGetErrorString(e));
    return MH_OK;
}

}  // extern "C"
