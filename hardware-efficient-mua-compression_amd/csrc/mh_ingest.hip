// mh_ingest.hip -- C ABI (include/muahuff_ingest.h) over the binner kernel in mh_ingest.hpp: argument checks and the
// launch.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

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

}  // extern "C"
