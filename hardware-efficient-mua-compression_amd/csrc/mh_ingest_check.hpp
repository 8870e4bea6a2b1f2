// mh_ingest_check.hpp -- the argument rules of the two calls of include/muahuff_ingest.h that have no layout header of
// their own: mhi_bin_events and mhi_seg_crc32.  Pure C++ (no HIP, no device, no global state), as mh_windows_layout.hpp:
// mh_ingest.hip checks with bin_events_check() and bin_events_table_check() / seg_crc_check() and launches what they
// return (the grids are those of mh_launch.hpp), and tests/crc_check.cpp prints their verdicts under
// -fsanitize=address,undefined.
#pragma once
#include <stdint.h>

#include "mh_launch.hpp"
#include "mh_msg.hpp"
#include "muahuff.h"

namespace mh {

// Where a table lives, as the runtime's allocation records say (mh_ingest.hip asks them; nothing here does)
constexpr uint32_t kWhereDevice = 0;    // device memory: the host cannot read it
constexpr uint32_t kWhereBoth = 1;      // pinned or managed: both can
constexpr uint32_t kWhereHostOnly = 2;  // plain host memory: the device cannot read it

// mhi_bin_events' arguments, pointers as plain addresses
struct BinArgs {
    uint64_t ticks, ev_off;
    uint32_t C;
    uint64_t origin, period, T;
    uint32_t bits;
    uint64_t out, out_off, chunk_stride;
};

// The rules that need nothing but the arguments: MH_OK, or MH_ERR_ARG with the text in m.  Nothing is read through a
// pointer.
inline int bin_events_check(Msg &m, const BinArgs &a)
{
    if (!a.ticks || !a.ev_off || !a.out || !a.out_off) return m.set(MH_ERR_ARG, "mhi_bin_events: NULL pointer");
    if (a.C == 0 || a.T == 0 || a.period == 0)
        return m.set(MH_ERR_ARG, "mhi_bin_events: C=%u, T=%llu, period=%llu (each at least 1)", a.C, (unsigned long long)a.T,
                     (unsigned long long)a.period);
    if (a.bits != 8 && a.bits != 4 && a.bits != 2) return m.set(MH_ERR_ARG, "mhi_bin_events: bits=%u (8, 4 or 2)", a.bits);
    if (!chunk_stride_ok(a.chunk_stride, a.bits))
        return m.set(MH_ERR_ARG, "mhi_bin_events: chunk_stride=%llu (packed output only, a multiple of 16, at least one chunk)",
                     (unsigned long long)a.chunk_stride);
    const unsigned __int128 end = (unsigned __int128)a.origin + (unsigned __int128)a.T * a.period;
    if (end > ((unsigned __int128)1 << 63))
        return m.set(MH_ERR_ARG, "mhi_bin_events: origin + T*period exceeds 2^63 (origin=%llu, T=%llu, period=%llu)",
                     (unsigned long long)a.origin, (unsigned long long)a.T, (unsigned long long)a.period);
    return MH_OK;
}

// What follows bin_events_check: the offsets of a packed call (bits != 8) are multiples of 16 -- the ONE place a check
// reads through a pointer, out_off[0 .. C), and only when `where` (kWhere*, looked at only then) says the host can -- the
// device can read the table, and the launch (chunks per workgroup and the grid, mh_launch.hpp).
inline int bin_events_table_check(Msg &m, const BinArgs &a, uint32_t where, BinLaunch *l)
{
    if (a.bits != 8) {
        if (where != kWhereDevice) {
            const uint64_t *const off = reinterpret_cast<const uint64_t *>((uintptr_t)a.out_off);
            for (uint32_t c = 0; c < a.C; ++c)
                if (off[c] % 16)
                    return m.set(MH_ERR_ARG, "mhi_bin_events: out_off[%u]=%llu is not a multiple of 16 (packed output)", c,
                                 (unsigned long long)off[c]);
        }
        if (where == kWhereHostOnly) return m.set(MH_ERR_ARG, "mhi_bin_events: out_off is host memory the device cannot read");
    }
    return bin_events_launch(m, a.C, a.T, a.period, l);
}

// mhi_seg_crc32's arguments, pointers as plain addresses: nothing here reads through them
struct CrcArgs {
    uint64_t payload, payload_words, seg_off, seg_words, n_segments, seg_idx, n_idx, crc, expect, bad;
};

struct CrcLaunch {
    uint64_t n_list;  // the segments to walk: n_idx with a list, else n_segments; 0: nothing to launch
    uint32_t grid;    // seg_crc_grid(n_list) (mh_launch.hpp: capped, the kernel strides); 0 when n_list is
};

inline int seg_crc_check(Msg &m, const CrcArgs &a, CrcLaunch *l)
{
    if (!a.payload || !a.seg_off || !a.seg_words) return m.set(MH_ERR_ARG, "mhi_seg_crc32: NULL pointer");
    if (!a.crc && !a.expect) return m.set(MH_ERR_ARG, "mhi_seg_crc32: neither crc nor expect is given");
    if (a.expect && !a.bad) return m.set(MH_ERR_ARG, "mhi_seg_crc32: expect is given without bad");
    if (a.payload % 4) return m.set(MH_ERR_ARG, "mhi_seg_crc32: payload is not 4-byte aligned");
    l->n_list = a.seg_idx ? a.n_idx : a.n_segments;
    l->grid = l->n_list ? seg_crc_grid(l->n_list) : 0;
    return MH_OK;
}

}  // namespace mh
