// mh_plan_arena.hpp -- what a plan (and a sweep handle) owns on the device, and where: ONE byte range per handle, laid
// out here on the host.  Pure C++ (no HIP, no device): muahuff.hip makes one allocation of tables_bytes +
// scratch_bytes, uploads `tables` to its front in one copy, zeroes the scratch part behind it and points its typed
// views at the regions' offsets; tests/planner_check.cpp --arena compiles the same header under the sanitizers.
//
// The tables part holds what the kernels only read (the planner's vectors and what is derived from them here: the
// 16-byte SCLV rows, the calibration tiles of a packed plan); the scratch part what they write.  Every region starts on
// a multiple of kArenaAlign bytes -- what an allocation of its own would give it, and what the 16-byte row loads, the
// 32-byte task records and the 64-bit atomics of the kernels rely on.  A region of zero elements still has an address
// of its own; an ABSENT region has none: its device pointer stays null, which is how some argument structs are told
// that the feature is off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <memory>
#include <vector>

#include "mh_planner.hpp"
#include "mh_sweep_planner.hpp"

namespace mh {

constexpr size_t kArenaAlign = 256;
// Scratch sizes the kernels fix (mh_device.hpp: kHistStride, kLut; mh_kernels.hpp: kScanBlock), which this header
// cannot include: muahuff.hip static_asserts that they agree.
constexpr size_t kArenaHistSlots = 16;    // 64-bit counters per histogram
constexpr size_t kArenaLutEntries = 16;   // 8-byte entries per channel's symbol table
constexpr size_t kArenaScanBlock = 2048;  // segments per block sum of mh_compact's scan

struct Region {
    size_t off = 0, bytes = 0;  // from the arena's first byte
    bool present = false;
};

struct Arena {
    struct Named {
        const char *name;
        bool scratch;
        Region r;
        const void *src;  // a table's elements until stage() has copied them
    };
    std::unique_ptr<uint8_t[]> tables;  // host staging of the tables part (stage())
    size_t tables_bytes = 0;            // a multiple of kArenaAlign
    size_t scratch_bytes = 0;           // the scratch part follows the tables part
    std::vector<Named> regions;         // every region in layout order, absent ones included

    size_t bytes() const { return tables_bytes + scratch_bytes; }

    static size_t padded(size_t n) { return ((n ? n : 1) + kArenaAlign - 1) / kArenaAlign * kArenaAlign; }

    // Lays a table out; `v` has to live until stage().  (All tables before the first scratch region.)
    template <class T>
    Region table(const char *name, const std::vector<T> &v)
    {
        const Region r{tables_bytes, v.size() * sizeof(T), true};
        tables_bytes += padded(r.bytes);
        regions.push_back({name, false, r, v.data()});
        return r;
    }
    Region scratch(const char *name, size_t n_bytes)
    {
        const Region r{bytes(), n_bytes, true};
        scratch_bytes += padded(n_bytes);
        regions.push_back({name, true, r, nullptr});
        return r;
    }
    Region absent(const char *name, bool is_scratch)
    {
        regions.push_back({name, is_scratch, Region{}, nullptr});
        return Region{};
    }
    // The staging blob, once every table is laid out: one allocation, every table copied once, the gaps zero.
    void stage()
    {
        tables.reset(new uint8_t[tables_bytes]);
        for (Named &g : regions) {
            if (g.scratch || !g.r.present) continue;
            if (g.r.bytes) memcpy(tables.get() + g.r.off, g.src, g.r.bytes);
            memset(tables.get() + g.r.off + g.r.bytes, 0, padded(g.r.bytes) - g.r.bytes);
            g.src = nullptr;
        }
    }
};

struct PlanArena : Arena {
    Region sclv16, tile_cnt, ch_off, ch_len, w0, w1, skip, sclv, codes, seg_ch, seg_first, seg_n, seg_off, tile_ch, tile_n,
        tile_start, wg_tasks, wave_tasks, cal_tile_ch, cal_tile_n, cal_tile_start;  // tables
    Region tile_done, hist, peak, enc, lut, scan, err, acc, calhist;                // scratch
    size_t n_cal_tiles = 0;  // records in cal_tile_*
};

// The K SCLV rows padded to 16 bytes: one vector load per lane in the in-wave calibration.
inline std::vector<uint32_t> sclv_rows16(const PlanHost &H)
{
    std::vector<uint32_t> rows16((size_t)H.info.K * 4, 0u);
    for (uint32_t k = 0; k < H.info.K; ++k)
        for (uint32_t r = 0; r < H.info.S; ++r)
            rows16[(size_t)k * 4 + (r >> 2)] |= (uint32_t)H.sclv[(size_t)k * H.info.S + r] << (8 * (r & 3));
    return rows16;
}

inline PlanArena plan_arena(const PlanHost &H)
{
    const size_t C = H.info.C;
    PlanArena a;
    const std::vector<uint32_t> rows16 = sclv_rows16(H);
    std::vector<uint32_t> tch, tn;  // calibration tiles built here
    std::vector<uint64_t> tstart;
    a.sclv16 = a.table("sclv16", rows16);
    a.tile_cnt = a.table("tile_cnt", H.tile_cnt);
    a.ch_off = a.table("ch_off", H.ch_off);
    a.ch_len = a.table("ch_len", H.ch_len);
    a.w0 = a.table("w0", H.w0);
    a.w1 = a.table("w1", H.w1);
    a.skip = a.table("skip", H.skip);
    a.sclv = a.table("sclv", H.sclv);
    a.codes = a.table("codes", H.codes);
    a.seg_ch = a.table("seg_ch", H.seg_ch);
    a.seg_first = a.table("seg_first", H.seg_first);
    a.seg_n = a.table("seg_n", H.seg_n);
    a.seg_off = a.table("seg_off", H.seg_off);
    a.tile_ch = a.table("tile_ch", H.tile_ch);
    a.tile_n = a.table("tile_n", H.tile_n);
    a.tile_start = a.table("tile_start", H.tile_start);
    a.wg_tasks = a.table("wg_tasks", H.wg_tasks);
    a.wave_tasks = H.use_wave_tasks ? a.table("wave_tasks", H.wave_tasks) : a.absent("wave_tasks", false);
    // Calibration tiles: the planner's, for windows above kCalDirect samples.  mh_measure on packed pieces histograms
    // EVERY calibration window with the tiled kernel, so a packed plan without planner tiles gets one tile per channel
    // here (the planner's lists stay what byte plans use).
    bool cal = !H.cal_tile_ch.empty();
    if (cal) {
        a.cal_tile_ch = a.table("cal_tile_ch", H.cal_tile_ch);
        a.cal_tile_n = a.table("cal_tile_n", H.cal_tile_n);
        a.cal_tile_start = a.table("cal_tile_start", H.cal_tile_start);
        a.n_cal_tiles = H.cal_tile_ch.size();
    } else if (H.input_bits != 8) {
        tch.resize(C), tn.resize(C), tstart.assign(C, 0);
        const uint64_t lim = (uint64_t)1 << H.info.h;
        for (uint32_t c = 0; c < C; ++c) {
            tch[c] = c;
            tn[c] = (uint32_t)(H.ch_len[c] < lim ? H.ch_len[c] : lim);
        }
        a.cal_tile_ch = a.table("cal_tile_ch", tch);
        a.cal_tile_n = a.table("cal_tile_n", tn);
        a.cal_tile_start = a.table("cal_tile_start", tstart);
        a.n_cal_tiles = C;
        cal = true;
    } else {
        for (const char *name : {"cal_tile_ch", "cal_tile_n", "cal_tile_start"}) a.absent(name, false);
    }
    a.stage();
    a.tile_done = a.scratch("tile_done", C * sizeof(uint32_t));  // fused measure: arrival tickets (zero between calls)
    a.hist = a.scratch("hist", C * kArenaHistSlots * sizeof(uint64_t));  // (zero between calls)
    a.peak = a.scratch("peak", C);
    a.enc = a.scratch("enc", C);
    a.lut = a.scratch("lut", C * kArenaLutEntries * 8);
    a.scan = a.scratch("scan", (H.seg_ch.size() / kArenaScanBlock + 2) * sizeof(uint64_t));
    a.err = a.scratch("err", sizeof(uint32_t));  // decode status word
    // wave-task encoder: per-channel {bits << 24 | finished records} (zero between launches)
    a.acc = H.use_wave_tasks ? a.scratch("acc", C * sizeof(uint64_t)) : a.absent("acc", true);
    a.calhist = cal ? a.scratch("calhist", C * kArenaHistSlots * sizeof(uint64_t)) : a.absent("calhist", true);
    return a;
}

// mh_sweep (mh_sweep_planner.hpp): the tiles of every (channel, interval) slot and one histogram per slot
struct SweepArena : Arena {
    Region ch_off, tile_ch, tile_n, tile_slot, tile_start, slot_len;  // tables
    Region hist;                                                      // scratch
};

inline SweepArena sweep_arena(const SweepHost &w)
{
    SweepArena a;
    a.ch_off = a.table("ch_off", w.ch_off);
    a.tile_ch = a.table("tile_ch", w.tile_ch);
    a.tile_n = a.table("tile_n", w.tile_n);
    a.tile_slot = a.table("tile_slot", w.tile_slot);
    a.tile_start = a.table("tile_start", w.tile_start);
    a.slot_len = a.table("slot_len", w.slot_len);
    a.stage();
    a.hist = a.scratch("hist", w.slot_len.size() * kArenaHistSlots * sizeof(uint64_t));
    return a;
}

}  // namespace mh
