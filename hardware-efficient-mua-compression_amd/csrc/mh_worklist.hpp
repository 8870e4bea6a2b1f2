// mh_worklist.hpp -- the host-built work lists of mh_decode_range and mh_decode_rebin: the records the kernels of
// mh_range.hpp / mh_rebin_decode.hpp read, and the builders that fill them from the plan's directory.  Pure C++ (no
// HIP, no device), as mh_planner.hpp: muahuff.hip uploads the packed list, tests/planner_check.cpp --worklist builds
// the same lists under -fsanitize=address,undefined and prints them for tests/test_host_worklist.py to execute.
// Every address the range kernels write is fixed here, never by stream contents.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "mh_planner.hpp"

namespace mh {

// One segment that overlaps the range (48 bytes).  Chunk c0 of the segment is the first one holding an in-range
// sample; `ncnk` chunks from c0 on (n samples in all) are decoded, and of those the bytes [lo, hi) are written, at
// out + dst + (sample index from chunk c0's first sample).  dst may be negative: nothing below lo is written.
struct RangeTask {
    int64_t dst;    // bytes from `out` to chunk c0's first sample in its output row
    uint32_t seg;   // directory entry (its seg_off entry is read)
    uint32_t skip;  // chunks in front of c0 (full chunks: header scanned, payload passed over)
    uint32_t ncnk;  // chunks decoded
    uint32_t n;     // samples in those chunks
    uint32_t lo;    // first byte written (< 16384: inside chunk c0)
    uint32_t hi;    // one past the last byte written (> (ncnk - 1) * 16384: inside the last chunk)
    uint32_t scr;   // scratch slot of the task's cut chunks (16 KiB each; unused when lo == 0 and hi == n)
    uint32_t pad_[3];
};

// Up to four consecutive tasks of one output row (one channel), one wave each; tables shared at LDS offset 0.
struct RangeWg {
    uint32_t task0, ntask, ch, pad_;
};

// Zero fill of bytes (mh_decode_range) or elements (mh_decode_rebin) [off, off + n) of `out`: the parts of a row
// outside its channel's window / the bins no task touches.
struct RangeFill {
    uint64_t off, n;
};

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// One segment that overlaps the range (64 bytes).  Sample x of the task = sample x counted from the first sample of
// chunk c0 (RangeTask); it lies in the task's bin (ph + x) / r, and the task's bin j is element dst + j of `out`.
struct RebinTask {
    int64_t dst;      // elements from `out` to the task's bin 0 (may be one bin before the row: nothing below jfirst is written)
    uint32_t seg;     // directory entry
    uint32_t skip;    // chunks in front of c0 (passed over)
    uint32_t n;       // samples decoded (whole chunks from c0 on, or up to the segment's end)
    uint32_t lo, hi;  // samples [lo, hi) of those are in range; the others count as 0
    uint32_t ph;      // position of sample 0 inside its bin (< r)
    uint32_t jfirst, jlast;  // bins of samples lo and hi - 1
    uint32_t head, tail;     // side slot of bin jfirst / jlast when another task touches it too, else kNoSlot
    uint32_t pad_[4];
};

// out[off] = side[slot] (saturated for the u8 form)
struct RebinFix {
    uint64_t off;
    uint32_t slot, pad_;
};

static_assert(sizeof(RangeTask) == 48 && sizeof(RangeWg) == 16 && sizeof(RangeFill) == 16, "the range kernels' records");
static_assert(sizeof(RebinTask) == 64 && sizeof(RebinFix) == 16, "the re-bin kernels' records");

// A work list as the device reads it: blob = tasks | workgroups | fix records | fill records, every section from a
// 16-byte boundary (b_*: the padded section sizes; the range list has no fix records, b_fix = 0).
struct WorkList {
    std::vector<uint8_t> blob;
    size_t b_task = 0, b_wg = 0, b_fix = 0;
    size_t ntask = 0, nwg = 0, nfix = 0, nfill = 0;
    uint32_t naux = 0;      // 16-KiB scratch slots of cut chunks (range) / u32 side words of shared bins (re-bin)
    uint64_t max_fill = 0;  // the longest fill record (sizes the fill launch)
};

// What a row's tasks are cut from: samples [lo, hi) of segment s (directory entry; first window sample sf, sn samples)
// are in range; they lie in its chunks c0 .. c1, and chunk c0 starts at sample `base` of the segment.
struct SegSpan {
    uint64_t s, sf, sn, lo, hi, c0, c1, base;
};

template <class Task>
struct ListParts {
    std::vector<Task> tasks;
    std::vector<RangeWg> wgs;
    std::vector<RebinFix> fixes;
    std::vector<RangeFill> fills;
    uint32_t naux = 0;
};

// The one walk over a query (sel, [t0, t1), r, out_pitch; arguments already checked, r = 1: samples as they are).  Row i
// holds the ceil((t1 - t0) / r) bins of channel sel[i] from element i * out_pitch on.  Per row: fill records for the bins
// in front of and behind the in-window part [a, b) of the range, emit(parts, row, w0, span, task0) for every segment
// that overlaps it (emit appends one task; task0 = the row's first), then the row's tasks four to a workgroup.
template <class Task, class Emit>
inline WorkList walk_query(const PlanHost &H, const uint32_t *sel, uint32_t n_sel, uint64_t t0, uint64_t t1, uint32_t r,
                           uint64_t out_pitch, Emit emit)
{
    ListParts<Task> L;
    WorkList w;
    const uint64_t nb = (t1 - t0 + r - 1) / r;
    auto fill = [&](uint64_t off, uint64_t n) {
        if (n == 0) return;
        L.fills.push_back(RangeFill{off, n});
        if (n > w.max_fill) w.max_fill = n;
    };
    const uint64_t *sf0 = H.seg_first.data();
    for (uint32_t i = 0; i < n_sel; ++i) {
        const uint32_t c = sel[i];
        const uint64_t row = (uint64_t)i * out_pitch, w0 = H.w0[c], w1 = H.w1[c];
        const uint64_t a = t0 > w0 ? t0 : w0, b = t1 < w1 ? t1 : w1;  // in-window part, channel samples
        if (a >= b) {
            fill(row, nb);
            continue;
        }
        fill(row, (a - t0) / r);                                        // bins in front of sample a's
        fill(row + (b - 1 - t0) / r + 1, nb - ((b - 1 - t0) / r + 1));  // bins behind sample (b - 1)'s
        const uint64_t ra = a - w0, rb = b - w0;  // the same, window samples
        const uint64_t end = H.ch_seg0[(size_t)c + 1];
        uint64_t s = (uint64_t)(std::upper_bound(sf0 + H.ch_seg0[c], sf0 + end, ra) - sf0) - 1;
        const size_t task0 = L.tasks.size();
        for (; s < end && H.seg_first[s] < rb; ++s) {
            SegSpan g;
            g.s = s, g.sf = H.seg_first[s], g.sn = H.seg_n[s];
            g.lo = (ra > g.sf ? ra : g.sf) - g.sf, g.hi = (rb < g.sf + g.sn ? rb : g.sf + g.sn) - g.sf;
            g.c0 = g.lo / MH_CHUNK, g.c1 = (g.hi - 1) / MH_CHUNK, g.base = g.c0 * MH_CHUNK;
            emit(L, row, w0, g, task0);
        }
        for (size_t k = task0; k < L.tasks.size(); k += 4)
            L.wgs.push_back(RangeWg{(uint32_t)k, (uint32_t)(L.tasks.size() - k < 4 ? L.tasks.size() - k : 4), c, 0u});
    }
    // ---- pack (one upload)
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    w.b_task = up16(L.tasks.size() * sizeof(Task));
    w.b_wg = up16(L.wgs.size() * sizeof(RangeWg));
    w.b_fix = up16(L.fixes.size() * sizeof(RebinFix));
    w.ntask = L.tasks.size(), w.nwg = L.wgs.size(), w.nfix = L.fixes.size(), w.nfill = L.fills.size();
    w.naux = L.naux;
    w.blob.assign(w.b_task + w.b_wg + w.b_fix + L.fills.size() * sizeof(RangeFill), 0);
    auto put = [&](size_t at, const void *src, size_t n) {
        if (n) memcpy(w.blob.data() + at, src, n);
    };
    put(0, L.tasks.data(), L.tasks.size() * sizeof(Task));
    put(w.b_task, L.wgs.data(), L.wgs.size() * sizeof(RangeWg));
    put(w.b_task + w.b_wg, L.fixes.data(), L.fixes.size() * sizeof(RebinFix));
    put(w.b_task + w.b_wg + w.b_fix, L.fills.data(), L.fills.size() * sizeof(RangeFill));
    return w;
}

// mh_decode_range's list: one RangeTask per overlapping segment, a scratch slot for each task with a cut chunk, byte
// fills outside the window.
inline WorkList range_work_list(const PlanHost &H, const uint32_t *sel, uint32_t n_sel, uint64_t t0, uint64_t t1,
                                uint64_t out_pitch)
{
    return walk_query<RangeTask>(H, sel, n_sel, t0, t1, 1u, out_pitch,
                                 [&](ListParts<RangeTask> &L, uint64_t row, uint64_t w0, const SegSpan &g, size_t) {
        RangeTask t{};
        t.dst = (int64_t)(row + w0 + g.sf + g.base) - (int64_t)t0;
        t.seg = (uint32_t)g.s;
        t.skip = (uint32_t)g.c0;
        t.ncnk = (uint32_t)(g.c1 - g.c0 + 1);
        t.n = (uint32_t)(g.sn - g.base < (uint64_t)t.ncnk * MH_CHUNK ? g.sn - g.base : (uint64_t)t.ncnk * MH_CHUNK);
        t.lo = (uint32_t)(g.lo - g.base);
        t.hi = (uint32_t)(g.hi - g.base);
        t.scr = t.lo > 0 || t.hi < t.n ? L.naux++ : 0u;
        L.tasks.push_back(t);
    });
}

// mh_decode_rebin's list: one RebinTask per overlapping segment, plus what the bins need.  The tasks of a row cover
// consecutive sample spans, so the bins they touch are consecutive too: a bin is shared when a task's first bin is the
// previous task's last one -- those get a side slot and a fix-up record; the bins of a row in front of the first task's
// and behind the last task's are zeroed (walk_query's fills).
inline WorkList rebin_work_list(const PlanHost &H, const uint32_t *sel, uint32_t n_sel, uint64_t t0, uint64_t t1, uint32_t r,
                                uint64_t out_pitch)
{
    uint64_t prev_last = 0;  // the previous task's last bin (of the row)
    return walk_query<RebinTask>(H, sel, n_sel, t0, t1, r, out_pitch,
                                 [&](ListParts<RebinTask> &L, uint64_t row, uint64_t w0, const SegSpan &g, size_t task0) {
        const uint64_t ncnk = g.c1 - g.c0 + 1;
        // sample 0 of the task (chunk c0's first) sits at g0 in the range, possibly in front of it (then in bin -1)
        const int64_t g0 = (int64_t)(w0 + g.sf + g.base) - (int64_t)t0;
        const int64_t b0 = g0 >= 0 ? g0 / (int64_t)r : -(((-g0) + (int64_t)r - 1) / (int64_t)r);
        RebinTask t{};
        t.ph = (uint32_t)(g0 - b0 * (int64_t)r);
        t.dst = (int64_t)row + b0;
        t.seg = (uint32_t)g.s;
        t.skip = (uint32_t)g.c0;
        t.n = (uint32_t)(g.sn - g.base < ncnk * MH_CHUNK ? g.sn - g.base : ncnk * MH_CHUNK);
        t.lo = (uint32_t)(g.lo - g.base);
        t.hi = (uint32_t)(g.hi - g.base);
        t.jfirst = (uint32_t)((t.ph + (uint64_t)t.lo) / r);
        t.jlast = (uint32_t)((t.ph + (uint64_t)t.hi - 1) / r);
        t.head = t.tail = kNoSlot;
        const uint64_t first = (uint64_t)(b0 + (int64_t)t.jfirst), last = (uint64_t)(b0 + (int64_t)t.jlast);
        if (L.tasks.size() > task0 && first == prev_last) {  // shared with the previous task (and maybe the ones before)
            RebinTask &q = L.tasks.back();
            uint32_t slot = q.jfirst == q.jlast && q.head != kNoSlot ? q.head : q.tail;
            if (slot == kNoSlot) {
                slot = L.naux++;
                L.fixes.push_back(RebinFix{row + first, slot, 0u});
            }
            q.tail = slot;
            t.head = slot;
        }
        prev_last = last;
        L.tasks.push_back(t);
    });
}

}  // namespace mh
