// mh_sweep_layout.hpp -- the argument rules, the items and the launch grids of mhq_gram_clips and mhq_xty_clips
// (include/muahuff_sweep.h): the Wiener statistics of every clip, lag difference and range of columns in one pass.  Pure
// C++ (no HIP, no device, no global state), as mh_gram_layout.hpp: mh_sweep.hip checks with gram_clips_check() /
// xty_clips_check(), launches what gram_clips_layout() / xty_clips_layout() return, the kernels of mh_sweep.hpp find
// their work with gram_clips_owner() / xty_clips_owner(), and tests/sweep_check.cpp walks all of it under
// -fsanitize=address,undefined.
//
// The RANGES [first[r], last[r]) are columns of x, ascending and disjoint; they and the CLIPS travel by value in the
// kernel parameters (SweepRanges, SweepClips).  Every range is cut into RUNS counted from its own start, and the runs of
// all ranges are numbered in range order: run_first[r] is the number of range r's first run, run_first[kSweepMaxRanges]
// the total.  An empty range has no run.
//
// mhq_gram_clips.  A run is at most kGramRunCols columns -- the int32 bound of mh_gram_layout.hpp.  A TILE PAIR is one
// (lag difference d, tile (ti, tj)): d = 0 has only the nt (nt + 1) / 2 tiles with tj >= ti, whose owner stores the mirror
// image too, every d > 0 all nt * nt; they are numbered d-major, `dt` of them in all.  An ITEM is one (run, clip, tile
// pair): item = (run * n_clips + clip) * dt + pair, so the items next to each other read the same columns.  The grid is
// capped at kSweepMaxBlocks, a multiple of 8, and walked as mhi_gram's (gram_first_item, then a stride of the grid).
// An item reads the columns [k0, k1) of the tile's a rows and [k0 - d, k1 - d) of its b rows: nothing before
// first[0] - (lags - 1), nothing at or after last[n_ranges - 1].
//
// mhq_xty_clips.  A run is kXtyRun columns, as mhw_xty cuts its own columns: range r's runs are the runs of the mhw_xty
// call on that range alone.  An ITEM is one (run, clip, channel): item = (run * n_clips + clip) * rows + channel; it
// stores its lags * k partial sums at scratch[item * lags * k + l * k + j].  The second kernel has one thread per (range,
// clip, channel, lag, covariate) ELEMENT, which adds that element's runs in run order.
#pragma once
#include <stdint.h>

#include "mh_gram_layout.hpp"
#include "mh_rows.hpp"
#include "mh_wiener_layout.hpp"

namespace mh {

constexpr uint32_t kSweepMaxRanges = 16;
constexpr uint32_t kSweepMaxClips = 64;
constexpr uint32_t kSweepMaxBlocks = 2048;     // the grid of k_gram_clips is capped; the kernel strides
static_assert(kSweepMaxBlocks % kGramXcds == 0, "every XCD takes the same share of the grid");
constexpr uint32_t kSweepXtyMaxBlocks = 4096;  // of k_xty_clips and of k_xty_clips_sum
constexpr uint32_t kSweepDirectClip = 127;     // up to here the clamped bytes are int8 operands as they are
static_assert((uint64_t)kSweepDirectClip * kSweepDirectClip * kGramRunCols < (1ull << 31), "a run of direct products fits int32");

// the ranges and the clips as the kernels get them, by value in the kernel parameters
struct SweepRanges {
    uint64_t first[kSweepMaxRanges];          // a of range r
    uint64_t last[kSweepMaxRanges];           // b of range r
    uint64_t run_first[kSweepMaxRanges + 1];  // the number of range r's first run; [kSweepMaxRanges] is the total
};

struct SweepClips {
    uint8_t q[kSweepMaxClips];
};

// the arguments, device pointers as plain addresses: nothing here reads through them.  `ranges` and `clips` are the
// host arrays.
struct GramClipsArgs {
    uint64_t x, x_row_stride, rows, cols;
    const uint64_t *ranges;
    uint32_t n_ranges;
    const uint32_t *clips;
    uint32_t n_clips, lags;
    uint64_t gram, sums;
};

struct XtyClipsArgs {
    uint64_t x, x_row_stride, rows, cols;
    const uint64_t *ranges;
    uint32_t n_ranges;
    const uint32_t *clips;
    uint32_t n_clips, lags, lead;
    uint64_t y, y_row_stride;
    uint32_t k;
    uint64_t out, scratch, scratch_bytes;
};

struct GramClipsLayout {
    SweepRanges ranges;
    SweepClips clips;
    uint32_t nt;      // tiles along the rows
    uint64_t tiles0;  // tile pairs of d = 0: nt * (nt + 1) / 2
    uint64_t tiles1;  // of every d > 0: nt * nt
    uint64_t dt;      // tile pairs of all lag differences
    uint64_t runs;    // of all ranges
    uint64_t items;   // runs * n_clips * dt
    uint32_t grid;    // workgroups: a multiple of 8, at most kSweepMaxBlocks
};

struct GramClipsItem {
    uint32_t r, n, d, ti, tj;  // the range, the clip's index, the lag difference, the tile
    uint64_t k0, k1;           // the columns [k0, k1) of x
};

struct XtyClipsLayout {
    SweepRanges ranges;
    SweepClips clips;
    uint64_t runs;      // of all ranges
    uint64_t items;     // runs * n_clips * rows
    uint32_t per_item;  // lags * k partial sums
    uint32_t grid;      // of the first kernel; 0: every range is empty, there is no first kernel
    uint64_t elements;  // n_ranges * n_clips * rows * lags * k
    uint32_t sum_grid;  // of the second
};

struct XtyClipsItem {
    uint32_t r, n, c;  // the range, the clip's index, the channel
    uint64_t c0, c1;   // the columns [c0, c1) counted from the range's start
};

// the limits both calls share, the clips and the ranges; `fn` names the call, `room` is where the last range may end
inline int sweep_check(Msg &m, const char *fn, uint64_t rows, uint64_t cols, uint32_t lags, const uint64_t *ranges,
                       uint32_t n_ranges, const uint32_t *clips, uint32_t n_clips, uint64_t room)
{
    if (lags < 1 || lags > kWienerMaxLags) return m.set(MH_ERR_ARG, "%s: lags=%u outside 1..%u", fn, lags, kWienerMaxLags);
    if (int rc = rows_rule(m, fn, rows, kWienerMaxRows)) return rc;
    if (int rc = cols_rule(m, fn, cols)) return rc;
    if (n_ranges < 1 || n_ranges > kSweepMaxRanges)
        return m.set(MH_ERR_ARG, "%s: n_ranges=%u outside 1..%u", fn, n_ranges, kSweepMaxRanges);
    if (n_clips < 1 || n_clips > kSweepMaxClips) return m.set(MH_ERR_ARG, "%s: n_clips=%u outside 1..%u", fn, n_clips, kSweepMaxClips);
    for (uint32_t n = 0; n < n_clips; ++n) {
        if (clips[n] < 1 || clips[n] > 255) return m.set(MH_ERR_ARG, "%s: clip %u is %u, outside 1..255", fn, n, clips[n]);
        if (n && clips[n] <= clips[n - 1])
            return m.set(MH_ERR_ARG, "%s: clip %u is %u, not above the %u in front", fn, n, clips[n], clips[n - 1]);
    }
    uint64_t end = lags - 1;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const uint64_t lo = ranges[2 * r], hi = ranges[2 * r + 1];
        if (hi < lo) return m.set(MH_ERR_ARG, "%s: range %u is [%llu, %llu), reversed", fn, r, (unsigned long long)lo, (unsigned long long)hi);
        if (lo < end)
            return m.set(MH_ERR_ARG, "%s: range %u starts at %llu, before %llu (%s)", fn, r, (unsigned long long)lo, (unsigned long long)end,
                         r ? "the end of the range in front" : "lags - 1");
        if (hi > room)
            return m.set(MH_ERR_ARG, "%s: range %u ends at %llu, past %llu", fn, r, (unsigned long long)hi, (unsigned long long)room);
        end = hi;
    }
    return MH_OK;
}

// the ranges and the clips by value, with the runs of `run` columns numbered in range order -> the number of runs
inline uint64_t sweep_pack(const uint64_t *ranges, uint32_t n_ranges, const uint32_t *clips, uint32_t n_clips, uint32_t run,
                           SweepRanges *R, SweepClips *Q)
{
    uint64_t runs = 0;
    for (uint32_t r = 0; r < kSweepMaxRanges; ++r) {
        R->first[r] = r < n_ranges ? ranges[2 * r] : 0;
        R->last[r] = r < n_ranges ? ranges[2 * r + 1] : 0;
        R->run_first[r] = runs;
        runs += (R->last[r] - R->first[r] + run - 1) / run;
    }
    R->run_first[kSweepMaxRanges] = runs;
    for (uint32_t n = 0; n < kSweepMaxClips; ++n) Q->q[n] = (uint8_t)(n < n_clips ? clips[n] : 255);
    return runs;
}

// the range a run belongs to; run < R.run_first[kSweepMaxRanges]
MH_HD inline uint32_t sweep_run_range(const SweepRanges &R, uint64_t run)
{
    uint32_t r = 0;
    while (run >= R.run_first[r + 1]) ++r;  // at most kSweepMaxRanges - 1 steps: run_first[kSweepMaxRanges] is above run
    return r;
}

// ---- mhq_gram_clips ---------------------------------------------------------------------------------------------------------
// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int gram_clips_check(Msg &m, const GramClipsArgs &a)
{
    if (!a.x || !a.ranges || !a.clips || !a.gram || !a.sums) return m.set(MH_ERR_ARG, "mhq_gram_clips: NULL pointer");
    if (int rc = sweep_check(m, "mhq_gram_clips", a.rows, a.cols, a.lags, a.ranges, a.n_ranges, a.clips, a.n_clips, a.cols)) return rc;
    if (a.gram % 8 || a.sums % 8) return m.set(MH_ERR_ARG, "mhq_gram_clips: gram and sums must be multiples of 8");
    if (a.rows > 1 && a.x_row_stride < a.cols)
        return m.set(MH_ERR_ARG, "mhq_gram_clips: x_row_stride=%llu is below cols=%llu", (unsigned long long)a.x_row_stride,
                     (unsigned long long)a.cols);
    return MH_OK;
}

// the whole layout; the arguments have passed gram_clips_check
inline void gram_clips_layout(const GramClipsArgs &a, GramClipsLayout *L)
{
    L->runs = sweep_pack(a.ranges, a.n_ranges, a.clips, a.n_clips, kGramRunCols, &L->ranges, &L->clips);
    L->nt = (uint32_t)((a.rows + kGramTile - 1) / kGramTile);  // at most 512
    L->tiles0 = (uint64_t)L->nt * (L->nt + 1) / 2;
    L->tiles1 = (uint64_t)L->nt * L->nt;
    L->dt = L->tiles0 + (a.lags - 1) * L->tiles1;          // below 2^23
    L->items = L->runs * a.n_clips * L->dt;                // below 2^25 * 2^6 * 2^23
    const uint64_t blocks = L->items < kSweepMaxBlocks ? L->items : kSweepMaxBlocks;
    L->grid = (uint32_t)((blocks + kGramXcds - 1) / kGramXcds * kGramXcds);  // 0: every range is empty, nothing to launch
}

// item -> its range, clip, lag difference, tile and columns
MH_HD inline GramClipsItem gram_clips_owner(const SweepRanges &R, uint32_t n_clips, uint32_t nt, uint64_t tiles0, uint64_t tiles1,
                                                  uint64_t dt, uint64_t item)
{
    GramClipsItem it;
    const uint64_t rn = item / dt;
    uint64_t t = item - rn * dt;
    const uint64_t run = rn / n_clips;
    it.n = (uint32_t)(rn - run * n_clips);
    if (t < tiles0) {  // row ti of the upper triangle holds nt - ti tiles
        uint32_t ti = 0;
        while (t >= nt - ti) t -= nt - ti, ++ti;
        it.d = 0, it.ti = ti, it.tj = ti + (uint32_t)t;
    } else {
        t -= tiles0;
        const uint64_t d1 = t / tiles1;
        t -= d1 * tiles1;
        it.d = (uint32_t)d1 + 1, it.ti = (uint32_t)(t / nt), it.tj = (uint32_t)(t - (uint64_t)it.ti * nt);
    }
    it.r = sweep_run_range(R, run);
    it.k0 = R.first[it.r] + (run - R.run_first[it.r]) * kGramRunCols;
    it.k1 = R.last[it.r] - it.k0 < kGramRunCols ? R.last[it.r] : it.k0 + kGramRunCols;
    return it;
}

// ---- mhq_xty_clips ----------------------------------------------------------------------------------------------------------
inline int xty_clips_shape_check(Msg &m, const char *fn, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint32_t n_ranges,
                                 uint32_t n_clips)
{
    if (int rc = wiener_shape_check(m, fn, rows, cols, lags, k)) return rc;
    if (n_ranges < 1 || n_ranges > kSweepMaxRanges)
        return m.set(MH_ERR_ARG, "%s: n_ranges=%u outside 1..%u", fn, n_ranges, kSweepMaxRanges);
    if (n_clips < 1 || n_clips > kSweepMaxClips) return m.set(MH_ERR_ARG, "%s: n_clips=%u outside 1..%u", fn, n_clips, kSweepMaxClips);
    return MH_OK;
}

// What mhq_xty_clips_scratch_bytes gives: room for the runs of ANY n_ranges disjoint ranges inside [0, cols).  Range r of
// n_r columns has ceil(n_r / kXtyRun) <= n_r / kXtyRun + 1 runs, and the n_r add up to cols at most.
inline uint64_t xty_clips_scratch_bytes(uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint32_t n_ranges, uint32_t n_clips)
{
    return (cols / kXtyRun + n_ranges) * n_clips * rows * lags * k * 8;  // below (2^25 + 2^4) * 2^6 * 2^16 * 2^5 * 2^3 * 2^3
}

inline int xty_clips_scratch_check(Msg &m, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint32_t n_ranges, uint32_t n_clips,
                                   uint64_t bytes_ptr)
{
    if (int rc = xty_clips_shape_check(m, "mhq_xty_clips_scratch_bytes", rows, cols, lags, k, n_ranges, n_clips)) return rc;
    if (!bytes_ptr) return m.set(MH_ERR_ARG, "mhq_xty_clips_scratch_bytes: NULL pointer");
    return MH_OK;
}

inline int xty_clips_check(Msg &m, const XtyClipsArgs &a)
{
    if (!a.x || !a.ranges || !a.clips || !a.y || !a.out || !a.scratch) return m.set(MH_ERR_ARG, "mhq_xty_clips: NULL pointer");
    if (int rc = k_rule(m, "mhq_xty_clips", a.k, kWienerMaxK)) return rc;
    if (a.lead >= a.cols) return m.set(MH_ERR_ARG, "mhq_xty_clips: lead=%u leaves none of the %llu columns", a.lead, (unsigned long long)a.cols);
    if (int rc = sweep_check(m, "mhq_xty_clips", a.rows, a.cols, a.lags, a.ranges, a.n_ranges, a.clips, a.n_clips, a.cols - a.lead))
        return rc;
    if (a.out % 8 || a.scratch % 8) return m.set(MH_ERR_ARG, "mhq_xty_clips: out and scratch must be multiples of 8");
    if (a.y % 4 || a.y_row_stride % 4) return m.set(MH_ERR_ARG, "mhq_xty_clips: y and y_row_stride must be multiples of 4");
    if (a.rows > 1 && a.x_row_stride < a.cols)
        return m.set(MH_ERR_ARG, "mhq_xty_clips: x_row_stride=%llu is below cols=%llu", (unsigned long long)a.x_row_stride,
                     (unsigned long long)a.cols);
    if (a.k > 1 && a.y_row_stride < 4 * a.cols)
        return m.set(MH_ERR_ARG, "mhq_xty_clips: y_row_stride=%llu is below the %llu bytes of a row", (unsigned long long)a.y_row_stride,
                     (unsigned long long)(4 * a.cols));
    const uint64_t need = xty_clips_scratch_bytes(a.rows, a.cols, a.lags, a.k, a.n_ranges, a.n_clips);
    if (a.scratch_bytes < need)
        return m.set(MH_ERR_ARG, "mhq_xty_clips: scratch_bytes=%llu is below the %llu that mhq_xty_clips_scratch_bytes asks for",
                     (unsigned long long)a.scratch_bytes, (unsigned long long)need);
    return MH_OK;
}

// the whole layout; the arguments have passed xty_clips_check
inline void xty_clips_layout(const XtyClipsArgs &a, XtyClipsLayout *L)
{
    L->runs = sweep_pack(a.ranges, a.n_ranges, a.clips, a.n_clips, kXtyRun, &L->ranges, &L->clips);
    L->items = L->runs * a.n_clips * a.rows;
    L->per_item = a.lags * a.k;
    L->grid = (uint32_t)(L->items < kSweepXtyMaxBlocks ? L->items : kSweepXtyMaxBlocks);
    L->elements = (uint64_t)a.n_ranges * a.n_clips * a.rows * L->per_item;  // below 2^4 * 2^6 * 2^16 * 2^8
    const uint64_t blocks = (L->elements + kXtySumThreads - 1) / kXtySumThreads;
    L->sum_grid = (uint32_t)(blocks < kSweepXtyMaxBlocks ? blocks : kSweepXtyMaxBlocks);
}

// item -> its range, clip, channel and the columns of its run, counted from the range's start as mhw_xty counts them
MH_HD inline XtyClipsItem xty_clips_owner(const SweepRanges &R, uint32_t n_clips, uint32_t rows, uint64_t item)
{
    XtyClipsItem it;
    const uint64_t rn = item / rows;
    it.c = (uint32_t)(item - rn * rows);
    const uint64_t run = rn / n_clips;
    it.n = (uint32_t)(rn - run * n_clips);
    it.r = sweep_run_range(R, run);
    xty_run_cols(run - R.run_first[it.r], R.last[it.r] - R.first[it.r], &it.c0, &it.c1);
    return it;
}

}  // namespace mh
