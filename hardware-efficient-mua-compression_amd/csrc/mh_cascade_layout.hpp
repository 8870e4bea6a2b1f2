// mh_cascade_layout.hpp -- the argument rules, the runs, the scratch and the launch grids of mhc_moments and mhc_polyval
// (include/muahuff_cascade.h): the power sums of a prediction against its target over ranges of columns, and the
// polynomial second stage of the Wiener cascade.  Pure C++ (no HIP, no device, no global state), as
// mh_wiener_layout.hpp: mh_cascade.hip checks with mom_check() / poly_check(), launches what mom_layout() /
// poly_layout() return, the kernels of mh_cascade.hpp find their work with the same functions, and
// tests/cascade_check.cpp walks all of it under -fsanitize=address,undefined.
//
// mhc_moments.  Every range [a, b) is cut into RUNS of kMomRun columns counted from a, so what a range's runs are does
// not depend on the other ranges of the call; the runs of all ranges are numbered in range order (run_first[r] is the
// number of range r's first run, run_first[n_ranges] the total).  An ITEM is one (run, output): item = run * k + j.  A
// workgroup takes an item at a time and stores its per = 3 * degree + 4 partial sums at scratch[item * per + s].  The
// grid is capped at kMomMaxBlocks; workgroup b starts at item b and strides by the grid.  The second kernel has one
// thread per ELEMENT (range, output, sum), element = (r * k + j) * per + s, which adds that element's runs in run order;
// its grid is capped at kMomSumMaxBlocks and strides too.
//
// mhc_polyval.  The columns are cut into TILES of kPolyTile; an ITEM is one (tile, output): item = tile * k + j.  Thread
// t of a workgroup owns the tile's columns 4t .. 4t + 3.  The grid is capped at kPolyMaxBlocks and strides.
#pragma once
#include <stdint.h>

#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kCascadeMaxK = 8;
constexpr uint32_t kCascadeMaxDegree = 6;

constexpr uint32_t kMomMaxRanges = 16;
constexpr uint32_t kMomThreads = 256;      // 4 waves
constexpr uint32_t kMomRun = 16384;        // columns of a run: 16 groups of 4 per thread
constexpr uint32_t kMomMaxBlocks = 2048;   // the grid is capped; the kernel strides
constexpr uint32_t kMomSumThreads = 64;    // at most 16 * 8 * 22 = 2816 elements: one wave per workgroup
constexpr uint32_t kMomSumMaxBlocks = 32;
constexpr uint32_t kMomMaxPer = 3 * kCascadeMaxDegree + 4;
static_assert(kMomRun % (4 * kMomThreads) == 0, "every thread of a workgroup walks the same number of groups of a full run");

constexpr uint32_t kPolyThreads = 256;
constexpr uint32_t kPolyTile = 4 * kPolyThreads;  // columns of a tile
constexpr uint32_t kPolyMaxBlocks = 2048;

// the arguments, device pointers as plain addresses: nothing here reads through them.  `ranges` is the host array.
struct MomArgs {
    uint64_t p, p_row_stride, y, y_row_stride;
    uint32_t k;
    uint64_t cols;
    const uint64_t *ranges;
    uint32_t n_ranges, degree;
    uint64_t center, inv_scale, out;
    uint32_t accumulate;
    uint64_t scratch, scratch_bytes;
};

struct PolyArgs {
    uint64_t p, p_row_stride;
    uint32_t k;
    uint64_t cols, coef;
    uint32_t degree;
    uint64_t center, inv_scale, out, out_row_stride;
};

// the ranges as the kernels get them, by value in the kernel parameters
struct MomRanges {
    uint64_t first[kMomMaxRanges];          // a of range r
    uint64_t last[kMomMaxRanges];           // b of range r
    uint64_t run_first[kMomMaxRanges + 1];  // the number of range r's first run; [n] is the total
    uint32_t n;
};

struct MomLayout {
    MomRanges ranges;
    uint64_t runs;      // of all ranges
    uint64_t items;     // runs * k
    uint32_t per;       // 3 * degree + 4 sums
    uint64_t used_bytes;  // of the scratch: items * per * 8
    uint32_t grid;      // of the first kernel; 0 when every range is empty (it is not launched then)
    uint32_t elements;  // n_ranges * k * per
    uint32_t sum_grid;  // of the second
};

struct PolyLayout {
    uint64_t tiles;  // ceil(cols / kPolyTile)
    uint64_t items;  // tiles * k
    uint32_t grid;
};

MH_HD inline uint32_t mom_per(uint32_t degree) { return 3 * degree + 4; }

// the limits mhc_moments and its scratch size share; `fn` names the call
inline int mom_shape_check(Msg &m, const char *fn, uint64_t cols, uint32_t k, uint32_t degree, uint32_t n_ranges)
{
    if (int rc = k_rule(m, fn, k, kCascadeMaxK)) return rc;
    if (int rc = cols_rule(m, fn, cols)) return rc;
    if (degree < 1 || degree > kCascadeMaxDegree) return m.set(MH_ERR_ARG, "%s: degree=%u outside 1..%u", fn, degree, kCascadeMaxDegree);
    if (n_ranges < 1 || n_ranges > kMomMaxRanges) return m.set(MH_ERR_ARG, "%s: n_ranges=%u outside 1..%u", fn, n_ranges, kMomMaxRanges);
    return MH_OK;
}

// What mhc_moments_scratch_bytes gives: room for the runs of ANY n_ranges disjoint ranges inside [0, cols).  Range r of
// length n_r has ceil(n_r / kMomRun) <= n_r / kMomRun + 1 runs and the lengths add up to cols at most.
inline uint64_t mom_scratch_bytes(uint64_t cols, uint32_t k, uint32_t degree, uint32_t n_ranges)
{
    return (cols / kMomRun + n_ranges) * k * mom_per(degree) * 8;  // below (2^26 + 2^4) * 2^3 * 22 * 2^3
}

inline int mom_scratch_check(Msg &m, uint64_t cols, uint32_t k, uint32_t degree, uint32_t n_ranges, uint64_t bytes_ptr)
{
    if (int rc = mom_shape_check(m, "mhc_moments_scratch_bytes", cols, k, degree, n_ranges)) return rc;
    if (!bytes_ptr) return m.set(MH_ERR_ARG, "mhc_moments_scratch_bytes: NULL pointer");
    return MH_OK;
}

// the whole layout of mhc_moments; the shape and the ranges have passed mom_check
inline void mom_layout(const uint64_t *ranges, uint32_t n_ranges, uint32_t k, uint32_t degree, MomLayout *L)
{
    MomRanges &R = L->ranges;
    R.n = n_ranges;
    uint64_t runs = 0;
    for (uint32_t r = 0; r < kMomMaxRanges; ++r) {
        R.first[r] = r < n_ranges ? ranges[2 * r] : 0;
        R.last[r] = r < n_ranges ? ranges[2 * r + 1] : 0;
        R.run_first[r] = runs;
        runs += (R.last[r] - R.first[r] + kMomRun - 1) / kMomRun;
    }
    R.run_first[kMomMaxRanges] = runs;
    L->runs = runs;
    L->items = runs * k;
    L->per = mom_per(degree);
    L->used_bytes = L->items * L->per * 8;
    L->grid = (uint32_t)(L->items < kMomMaxBlocks ? L->items : kMomMaxBlocks);
    L->elements = n_ranges * k * L->per;
    const uint32_t blocks = (L->elements + kMomSumThreads - 1) / kMomSumThreads;
    L->sum_grid = blocks < kMomSumMaxBlocks ? blocks : kMomSumMaxBlocks;
}

// the range a run belongs to and its columns [c0, c1); run < R.run_first[kMomMaxRanges]
MH_HD inline uint32_t mom_run_cols(const MomRanges &R, uint64_t run, uint64_t *c0, uint64_t *c1)
{
    uint32_t r = 0;
    while (run >= R.run_first[r + 1]) ++r;  // at most kMomMaxRanges - 1 steps: run_first[kMomMaxRanges] is above run
    *c0 = R.first[r] + (run - R.run_first[r]) * kMomRun;
    *c1 = R.last[r] - *c0 < kMomRun ? R.last[r] : *c0 + kMomRun;
    return r;
}

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int mom_check(Msg &m, const MomArgs &a)
{
    if (!a.p || !a.y || !a.out || !a.scratch || !a.ranges) return m.set(MH_ERR_ARG, "mhc_moments: NULL pointer");
    if (int rc = mom_shape_check(m, "mhc_moments", a.cols, a.k, a.degree, a.n_ranges)) return rc;
    if (a.accumulate > 1) return m.set(MH_ERR_ARG, "mhc_moments: accumulate=%u (0 or 1)", a.accumulate);
    uint64_t end = 0;
    for (uint32_t r = 0; r < a.n_ranges; ++r) {
        const uint64_t lo = a.ranges[2 * r], hi = a.ranges[2 * r + 1];
        if (lo > hi || hi > a.cols || lo < end)
            return m.set(MH_ERR_ARG, "mhc_moments: range %u = [%llu, %llu) is reversed, before the end %llu of the one in front, or past cols=%llu",
                         r, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)end, (unsigned long long)a.cols);
        end = hi;
    }
    if (a.p % 4 || a.p_row_stride % 4 || a.y % 4 || a.y_row_stride % 4)
        return m.set(MH_ERR_ARG, "mhc_moments: p, y and their row strides must be multiples of 4");
    if (a.out % 8 || a.scratch % 8 || a.center % 8 || a.inv_scale % 8)
        return m.set(MH_ERR_ARG, "mhc_moments: out, scratch, center and inv_scale must be multiples of 8");
    if (a.k > 1 && (a.p_row_stride < 4 * a.cols || a.y_row_stride < 4 * a.cols))
        return m.set(MH_ERR_ARG, "mhc_moments: p_row_stride=%llu or y_row_stride=%llu is below the %llu bytes of a row",
                     (unsigned long long)a.p_row_stride, (unsigned long long)a.y_row_stride, (unsigned long long)(4 * a.cols));
    const uint64_t need = mom_scratch_bytes(a.cols, a.k, a.degree, a.n_ranges);
    if (a.scratch_bytes < need)
        return m.set(MH_ERR_ARG, "mhc_moments: scratch_bytes=%llu is below the %llu that mhc_moments_scratch_bytes asks for",
                     (unsigned long long)a.scratch_bytes, (unsigned long long)need);
    return MH_OK;
}

// the whole layout of mhc_polyval; the shape has passed poly_check
inline void poly_layout(uint64_t cols, uint32_t k, PolyLayout *L)
{
    L->tiles = (cols + kPolyTile - 1) / kPolyTile;
    L->items = L->tiles * k;  // below 2^30 * 2^3
    L->grid = (uint32_t)(L->items < kPolyMaxBlocks ? L->items : kPolyMaxBlocks);
}

inline int poly_check(Msg &m, const PolyArgs &a)
{
    if (!a.p || !a.coef || !a.out) return m.set(MH_ERR_ARG, "mhc_polyval: NULL pointer");
    if (int rc = k_rule(m, "mhc_polyval", a.k, kCascadeMaxK)) return rc;
    if (int rc = cols_rule(m, "mhc_polyval", a.cols)) return rc;
    if (a.degree < 1 || a.degree > kCascadeMaxDegree)
        return m.set(MH_ERR_ARG, "mhc_polyval: degree=%u outside 1..%u", a.degree, kCascadeMaxDegree);
    if (a.p % 4 || a.p_row_stride % 4 || a.out % 4 || a.out_row_stride % 4)
        return m.set(MH_ERR_ARG, "mhc_polyval: p, out and their row strides must be multiples of 4");
    if (a.coef % 4 || a.center % 4 || a.inv_scale % 4) return m.set(MH_ERR_ARG, "mhc_polyval: coef, center and inv_scale must be multiples of 4");
    if (a.k > 1 && (a.p_row_stride < 4 * a.cols || a.out_row_stride < 4 * a.cols))
        return m.set(MH_ERR_ARG, "mhc_polyval: p_row_stride=%llu or out_row_stride=%llu is below the %llu bytes of a row",
                     (unsigned long long)a.p_row_stride, (unsigned long long)a.out_row_stride, (unsigned long long)(4 * a.cols));
    // in place (the same rows) is the one overlap of p and out that is allowed; the strides are below 2^60 here or the
    // sums below wrap, which only refuses more
    const uint64_t row = 4 * a.cols;
    const uint64_t p_end = strided_end(a.p, a.k, a.p_row_stride, row);
    const uint64_t o_end = strided_end(a.out, a.k, a.out_row_stride, row);
    const bool in_place = a.p == a.out && (a.k == 1 || a.p_row_stride == a.out_row_stride);
    if (!in_place && ranges_overlap(a.p, p_end, a.out, o_end))
        return m.set(MH_ERR_ARG, "mhc_polyval: out overlaps p without being p itself with the same row stride");
    const uint64_t c_end = a.coef + 4ull * a.k * (a.degree + 1);
    if (ranges_overlap(a.coef, c_end, a.out, o_end)) return m.set(MH_ERR_ARG, "mhc_polyval: out overlaps coef");
    return MH_OK;
}

}  // namespace mh
