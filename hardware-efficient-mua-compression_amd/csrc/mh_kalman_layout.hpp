// mh_kalman_layout.hpp -- the argument rules, the tiles, the scratch and the launch grids of mhk_project and mhk_scan
// (include/muahuff_kalman.h): the constant projection of clipped counts onto the k state directions of a Kalman filter and
// the scan of its affine recurrence over ranges of columns.  Pure C++ (no HIP, no device, no global state), as
// mh_wiener_layout.hpp: mh_kalman.hip checks with project_check() / scan_check(), launches what project_layout() /
// scan_layout() return, the kernels of mh_kalman.hpp find their work with the same functions, and tests/kalman_check.cpp
// walks all of it under -fsanitize=address,undefined.
//
// mhk_project.  The columns are cut into TILES of kProjTileCols = 4 * kProjThreads; thread t of a workgroup owns the 4
// columns from 4 t on of its tile and walks the channels.  The 4 bytes of a channel come from the aligned dwords that hold
// them where both lie inside the row (dwords_ok of mh_rows.hpp), byte by byte otherwise: nothing outside a row's cols bytes is read.
// The grid is capped at kProjMaxBlocks; workgroup b starts at tile b and strides by the grid.
//
// mhk_scan.  A range [a, b) has b - a - 1 STEPS, step i at column a + 1 + i with gain min(i, n_gain - 1).  The steps are cut
// into TILES of kScanTile counted from the range's own start; the tiles of all ranges are numbered through, range r's from
// ScanLayout::tile_base[r] on.  Scratch holds kScanPerTile(k) = k * (k + 2) doubles per tile: the composite map
// (k x k, row major), the local end state (k) and the carry (k: the state in front of the tile's first step).  Kernel 1 and
// kernel 3 give a thread a tile; their grids are capped at kScanMaxBlocks workgroups of kScanThreads and stride.  Kernel 2
// has one wave per range: lane l owns the tiles [l * per, (l + 1) * per) of the range, per = ceil(tiles / 64).
#pragma once
#include <stdint.h>

#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kKalmanMaxK = 8;
constexpr uint64_t kKalmanMaxRows = 65536;
constexpr uint32_t kKalmanMaxGains = 4096;
constexpr uint32_t kKalmanMaxRanges = 16;

constexpr uint32_t kProjThreads = 256;              // 4 waves
constexpr uint32_t kProjGroup = 4;                  // columns a thread owns: one dword of every channel
constexpr uint32_t kProjTileCols = kProjGroup * kProjThreads;
constexpr uint32_t kProjMaxBlocks = 4096;           // the grid is capped; the kernel strides
constexpr uint32_t kProjUnroll = 8;                 // channels whose loads are issued before the first is used

constexpr uint32_t kScanThreads = 64;               // one wave: a thread owns a tile
constexpr uint32_t kScanTile = 512;                 // steps of a tile
constexpr uint32_t kScanMaxBlocks = 512;            // the grids of kernels 1 and 3 are capped; they stride

MH_HD inline uint32_t scan_per_tile(uint32_t k) { return k * (k + 2); }

// the arguments, pointers as plain addresses: nothing here reads through them
struct ProjectArgs {
    uint64_t x, x_row_stride, rows, cols;
    uint32_t clip;
    uint64_t m, m0;
    uint32_t k;
    uint64_t v, v_row_stride;
};

struct ScanArgs {
    uint64_t v, v_row_stride;
    uint32_t k;
    uint64_t cols;
    const uint64_t *ranges;  // host, 2 * n_ranges: the one pointer that is read, after the NULL and the count checks
    uint32_t n_ranges;
    uint64_t f, b;
    uint32_t n_gain;
    uint64_t init, out, out_row_stride, scratch, scratch_bytes;
};

struct ProjectLayout {
    uint64_t tiles;  // ceil(cols / kProjTileCols)
    uint32_t grid;
};

struct ScanLayout {
    uint64_t a[kKalmanMaxRanges], b[kKalmanMaxRanges];
    uint64_t tile_base[kKalmanMaxRanges + 1];  // the first tile of a range; [n_ranges] is the number of tiles
    uint32_t n_ranges;
    uint64_t tiles;                            // of all ranges
    uint64_t scratch_bytes;                    // what THESE ranges need: at most scan_scratch_bytes(cols, k, n_ranges)
    uint32_t grid;                             // of kernels 1 and 3; 0: no tile, they are not launched
};

// ---- mhk_project ------------------------------------------------------------------------------------------------------------
inline void project_layout(uint64_t cols, ProjectLayout *L)
{
    L->tiles = (cols + kProjTileCols - 1) / kProjTileCols;  // below 2^30
    L->grid = (uint32_t)(L->tiles < kProjMaxBlocks ? L->tiles : kProjMaxBlocks);
}

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int project_check(Msg &m, const ProjectArgs &a)
{
    if (!a.x || !a.m || !a.v) return m.set(MH_ERR_ARG, "mhk_project: NULL pointer");
    if (int rc = k_rule(m, "mhk_project", a.k, kKalmanMaxK)) return rc;
    if (int rc = rows_rule(m, "mhk_project", a.rows, kKalmanMaxRows)) return rc;
    if (int rc = cols_rule(m, "mhk_project", a.cols)) return rc;
    if (int rc = clip_rule(m, "mhk_project", a.clip)) return rc;
    if (a.m % 8 || a.m0 % 8 || a.v % 8 || a.v_row_stride % 8)
        return m.set(MH_ERR_ARG, "mhk_project: m, m0, v and v_row_stride must be multiples of 8");
    if (a.rows > 1 && (a.x_row_stride < a.cols || a.x_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhk_project: x_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.x_row_stride, (unsigned long long)a.cols);
    if (a.k > 1 && (a.v_row_stride < 8 * a.cols || a.v_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhk_project: v_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.v_row_stride, (unsigned long long)(8 * a.cols));
    const uint64_t x_end = strided_end(a.x, a.rows, a.x_row_stride, a.cols);
    const uint64_t v_end = strided_end(a.v, a.k, a.v_row_stride, 8 * a.cols);
    if (ranges_overlap(a.v, v_end, a.x, x_end) || ranges_overlap(a.v, v_end, a.m, a.m + 8 * a.k * a.rows) ||
        (a.m0 && ranges_overlap(a.v, v_end, a.m0, a.m0 + 8ull * a.k)))
        return m.set(MH_ERR_ARG, "mhk_project: v overlaps x, m or m0");
    return MH_OK;
}

// ---- mhk_scan ---------------------------------------------------------------------------------------------------------------
MH_HD inline uint64_t scan_range_steps(uint64_t a, uint64_t b) { return b - a > 1 ? b - a - 1 : 0; }
MH_HD inline uint64_t scan_range_tiles(uint64_t a, uint64_t b) { return (scan_range_steps(a, b) + kScanTile - 1) / kScanTile; }

// the steps [i0, i1) of tile q of a range: step i is column a + 1 + i
MH_HD inline void scan_tile_steps(uint64_t q, uint64_t a, uint64_t b, uint64_t *i0, uint64_t *i1)
{
    const uint64_t n = scan_range_steps(a, b);
    *i0 = q * kScanTile;
    *i1 = n - *i0 < kScanTile ? n : *i0 + kScanTile;
}

// what any n_ranges ranges inside cols columns need at most: every range may end in a ragged tile
inline uint64_t scan_scratch_bytes(uint64_t cols, uint32_t k, uint32_t n_ranges)
{
    return (cols / kScanTile + n_ranges) * scan_per_tile(k) * 8;  // below 2^32 * 80 * 8
}

inline int scan_shape_check(Msg &m, const char *fn, uint64_t cols, uint32_t k, uint32_t n_ranges)
{
    if (int rc = k_rule(m, fn, k, kKalmanMaxK)) return rc;
    if (int rc = cols_rule(m, fn, cols)) return rc;
    if (n_ranges < 1 || n_ranges > kKalmanMaxRanges) return m.set(MH_ERR_ARG, "%s: n_ranges=%u outside 1..%u", fn, n_ranges, kKalmanMaxRanges);
    return MH_OK;
}

inline int scan_scratch_check(Msg &m, uint64_t cols, uint32_t k, uint32_t n_ranges, uint64_t bytes_ptr)
{
    if (int rc = scan_shape_check(m, "mhk_scan_scratch_bytes", cols, k, n_ranges)) return rc;
    if (!bytes_ptr) return m.set(MH_ERR_ARG, "mhk_scan_scratch_bytes: NULL pointer");
    return MH_OK;
}

// the whole layout of mhk_scan; the ranges have passed scan_check
inline void scan_layout(const uint64_t *ranges, uint32_t n_ranges, uint32_t k, ScanLayout *L)
{
    L->n_ranges = n_ranges;
    uint64_t t = 0;
    for (uint32_t r = 0; r < kKalmanMaxRanges; ++r) {
        L->a[r] = r < n_ranges ? ranges[2 * r] : 0;
        L->b[r] = r < n_ranges ? ranges[2 * r + 1] : 0;
        L->tile_base[r] = t;
        if (r < n_ranges) t += scan_range_tiles(L->a[r], L->b[r]);
    }
    L->tile_base[kKalmanMaxRanges] = t;
    L->tiles = t;
    L->scratch_bytes = t * scan_per_tile(k) * 8;
    const uint64_t blocks = (t + kScanThreads - 1) / kScanThreads;
    L->grid = (uint32_t)(blocks < kScanMaxBlocks ? blocks : kScanMaxBlocks);
}

// the range of a tile: the last one whose first tile is not behind it and that has tiles
MH_HD inline uint32_t scan_tile_range(uint64_t tile, const uint64_t *tile_base, uint32_t n_ranges)
{
    uint32_t r = 0;
    for (uint32_t i = 1; i < n_ranges; ++i)
        if (tile_base[i] <= tile) r = i;
    return r;
}

inline int scan_check(Msg &m, const ScanArgs &a)
{
    if (!a.v || !a.f || !a.b || !a.init || !a.out || !a.scratch || !a.ranges) return m.set(MH_ERR_ARG, "mhk_scan: NULL pointer");
    if (int rc = scan_shape_check(m, "mhk_scan", a.cols, a.k, a.n_ranges)) return rc;
    if (a.n_gain < 1 || a.n_gain > kKalmanMaxGains) return m.set(MH_ERR_ARG, "mhk_scan: n_gain=%u outside 1..%u", a.n_gain, kKalmanMaxGains);
    if (a.v % 8 || a.v_row_stride % 8 || a.out % 8 || a.out_row_stride % 8)
        return m.set(MH_ERR_ARG, "mhk_scan: v, out and their row strides must be multiples of 8");
    if (a.f % 8 || a.b % 8 || a.init % 8 || a.scratch % 8) return m.set(MH_ERR_ARG, "mhk_scan: F, B, init and scratch must be multiples of 8");
    const uint64_t row = 8 * a.cols;
    if (a.k > 1 && (a.v_row_stride < row || a.out_row_stride < row || a.v_row_stride >= kMaxStride || a.out_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "mhk_scan: v_row_stride=%llu or out_row_stride=%llu is below the %llu bytes of a row, or not below 2^48",
                     (unsigned long long)a.v_row_stride, (unsigned long long)a.out_row_stride, (unsigned long long)row);
    uint64_t prev = 0;
    for (uint32_t r = 0; r < a.n_ranges; ++r) {
        const uint64_t lo = a.ranges[2 * r], hi = a.ranges[2 * r + 1];
        if (lo > hi || lo < prev || hi > a.cols)
            return m.set(MH_ERR_ARG, "mhk_scan: range %u = [%llu, %llu) is reversed, starts before the one in front ends (%llu) or ends past cols=%llu",
                         r, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)prev, (unsigned long long)a.cols);
        prev = hi;
    }
    const uint64_t v_end = strided_end(a.v, a.k, a.v_row_stride, row);
    const uint64_t out_end = strided_end(a.out, a.k, a.out_row_stride, row);
    const bool same = a.out == a.v && (a.k == 1 || a.out_row_stride == a.v_row_stride);
    if (!same && ranges_overlap(a.out, out_end, a.v, v_end))
        return m.set(MH_ERR_ARG, "mhk_scan: out overlaps v without being v with the same row stride");
    ScanLayout L;
    scan_layout(a.ranges, a.n_ranges, a.k, &L);
    if (a.scratch_bytes < L.scratch_bytes)
        return m.set(MH_ERR_ARG, "mhk_scan: scratch_bytes=%llu is below the %llu these ranges need (mhk_scan_scratch_bytes gives enough for any)",
                     (unsigned long long)a.scratch_bytes, (unsigned long long)L.scratch_bytes);
    const uint64_t kk = 8ull * a.k * a.k * a.n_gain;
    if (ranges_overlap(a.out, out_end, a.scratch, a.scratch + L.scratch_bytes) || ranges_overlap(a.v, v_end, a.scratch, a.scratch + L.scratch_bytes) ||
        ranges_overlap(a.out, out_end, a.f, a.f + kk) || ranges_overlap(a.out, out_end, a.b, a.b + kk) ||
        ranges_overlap(a.out, out_end, a.init, a.init + 8ull * a.k * a.n_ranges))
        return m.set(MH_ERR_ARG, "mhk_scan: scratch overlaps v or out, or out overlaps F, B or init");
    return MH_OK;
}

}  // namespace mh
