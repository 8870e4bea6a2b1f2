// kalman_check.cpp -- walks what csrc/mh_kalman_layout.hpp decides for mhk_project and mhk_scan (the argument rules, the tiles,
// the bytes a thread may load, the scratch and the capped grids) as a plain host program: no HIP, no Python, so that it can be
// built with -fsanitize=address,undefined (tests/test_host_kalman.py).  Reads lines from stdin:
//   project x x_row_stride rows cols clip m m0 k v v_row_stride
//   scratch cols k n_ranges bytes_ptr
//   scan v v_row_stride k cols ranges_given n_ranges f b n_gain init out out_row_stride scratch scratch_bytes a0 b0 a1 b1 ..
//         (pointers as plain numbers, 0 = NULL; nothing is read through them but the ranges, which follow as numbers;
//          ranges_given = 0 passes NULL for them)
//     -> "ok", or "error <code> <message>"
//   layout cols k n_ranges a0 b0 a1 b1 ..             (a shape that passes the checks)
//     -> proj_tiles proj_grid scan_tiles scan_grid scratch_bytes
//        after checking what the kernels rely on.  mhk_project: the tiles partition the columns; of the first two and the
//        last tile, at every alignment of a row's first byte, a thread's dwords lie inside the row where dwords_ok
//        says so and the byte path stays inside it otherwise; the grid is under its cap and the stride loop reaches
//        every tile once.  mhk_scan: the tiles partition every range's steps from the range's own start and every step's
//        column lies inside the range; every tile finds its range; every record the three kernels read or write lies
//        inside the scratch these ranges need, which mhk_scan_scratch_bytes covers; the lanes of the carry pass partition
//        a range's tiles; the grid is under its cap and the stride loop reaches every tile once.  What is too large to
//        enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_kalman_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

typedef unsigned long long ull;

static int report(int rc, const mh::Msg &m)
{
    CHECK((rc == MH_OK) == (m.text[0] == 0));
    CHECK(rc == MH_OK || rc == MH_ERR_ARG);
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

static int check_project(const std::vector<ull> &v)
{
    CHECK(v.size() == 10);
    const mh::ProjectArgs a = {v[0], v[1], v[2], v[3], (uint32_t)v[4], v[5], v[6], (uint32_t)v[7], v[8], v[9]};
    mh::Msg m;
    return report(mh::project_check(m, a), m);
}

static int check_scratch(const std::vector<ull> &v)
{
    CHECK(v.size() == 4);
    mh::Msg m;
    return report(mh::scan_scratch_check(m, v[0], (uint32_t)v[1], (uint32_t)v[2], v[3]), m);
}

static int check_scan(const std::vector<ull> &v)
{
    CHECK(v.size() >= 14);
    std::vector<uint64_t> ranges(v.begin() + 14, v.end());
    const uint32_t n_ranges = (uint32_t)v[5];
    // the ranges are read only after n_ranges has passed, so exactly 2 * n_ranges numbers follow where it can pass
    CHECK(n_ranges < 1 || n_ranges > mh::kKalmanMaxRanges || !v[4] || ranges.size() == 2 * (size_t)n_ranges);
    static const uint64_t none[2] = {0, 0};  // a pointer that is not NULL where no range follows
    const mh::ScanArgs a = {v[0], v[1], (uint32_t)v[2], v[3], !v[4] ? nullptr : ranges.empty() ? none : ranges.data(), n_ranges, v[6], v[7], (uint32_t)v[8],
                            v[9], v[10], v[11], v[12], v[13]};
    mh::Msg m;
    return report(mh::scan_check(m, a), m);
}

// the indices [0, n) that `walkers` walkers reach, walker b taking b, b + walkers, ...: all of them once.  Enumerated
// when small; otherwise the arithmetic at both ends: index i belongs to walker i % walkers alone.
static int strided(ull n, ull walkers)
{
    CHECK(walkers >= 1);
    if (n <= (1u << 20)) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (ull b = 0; b < walkers && b < n; ++b)
            for (ull i = b; i < n; i += walkers) CHECK(seen[(size_t)i]++ == 0);
        for (ull i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
    } else {
        const ull ends[2] = {0, n - 4096};
        for (ull e : ends)
            for (ull i = e; i < e + 4096; ++i) {
                const ull b = i % walkers, other = (b + 1) % walkers;
                CHECK(b + (i - b) / walkers * walkers == i);
                CHECK(walkers == 1 || (i + walkers - other) % walkers != 0);
            }
    }
    return 0;
}

// one tile of mhk_project as k_project walks it, the row's first byte `sh` bytes behind a dword boundary
static int walk_project_tile(ull tile, ull cols, uint32_t sh)
{
    const ull row = (1ull << 32) + sh;  // any address with that alignment
    for (uint32_t tid = 0; tid < mh::kProjThreads; ++tid) {
        const ull t = tile * mh::kProjTileCols + (ull)mh::kProjGroup * tid;
        if (t >= cols) continue;
        if (mh::dwords_ok(t, sh, cols)) {
            CHECK(t >= sh);
            const ull a0 = row + t - sh, end = a0 + (sh ? 8 : 4);
            CHECK(a0 % 4 == 0 && a0 >= row && end <= row + cols);       // aligned, inside the row
            CHECK(a0 <= row + t && row + t + 4 <= end);                 // and they hold the 4 columns
        } else {
            for (uint32_t b = 0; b < 4; ++b)
                if (t + b < cols) CHECK(row + t + b < row + cols);
            CHECK(t == 0 || t + 8 > cols);                              // only at a row's two ends
        }
    }
    return 0;
}

static int layout(const std::vector<ull> &v)
{
    CHECK(v.size() >= 3);
    const ull cols = v[0];
    const uint32_t k = (uint32_t)v[1], n_ranges = (uint32_t)v[2];
    CHECK(v.size() == 3 + 2 * (size_t)n_ranges);
    std::vector<uint64_t> ranges(v.begin() + 3, v.end());
    const ull far = 1ull << 62;
    {   // the shape passes, with stand-in pointers far from each other
        const mh::ProjectArgs a = {1ull << 32, cols, 2, cols, 255, 1ull << 50, 1ull << 51, k, far, 8 * cols};
        mh::Msg m;
        CHECK(mh::project_check(m, a) == MH_OK);
    }
    mh::ProjectLayout P;
    mh::project_layout(cols, &P);
    CHECK(P.tiles * mh::kProjTileCols >= cols && (P.tiles - 1) * mh::kProjTileCols < cols);
    CHECK(P.grid >= 1 && P.grid == (P.tiles < mh::kProjMaxBlocks ? P.tiles : mh::kProjMaxBlocks));
    CHECK(mh::kProjTileCols == mh::kProjGroup * mh::kProjThreads);  // thread t owns the tile's columns 4 t .. 4 t + 3: every column one owner
    const ull ts[3] = {0, P.tiles > 1 ? 1ull : 0ull, P.tiles - 1};
    for (ull t : ts)
        for (uint32_t sh = 0; sh < 4; ++sh)
            if (int rc = walk_project_tile(t, cols, sh)) return rc;
    if (int rc = strided(P.tiles, P.grid)) return rc;

    mh::ScanLayout L;
    mh::scan_layout(ranges.data(), n_ranges, k, &L);
    const ull per = mh::scan_per_tile(k);
    {
        const mh::ScanArgs a = {far, 8 * cols, k, cols, ranges.data(), n_ranges, 1ull << 50, 1ull << 51, 7, 1ull << 52, far, 8 * cols,
                                1ull << 40, L.scratch_bytes};
        mh::Msg m;
        CHECK(mh::scan_check(m, a) == MH_OK);
        const mh::ScanArgs small = {far, 8 * cols, k, cols, ranges.data(), n_ranges, 1ull << 50, 1ull << 51, 7, 1ull << 52, far, 8 * cols,
                                    1ull << 40, L.scratch_bytes - 1};
        CHECK(L.scratch_bytes == 0 || mh::scan_check(m, small) == MH_ERR_ARG);
    }
    CHECK(L.scratch_bytes == L.tiles * per * 8 && L.scratch_bytes <= mh::scan_scratch_bytes(cols, k, n_ranges));
    CHECK(L.n_ranges == n_ranges && L.tile_base[0] == 0 && L.tile_base[mh::kKalmanMaxRanges] == L.tiles);
    ull total = 0;
    for (uint32_t r = 0; r < n_ranges; ++r) {
        const ull a = L.a[r], b = L.b[r], steps = mh::scan_range_steps(a, b), n = mh::scan_range_tiles(a, b);
        CHECK(a == ranges[2 * r] && b == ranges[2 * r + 1] && L.tile_base[r] == total);
        CHECK(steps == (b > a ? b - a - 1 : 0) && n * mh::kScanTile >= steps && (n == 0 || (n - 1) * mh::kScanTile < steps));
        // the tiles of the range: consecutive, from step 0 to the last, every column inside (a, b)
        const ull qs[4] = {0, n > 1 ? 1ull : 0ull, n > 1 ? n - 2 : 0ull, n ? n - 1 : 0ull};
        for (ull q : qs) {
            if (!n) break;
            uint64_t i0, i1;
            mh::scan_tile_steps(q, a, b, &i0, &i1);
            CHECK(i0 == q * mh::kScanTile && i1 > i0 && i1 - i0 <= mh::kScanTile && i1 <= steps);
            CHECK(q + 1 < n ? i1 == (q + 1) * mh::kScanTile : i1 == steps);
            CHECK(a + 1 + i0 > a && a + 1 + (i1 - 1) < b && b <= cols);
            const ull tile = total + q;
            CHECK(mh::scan_tile_range(tile, L.tile_base, n_ranges) == r);
            CHECK((tile + 1) * per * 8 <= L.scratch_bytes);             // composite, local end state and carry of the tile
        }
        // the carry pass: lane l owns [l per_lane, (l + 1) per_lane), cut at n
        const ull per_lane = (n + mh::kScanThreads - 1) / mh::kScanThreads;
        ull next = 0;
        for (uint32_t lane = 0; lane < mh::kScanThreads; ++lane) {
            const ull q0 = lane * per_lane < n ? lane * per_lane : n, q1 = q0 + per_lane < n ? q0 + per_lane : n;
            CHECK(q0 == next && q1 >= q0 && q1 <= n);
            next = q1;
        }
        CHECK(next == n);
        total += n;
    }
    CHECK(total == L.tiles);
    const ull blocks = (L.tiles + mh::kScanThreads - 1) / mh::kScanThreads;
    CHECK(L.grid == (blocks < mh::kScanMaxBlocks ? blocks : mh::kScanMaxBlocks) && (L.grid >= 1) == (L.tiles >= 1));
    if (L.tiles)
        if (int rc = strided(L.tiles, (ull)L.grid * mh::kScanThreads)) return rc;
    printf("%llu %u %llu %u %llu\n", (ull)P.tiles, P.grid, (ull)L.tiles, L.grid, (ull)L.scratch_bytes);
    return 0;
}

int main()
{
    static char line[1 << 12];
    while (fgets(line, sizeof(line), stdin)) {
        char *s = line;
        while (*s == ' ') ++s;
        if (*s == '\n' || !*s) continue;
        char *end = s;
        while (*end && *end != ' ' && *end != '\n') ++end;
        const size_t wl = (size_t)(end - s);
        std::vector<ull> v;
        for (char *q = end;;) {
            char *nx;
            const ull x = strtoull(q, &nx, 10);
            if (nx == q) break;
            v.push_back(x);
            q = nx;
        }
        int rc;
        if (wl == 7 && !strncmp(s, "project", 7))
            rc = check_project(v);
        else if (wl == 7 && !strncmp(s, "scratch", 7))
            rc = check_scratch(v);
        else if (wl == 4 && !strncmp(s, "scan", 4))
            rc = check_scan(v);
        else if (wl == 6 && !strncmp(s, "layout", 6))
            rc = layout(v);
        else
            return 3;
        if (rc) return rc;
    }
    return 0;
}
