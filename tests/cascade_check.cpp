// cascade_check.cpp -- walks what csrc/mh_cascade_layout.hpp decides for mhc_moments and mhc_polyval (the argument rules,
// the runs of every range, the scratch, the tiles and the capped grids) as a plain host program: no HIP, no Python, so
// that it can be built with -fsanitize=address,undefined (tests/test_host_cascade.py).  Reads lines from stdin:
//   mom p p_row_stride y y_row_stride k cols ranges n_ranges degree center inv_scale out accumulate scratch scratch_bytes a0 b0 a1 b1 ...
//         (`ranges` 0 = NULL, anything else = the numbers that end the line)
//   poly p p_row_stride k cols coef degree center inv_scale out out_row_stride
//   scratch cols k degree n_ranges bytes_pointer
//         (pointers as plain numbers, 0 = NULL; nothing is read through them)
//     -> "ok", or "error <code> <message>"
//   layout cols k degree n_ranges a0 b0 a1 b1 ...        (a shape and ranges that pass the check)
//     -> runs items per used_bytes grid elements sum_grid scratch_bytes tiles poly_items poly_grid
//        after checking what the kernels rely on: every range's runs partition it and are counted from its own start; the
//        scratch mhc_moments_scratch_bytes asks for covers every item's partial sums and the sum kernel's reads; the
//        tiles partition the columns; the grids are under their caps and the stride loops reach every item and element
//        once.  What is too large to enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_cascade_layout.hpp"

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

static int check_mom(const std::vector<ull> &v)
{
    CHECK(v.size() >= 15);
    // exactly the numbers that were given: a rule that reads past 2 * n_ranges of them is the sanitizer's to find
    std::vector<uint64_t> ranges(v.begin() + 15, v.end());
    ranges.reserve(1);  // no number given and `ranges` not 0: a pointer to nothing, not NULL
    const uint32_t n_ranges = (uint32_t)v[7];
    CHECK(!v[6] || n_ranges > mh::kMomMaxRanges || ranges.size() == 2 * (size_t)n_ranges);
    const mh::MomArgs a = {v[0], v[1], v[2], v[3], (uint32_t)v[4], v[5], v[6] ? ranges.data() : nullptr, n_ranges, (uint32_t)v[8], v[9], v[10],
                           v[11], (uint32_t)v[12], v[13], v[14]};
    mh::Msg m;
    return report(mh::mom_check(m, a), m);
}

static int check_poly(const std::vector<ull> &v)
{
    CHECK(v.size() == 10);
    const mh::PolyArgs a = {v[0], v[1], (uint32_t)v[2], v[3], v[4], (uint32_t)v[5], v[6], v[7], v[8], v[9]};
    mh::Msg m;
    return report(mh::poly_check(m, a), m);
}

static int check_scratch(const std::vector<ull> &v)
{
    CHECK(v.size() == 5);
    mh::Msg m;
    return report(mh::mom_scratch_check(m, v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], v[4]), m);
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
                CHECK(b + (i - b) / walkers * walkers == i);                       // walker b arrives at i
                CHECK(walkers == 1 || (i + walkers - other) % walkers != 0);       // its neighbour does not
            }
    }
    return 0;
}

static int layout(const std::vector<ull> &v)
{
    CHECK(v.size() >= 4);
    const ull cols = v[0];
    const uint32_t k = (uint32_t)v[1], degree = (uint32_t)v[2], n_ranges = (uint32_t)v[3];
    std::vector<uint64_t> ranges(v.begin() + 4, v.end());
    CHECK(ranges.size() == 2 * (size_t)n_ranges);
    const uint64_t scratch_bytes = mh::mom_scratch_bytes(cols, k, degree, n_ranges);
    {   // the shape and the ranges pass, with stand-in pointers
        const mh::MomArgs a = {64, 4 * cols, 64, 4 * cols, k, cols, ranges.data(), n_ranges, degree, 0, 0, 64, 0, 64, scratch_bytes};
        mh::Msg m;
        CHECK(mh::mom_check(m, a) == MH_OK);
    }
    mh::MomLayout M;
    mh::mom_layout(ranges.data(), n_ranges, k, degree, &M);
    const mh::MomRanges &R = M.ranges;
    CHECK(R.n == n_ranges && M.per == 3 * degree + 4 && M.per <= mh::kMomMaxPer);
    CHECK(R.run_first[0] == 0 && R.run_first[mh::kMomMaxRanges] == M.runs && R.run_first[n_ranges] == M.runs);
    CHECK(M.items == M.runs * k && M.used_bytes == M.items * M.per * 8 && M.used_bytes / 8 / M.per == M.items);
    CHECK(M.used_bytes <= scratch_bytes);  // what the caller was asked for covers the last item's last partial sum
    const ull few = 2048;
    for (uint32_t r = 0; r < n_ranges; ++r) {  // the runs of range r partition it: all of them, or the ends of the list
        const ull a = ranges[2 * r], b = ranges[2 * r + 1], runs = R.run_first[r + 1] - R.run_first[r];
        CHECK(runs * mh::kMomRun >= b - a && (runs == 0 ? a == b : (runs - 1) * mh::kMomRun < b - a));
        ull covered = a;
        for (ull i = 0; i < runs; ++i) {
            if (i == few && runs > 2 * few) i = runs - few, covered = a + i * mh::kMomRun;
            uint64_t c0, c1;
            CHECK(mh::mom_run_cols(R, R.run_first[r] + i, &c0, &c1) == r);
            CHECK(c0 == covered && c0 == a + i * mh::kMomRun && c1 > c0 && c1 <= b && c1 - c0 <= mh::kMomRun);
            CHECK(c1 - c0 == mh::kMomRun || i == runs - 1);
            covered = c1;
        }
        CHECK(covered == b);
        // the sum kernel's reads of this range: ((run_first[r] + i) * k + j) * per + s, the last one inside what was written
        if (runs) CHECK(((R.run_first[r] + runs - 1) * k + (k - 1)) * M.per + M.per - 1 < M.used_bytes / 8);
    }
    CHECK(M.grid == (M.items < mh::kMomMaxBlocks ? M.items : mh::kMomMaxBlocks));
    if (M.items) {
        if (int rc = strided(M.items, M.grid)) return rc;
    }
    CHECK(M.elements == n_ranges * k * M.per);
    {
        const uint32_t blocks = (M.elements + mh::kMomSumThreads - 1) / mh::kMomSumThreads;
        CHECK(M.sum_grid >= 1 && M.sum_grid == (blocks < mh::kMomSumMaxBlocks ? blocks : mh::kMomSumMaxBlocks));
        if (int rc = strided(M.elements, (ull)M.sum_grid * mh::kMomSumThreads)) return rc;
    }
    // ---- mhc_polyval on the same cols and k
    mh::PolyLayout P;
    mh::poly_layout(cols, k, &P);
    CHECK(P.tiles * mh::kPolyTile >= cols && (P.tiles - 1) * mh::kPolyTile < cols);
    CHECK(P.items == P.tiles * k && P.grid >= 1 && P.grid == (P.items < mh::kPolyMaxBlocks ? P.items : mh::kPolyMaxBlocks));
    CHECK(mh::kPolyTile == 4 * mh::kPolyThreads);  // thread t owns the tile's columns 4t .. 4t + 3: every column one owner
    if (int rc = strided(P.items, P.grid)) return rc;
    printf("%llu %llu %u %llu %u %u %u %llu %llu %llu %u\n", (ull)M.runs, (ull)M.items, M.per, (ull)M.used_bytes, M.grid, M.elements,
           M.sum_grid, (ull)scratch_bytes, (ull)P.tiles, (ull)P.items, P.grid);
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
        if (wl == 3 && !strncmp(s, "mom", 3))
            rc = check_mom(v);
        else if (wl == 4 && !strncmp(s, "poly", 4))
            rc = check_poly(v);
        else if (wl == 7 && !strncmp(s, "scratch", 7))
            rc = check_scratch(v);
        else if (wl == 6 && !strncmp(s, "layout", 6))
            rc = layout(v);
        else
            return 3;
        if (rc) return rc;
    }
    return 0;
}
