// wiener_check.cpp -- walks what csrc/mh_wiener_layout.hpp decides for mhw_xty and mhw_fir (the argument rules, the runs,
// the scratch, the workgroup tiles, the M-tiles and the capped grids) as a plain host program: no HIP, no Python, so that
// it can be built with -fsanitize=address,undefined (tests/test_host_wiener.py).  Reads lines from stdin:
//   xty x x_row_stride rows cols lags clip y y_row_stride k out accumulate scratch scratch_bytes
//   fir x x_row_stride rows cols lags clip w bias k out out_row_stride
//   scratch rows cols lags k bytes_pointer
//         (pointers as plain numbers, 0 = NULL; nothing is read through them)
//     -> "ok", or "error <code> <message>"
//   layout rows cols lags k        (a shape that passes the check)
//     -> runs items per_item scratch_bytes grid elements sum_grid tile_outputs tiles per_mtile mtiles fir_items fir_grid
//        after checking what the kernels rely on: the runs partition [0, cols); the scratch covers every item's partial
//        sums and the sum kernel's reads; the workgroup tiles own every output column once, overlap by lags - 1 P
//        columns and stay inside a tile's 512; the M-tiles hold whole outputs, each output once; the grids are under
//        their caps and the stride loops reach every item.  What is too large to enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_wiener_layout.hpp"

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

static int check_xty(const ull *v)
{
    const mh::XtyArgs a = {v[0], v[1], v[2], v[3], (uint32_t)v[4], (uint32_t)v[5], v[6], v[7], (uint32_t)v[8], v[9], (uint32_t)v[10],
                           v[11], v[12]};
    mh::Msg m;
    return report(mh::xty_check(m, a), m);
}

static int check_fir(const ull *v)
{
    const mh::FirArgs a = {v[0], v[1], v[2], v[3], (uint32_t)v[4], (uint32_t)v[5], v[6], v[7], (uint32_t)v[8], v[9], v[10]};
    mh::Msg m;
    return report(mh::fir_check(m, a), m);
}

static int check_scratch(const ull *v)
{
    mh::Msg m;
    return report(mh::xty_scratch_check(m, v[0], v[1], (uint32_t)v[2], (uint32_t)v[3], v[4]), m);
}

// the indices [0, n) a capped grid of `grid` walkers reaches with stride `grid`: all of them once.  Enumerated when
// small; otherwise the arithmetic: walker b takes b, b + grid, ...: index i belongs to walker i % grid alone.
static int strided(ull n, ull grid, ull cap)
{
    CHECK(grid >= 1 && grid <= cap && grid == (n < cap ? n : cap));
    if (n <= (1u << 20)) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (ull b = 0; b < grid; ++b)
            for (ull i = b; i < n; i += grid) CHECK(seen[(size_t)i]++ == 0);
        for (ull i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
    } else {
        const ull ends[2] = {0, n - 4096};
        for (ull e : ends)
            for (ull i = e; i < e + 4096; ++i) {
                const ull b = i % grid, other = (b + 1) % grid;
                CHECK(b + (i - b) / grid * grid == i);                       // walker b arrives at i
                CHECK(grid == 1 || (i + grid - other) % grid != 0);          // its neighbour does not
            }
    }
    return 0;
}

static int layout(ull rows, ull cols, ull lags_, ull k_)
{
    const uint32_t lags = (uint32_t)lags_, k = (uint32_t)k_;
    mh::Msg m;
    CHECK(mh::wiener_shape_check(m, "layout", rows, cols, lags, k) == MH_OK);
    // ---- mhw_xty
    mh::XtyLayout X;
    mh::xty_layout(rows, cols, lags, k, &X);
    CHECK(X.runs * mh::kXtyRun >= cols && (X.runs - 1) * mh::kXtyRun < cols);
    CHECK(X.items == X.runs * rows && X.per_item == lags * k && X.elements == rows * X.per_item);
    CHECK(X.scratch_bytes % 8 == 0);
    {   // the runs partition [0, cols): all of them, or the ends of the list
        const ull few = 4096;
        ull covered = 0;
        for (ull run = 0; run < X.runs; ++run) {
            if (run == few && X.runs > 2 * few) run = X.runs - few, covered = run * mh::kXtyRun;
            uint64_t c0, c1;
            mh::xty_run_cols(run, cols, &c0, &c1);
            CHECK(c0 == covered && c1 > c0 && c1 <= cols && c1 - c0 <= mh::kXtyRun);
            CHECK(c1 - c0 == mh::kXtyRun || run == X.runs - 1);
            covered = c1;
        }
        CHECK(covered == cols);
    }
    // the last item's last partial sum, and the sum kernel's last read (run * elements + e), end inside the scratch
    CHECK(((X.items - 1) * X.per_item + X.per_item) * 8 == X.scratch_bytes);
    CHECK(((X.runs - 1) * X.elements + X.elements) * 8 == X.scratch_bytes);
    CHECK(X.scratch_bytes / 8 / X.per_item == X.items);  // (no wrap)
    if (int rc = strided(X.items, X.grid, mh::kXtyMaxBlocks)) return rc;
    {
        const ull blocks = (X.elements + mh::kXtySumThreads - 1) / mh::kXtySumThreads;
        CHECK(X.sum_grid >= 1 && X.sum_grid == (blocks < mh::kXtySumMaxBlocks ? blocks : mh::kXtySumMaxBlocks));
        // thread g of sum_grid * 256 takes g, g + threads, ...: every element once
        const ull threads = (ull)X.sum_grid * mh::kXtySumThreads;
        CHECK(threads >= (X.elements < threads ? X.elements : threads));
        std::vector<uint8_t> seen((size_t)X.elements, 0);  // at most 2^16 * 2^8
        for (ull g = 0; g < threads; ++g)
            for (ull e = g; e < X.elements; e += threads) CHECK(seen[(size_t)e]++ == 0);
        for (ull e = 0; e < X.elements; ++e) CHECK(seen[(size_t)e] == 1);
    }
    // ---- mhw_fir
    mh::FirLayout F;
    mh::fir_layout(cols, lags, k, &F);
    CHECK(F.tile_outputs == mh::kFirTileCols - (lags - 1) && F.tile_outputs >= 1);
    CHECK(F.tiles * F.tile_outputs >= cols && (F.tiles - 1) * F.tile_outputs < cols);
    CHECK(F.per_mtile >= 1 && F.per_mtile * lags <= mh::kFirMRows && (F.per_mtile + 1) * lags > mh::kFirMRows);
    CHECK((ull)F.mtiles * F.per_mtile >= k && (ull)(F.mtiles - 1) * F.per_mtile < k);
    CHECK(F.items == F.tiles * F.mtiles);
    {   // every output j in exactly one M-tile, whole: its lags rows are consecutive rows below 32
        std::vector<uint8_t> seen(k, 0);
        for (uint32_t mt = 0; mt < F.mtiles; ++mt)
            for (uint32_t jj = 0; jj < F.per_mtile; ++jj) {
                const uint32_t j = mt * F.per_mtile + jj;
                if (j >= k) break;
                CHECK(seen[j]++ == 0);
                CHECK(jj * lags + lags - 1 < mh::kFirMRows);
            }
        for (uint32_t j = 0; j < k; ++j) CHECK(seen[j] == 1);
        // the A operand's row map: row m is (m / lags, m % lags); rows past per_mtile outputs are zero rows
        for (uint32_t mrow = 0; mrow < mh::kFirMRows; ++mrow) CHECK((mrow / lags < F.per_mtile) == (mrow < F.per_mtile * lags));
    }
    {   // the tiles: outputs [i0, i0 + n) with i0 = tile * tile_outputs, P columns [i0, i0 + n + lags - 1) within the
        // tile's 512; consecutive tiles overlap by lags - 1 P columns
        const ull few = 4096;
        ull covered = 0;
        for (ull t = 0; t < F.tiles; ++t) {
            if (t == few && F.tiles > 2 * few) t = F.tiles - few, covered = t * F.tile_outputs;
            const ull i0 = t * F.tile_outputs, left = cols - i0, n = left < F.tile_outputs ? left : F.tile_outputs;
            CHECK(i0 == covered && n >= 1);
            CHECK(n + lags - 1 <= mh::kFirTileCols);                      // the P columns it needs are in its LDS image
            CHECK(i0 + n + lags - 1 <= cols + lags - 1);                  // ... and they exist
            if (t + 1 < F.tiles) CHECK(i0 + mh::kFirTileCols - (i0 + F.tile_outputs) == lags - 1);
            covered = i0 + n;
        }
        CHECK(covered == cols);
    }
    if (int rc = strided(F.items, F.grid, mh::kFirMaxBlocks)) return rc;
    printf("%llu %llu %u %llu %u %llu %u %u %llu %u %u %llu %u\n", (ull)X.runs, (ull)X.items, X.per_item, (ull)X.scratch_bytes, X.grid,
           (ull)X.elements, X.sum_grid, F.tile_outputs, (ull)F.tiles, F.per_mtile, F.mtiles, (ull)F.items, F.grid);
    return 0;
}

int main()
{
    char word[16];
    while (scanf("%15s", word) == 1) {
        ull v[13];
        const int n = !strcmp(word, "xty") ? 13 : !strcmp(word, "fir") ? 11 : !strcmp(word, "scratch") ? 5 : !strcmp(word, "layout") ? 4 : 0;
        if (!n) return 3;
        for (int i = 0; i < n; ++i)
            if (scanf("%llu", &v[i]) != 1) return 3;
        const int rc = n == 13 ? check_xty(v) : n == 11 ? check_fir(v) : n == 5 ? check_scratch(v) : layout(v[0], v[1], v[2], v[3]);
        if (rc) return rc;
    }
    return 0;
}
