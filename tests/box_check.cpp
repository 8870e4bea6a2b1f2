// box_check.cpp -- walks what csrc/mh_smooth_layout.hpp decides for mhs_box and mhs_box_f32 (the argument rules, the tiles,
// the halos, the dwords a workgroup may load and the capped grids) as a plain host program: no HIP, no Python, so that it
// can be built with -fsanitize=address,undefined (tests/test_host_box.py).  Reads lines from stdin:
//   box x x_row_stride rows cols window clip lo hi out_row_stride
//   boxf in in_row_stride k cols window bias out out_row_stride
//         (pointers as plain numbers, 0 = NULL; nothing is read through them)
//     -> "ok", or "error <code> <message>"
//   layout rows cols window k x x_row_stride        (a shape that passes the checks; x is the address of the first byte)
//     -> tiles items grid boxf_tiles boxf_items boxf_grid
//        after checking what the kernels rely on: the tiles partition the columns and start on 16-byte boundaries of the
//        output; of the first and last rows and tiles, the span holds the shift, the tile and its halo, every byte the
//        tile needs lies in a dword that is loaded, every dword that is loaded holds a byte of the row, and the largest
//        prefix index is inside the span; the grids are under their caps and the stride loops reach every item once.
//        What is too large to enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_smooth_layout.hpp"

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

static int check_box(const std::vector<ull> &v)
{
    CHECK(v.size() == 9);
    const mh::BoxArgs a = {v[0], v[1], v[2], v[3], (uint32_t)v[4], (uint32_t)v[5], v[6], v[7], v[8]};
    mh::Msg m;
    return report(mh::box_check(m, a), m);
}

static int check_boxf(const std::vector<ull> &v)
{
    CHECK(v.size() == 8);
    const mh::BoxfArgs a = {v[0], v[1], (uint32_t)v[2], v[3], (uint32_t)v[4], v[5], v[6], v[7]};
    mh::Msg m;
    return report(mh::boxf_check(m, a), m);
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

// one (channel, tile) as k_box walks it
static int walk_tile(ull x, ull x_row_stride, ull cols, uint32_t window, ull c, ull tile)
{
    uint64_t i0;
    const uint32_t n = mh::box_tile_outputs(tile, cols, &i0);
    CHECK(n >= 1 && n <= mh::kBoxTileCols && i0 % 16 == 0 && i0 + n <= cols);
    const ull row = x + c * x_row_stride, row_end = row + cols + window - 1;
    const ull first = row + i0, need_end = first + n + window - 1;
    CHECK(need_end <= row_end);
    const uint32_t shift = (uint32_t)(first & (mh::kBoxGroup - 1));
    const ull base = first - shift;
    CHECK(base % 16 == 0 && shift + n + window - 1 <= mh::kBoxSpan);
    CHECK(shift + (n - 1) + window <= mh::kBoxSpan);  // the largest index into the prefix sums P[0 .. kBoxSpan]
    std::vector<uint8_t> loaded(mh::kBoxSpan, 0);
    for (uint32_t t = 0; t < mh::kBoxThreads; ++t) {
        const ull ga = base + (ull)mh::kBoxGroup * t;
        const bool whole = mh::box_dword_ok(ga, row, need_end) && mh::box_dword_ok(ga + 12, row, need_end);
        for (uint32_t k = 0; k < 4; ++k) {
            const ull a = ga + 4 * k;
            const bool ok = mh::box_dword_ok(a, row, need_end);
            CHECK(!whole || ok);  // a group that is loaded at once has four dwords that may be
            if (!ok) continue;
            CHECK(a % 4 == 0 && a + 4 > row && a < row_end);  // the dword holds a byte of the row
            for (uint32_t b = 0; b < 4; ++b) loaded[mh::kBoxGroup * t + 4 * k + b] = 1;
        }
    }
    for (ull p = shift; p < shift + n + window - 1; ++p) CHECK(loaded[(size_t)p]);  // every byte the tile needs
    return 0;
}

static int layout(const std::vector<ull> &v)
{
    CHECK(v.size() == 6);
    const ull rows = v[0], cols = v[1], x = v[4], xs = v[5];
    const uint32_t window = (uint32_t)v[2], k = (uint32_t)v[3];
    {   // the shape passes, with stand-in output pointers far behind x
        const ull far = 1ull << 62;
        const mh::BoxArgs a = {x, xs, rows, cols, window, 255, far, far + (1ull << 60), (cols + 15) / 16 * 16};
        mh::Msg m;
        CHECK(mh::box_check(m, a) == MH_OK);
        const mh::BoxfArgs f = {64, 4 * cols, k, cols, window, 1ull << 61, far, 4 * cols};
        CHECK(mh::boxf_check(m, f) == MH_OK);
    }
    mh::BoxLayout L;
    mh::box_layout(rows, cols, true, &L);
    CHECK(L.tiles * mh::kBoxTileCols >= cols && (L.tiles - 1) * mh::kBoxTileCols < cols);
    CHECK(L.items == rows * L.tiles && L.items / rows == L.tiles && L.planes == 2);
    CHECK(L.grid >= 1 && L.grid == (L.items < mh::kBoxMaxBlocks ? L.items : mh::kBoxMaxBlocks));
    mh::BoxLayout one;
    mh::box_layout(rows, cols, false, &one);
    CHECK(one.planes == 1 && one.items == L.items && one.grid == L.grid);
    const ull cs[2] = {0, rows - 1}, ts[4] = {0, L.tiles > 1 ? 1ull : 0ull, L.tiles > 1 ? L.tiles - 2 : 0ull, L.tiles - 1};
    for (ull c : cs)
        for (ull t : ts) {
            uint64_t cc, tt;
            mh::box_item(c * L.tiles + t, L.tiles, &cc, &tt);
            CHECK(cc == c && tt == t);
            if (int rc = walk_tile(x, rows > 1 ? xs : 0, cols, window, c, t)) return rc;
        }
    {   // consecutive tiles share nothing of the output and leave nothing out
        uint64_t a0, a1;
        const uint32_t n0 = mh::box_tile_outputs(0, cols, &a0);
        CHECK(a0 == 0);
        if (L.tiles > 1) {
            mh::box_tile_outputs(1, cols, &a1);
            CHECK(a1 == n0);
        }
        uint64_t z;
        const uint32_t nz = mh::box_tile_outputs(L.tiles - 1, cols, &z);
        CHECK(z + nz == cols);
    }
    if (int rc = strided(L.items, L.grid)) return rc;
    mh::BoxfLayout F;
    mh::boxf_layout(cols, k, &F);
    CHECK(F.tiles * mh::kBoxfTile >= cols && (F.tiles - 1) * mh::kBoxfTile < cols);
    CHECK(F.items == F.tiles * k && F.grid >= 1 && F.grid == (F.items < mh::kBoxfMaxBlocks ? F.items : mh::kBoxfMaxBlocks));
    CHECK(mh::kBoxfTile == mh::kBoxfThreads);  // thread t owns the tile's column t: every column one owner
    if (int rc = strided(F.items, F.grid)) return rc;
    printf("%llu %llu %u %llu %llu %u\n", (ull)L.tiles, (ull)L.items, L.grid, (ull)F.tiles, (ull)F.items, F.grid);
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
        if (wl == 3 && !strncmp(s, "box", 3))
            rc = check_box(v);
        else if (wl == 4 && !strncmp(s, "boxf", 4))
            rc = check_boxf(v);
        else if (wl == 6 && !strncmp(s, "layout", 6))
            rc = layout(v);
        else
            return 3;
        if (rc) return rc;
    }
    return 0;
}
