// lstm_check.cpp -- walks what csrc/mh_lstm_layout.hpp decides for mhl_inproj and mhl_windows (the argument rules, the tiles,
// the bytes a lane may load, the permutation of the gates, the scratch and the capped grids) as a plain host program: no HIP,
// no Python, so that it can be built with -fsanitize=address,undefined (tests/test_host_lstm.py).  Reads lines from stdin:
//   inproj x x_row_stride rows cols clip wx bias units p
//   windows p cols lags units wh wd bd k out out_row_stride
//         (pointers as plain numbers, 0 = NULL; nothing is read through them)
//     -> "ok", or "error <code> <message>"
//   layout cols lags units                              (a shape that passes the checks)
//     -> in_tiles gtiles in_grid win_tiles blocks per_wave ksteps win_grid p_bytes
//        after checking what the kernels rely on.  mhl_inproj: the tiles partition the columns and the g-tiles the 4 units
//        pre-activations; of the first two and the last tile, at every alignment of a row's first byte, a lane's dwords lie
//        inside the row where dwords_ok says so and the byte path stays inside it otherwise; every (bin, pre-activation)
//        a lane stores lies inside p's inproj_bytes; the grid is under its cap and the stride loop reaches every item once.
//        mhl_windows: the tiles partition the windows, every row of p a window reads lies inside p; the registers of the
//        blocks name every (gate, unit) once and as the row of Wh the A operand holds; a wave owns at most per_wave blocks;
//        the k-steps cover the units and h's LDS image; the grid is under its cap and the stride loop reaches every tile
//        once.  What is too large to enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_lstm_layout.hpp"

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

static int check_inproj(const std::vector<ull> &v)
{
    CHECK(v.size() == 9);
    const mh::InprojArgs a = {v[0], v[1], v[2], v[3], (uint32_t)v[4], v[5], v[6], (uint32_t)v[7], v[8]};
    mh::Msg m;
    return report(mh::inproj_check(m, a), m);
}

static int check_windows(const std::vector<ull> &v)
{
    CHECK(v.size() == 10);
    const mh::WindowsArgs a = {v[0], v[1], (uint32_t)v[2], (uint32_t)v[3], v[4], v[5], v[6], (uint32_t)v[7], v[8], v[9]};
    mh::Msg m;
    return report(mh::windows_check(m, a), m);
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

// one column tile of mhl_inproj as k_inproj walks it, the row's first byte `sh` bytes behind a dword boundary: the loads
// of every lane, and the stores of the g-tile `gt`
static int walk_inproj_tile(ull tile, ull cols, uint32_t units, uint32_t gt, uint32_t sh)
{
    const ull row = (1ull << 32) + sh;  // any address with that alignment
    const ull G = 4ull * units, bytes = mh::inproj_bytes(cols, units);
    for (uint32_t wave = 0; wave < mh::kInThreads / 64; ++wave) {
        const ull t0 = tile * mh::kInTileCols + (ull)wave * mh::kInWaveCols;
        std::vector<uint8_t> stored(mh::kInWaveCols, 0);
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t col = lane & 31, h = lane >> 5;
            const ull u = t0 + 4 * col;
            if (u < cols) {
                if (mh::dwords_ok(u, sh, cols)) {
                    CHECK(u >= sh);
                    const ull a0 = row + u - sh, end = a0 + (sh ? 8 : 4);
                    CHECK(a0 % 4 == 0 && a0 >= row && end <= row + cols);   // aligned, inside the row
                    CHECK(a0 <= row + u && row + u + 4 <= end);             // and they hold the 4 columns
                } else {
                    for (uint32_t b = 0; b < 4; ++b)
                        if (u + b < cols) CHECK(row + u + b < row + cols);
                    CHECK(u == 0 || u + 8 > cols);                          // only at a row's two ends
                }
            }
            const ull g = (ull)gt * mh::kInGTile + col;
            if (g >= G) continue;
            for (uint32_t r = 0; r < 16; ++r) {
                const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * h;
                CHECK(i < 32);
                for (uint32_t b = 0; b < 4; ++b) {
                    const ull t = t0 + 4 * i + b;
                    if (col == 0) CHECK(stored[(size_t)(t - t0)]++ == 0);   // every column of the wave one (register, tile)
                    if (t < cols) CHECK((t * G + g + 1) * 4 <= bytes);
                }
            }
        }
        if ((ull)gt * mh::kInGTile < G)
            for (uint32_t i = 0; i < mh::kInWaveCols; ++i) CHECK(stored[i] == 1);
    }
    return 0;
}

static int layout(const std::vector<ull> &v)
{
    CHECK(v.size() == 3);
    const ull cols = v[0];
    const uint32_t lags = (uint32_t)v[1], units = (uint32_t)v[2];
    const ull far = 1ull << 62, G = 4ull * units;
    {   // the shape passes, with stand-in pointers far from each other
        const mh::InprojArgs a = {1ull << 32, cols, 2, cols, 255, 1ull << 50, 1ull << 51, units, far};
        const mh::WindowsArgs w = {far, cols, lags, units, 1ull << 50, 1ull << 51, 1ull << 52, 8, 1ull << 40, 4 * cols};
        mh::Msg m;
        CHECK(mh::inproj_check(m, a) == MH_OK);
        CHECK(mh::windows_check(m, w) == MH_OK);
    }
    mh::InprojLayout P;
    mh::inproj_layout(cols, units, &P);
    CHECK(P.tiles * mh::kInTileCols >= cols && (P.tiles - 1) * mh::kInTileCols < cols);
    CHECK((ull)P.gtiles * mh::kInGTile >= G && (ull)(P.gtiles - 1) * mh::kInGTile < G);
    CHECK(P.items == P.tiles * P.gtiles);
    CHECK(P.grid >= 1 && P.grid == (P.items < mh::kInMaxBlocks ? P.items : mh::kInMaxBlocks));
    CHECK(mh::kInTileCols == mh::kInWaveCols * (mh::kInThreads / 64) && mh::kInWaveCols == 4 * 32 && mh::kInGTile == 32);
    CHECK(mh::inproj_bytes(cols, units) == cols * G * 4);
    const ull ts[3] = {0, P.tiles > 1 ? 1ull : 0ull, P.tiles - 1};
    for (ull t : ts)
        for (uint32_t sh = 0; sh < 4; ++sh) {
            if (int rc = walk_inproj_tile(t, cols, units, 0, sh)) return rc;
            if (int rc = walk_inproj_tile(t, cols, units, P.gtiles - 1, sh)) return rc;
        }
    if (int rc = strided(P.items, P.grid)) return rc;

    mh::WinLayout W;
    mh::windows_layout(cols, lags, units, &W);
    CHECK(W.windows == cols - lags + 1 && W.windows >= 1);
    CHECK(W.tiles * mh::kWinTile >= W.windows && (W.tiles - 1) * mh::kWinTile < W.windows);
    CHECK(W.grid >= 1 && W.grid == (W.tiles < mh::kWinMaxBlocks ? W.tiles : mh::kWinMaxBlocks));
    CHECK(W.blocks * mh::kWinBlockUnits >= units && (W.blocks - 1) * mh::kWinBlockUnits < units);
    CHECK(W.per_wave >= 1 && W.per_wave <= 2 && W.blocks <= W.per_wave * mh::kWinWaves);
    CHECK((W.per_wave == 1) == (W.ksteps <= 32));                       // what mhl_windows' dispatch relies on
    CHECK(W.ksteps % mh::kWinKGroup == 0 && W.ksteps <= 64 && 2 * W.ksteps >= units && 2 * (W.ksteps - mh::kWinKGroup) < units);
    // the rows of p the windows of the first, the second and the last tile read: inside p
    const ull ws[3] = {0, W.tiles > 1 ? 1ull : 0ull, W.tiles - 1};
    for (ull t : ws)
        for (uint32_t n = 0; n < mh::kWinTile; ++n) {
            const ull i = t * mh::kWinTile + n;
            if (i >= W.windows) continue;
            CHECK(i + lags - 1 < cols && (i + lags) * G * 4 <= mh::inproj_bytes(cols, units));
        }
    // the permutation: the registers of the blocks name every (gate, unit) once, as the row the A operand holds
    std::vector<uint8_t> seen((size_t)G, 0);
    for (uint32_t q = 0; q < W.blocks; ++q) {
        CHECK(q % mh::kWinWaves < mh::kWinWaves && q / mh::kWinWaves < W.per_wave);   // wave q % 8 owns it as its block q / 8
        for (uint32_t h = 0; h < 2; ++h)
            for (uint32_t r = 0; r < 16; ++r) {
                const uint32_t m = (r & 3) + 8 * (r >> 2) + 4 * h;  // the row of the C layout
                const uint32_t unit = mh::win_unit(q, h, r), gate = mh::win_gate(r);
                CHECK(unit == mh::win_row_unit(q, m) && gate == mh::win_row_gate(m) && gate < 4);
                CHECK(mh::win_unit(q, h, r & 3) == unit);           // the four gates of a unit lie in one lane
                if (unit < units) CHECK(seen[(size_t)(gate * units + unit)]++ == 0);
                if (unit < units) CHECK(unit < 2 * W.ksteps);       // its row of h's LDS image
            }
    }
    for (ull g = 0; g < G; ++g) CHECK(seen[(size_t)g] == 1);
    if (int rc = strided(W.tiles, W.grid)) return rc;
    printf("%llu %u %u %llu %u %u %u %u %llu\n", (ull)P.tiles, P.gtiles, P.grid, (ull)W.tiles, W.blocks, W.per_wave, W.ksteps, W.grid,
           (ull)mh::inproj_bytes(cols, units));
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
        if (wl == 6 && !strncmp(s, "inproj", 6))
            rc = check_inproj(v);
        else if (wl == 7 && !strncmp(s, "windows", 7))
            rc = check_windows(v);
        else if (wl == 6 && !strncmp(s, "layout", 6))
            rc = layout(v);
        else
            return 3;
        if (rc) return rc;
    }
    return 0;
}
