// windows_check.cpp -- prints what csrc/mh_windows_layout.hpp decides for mhi_windows (the argument rules, the form and
// the tile of (W, r), the capped grid) as a plain host program: no HIP, no Python, so that it can be built with
// -fsanitize=address,undefined (tests/test_host_windows.py).  Reads lines from stdin:
//   check in row_stride rows cols win_off win_idx n_win n_out W r mode out out_bits out_win_stride out_row_stride sumsq
//         sq_row_stride accumulate bad        (pointers as plain numbers, 0 = NULL; nothing is read through them)
//     -> "ok", or "error <code> <message>"
//   layout mode rows W r n_win                (arguments that pass the check)
//     -> form nb tile_bins tiles items per_block grid max_blocks
//        after checking what the kernels rely on: the tiles cover [0, nb) exactly once, a staged tile fits its LDS, the
//        grid is capped and, below the cap, holds every item.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mh_windows_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

static int check(const unsigned long long *v)
{
    const mh::WinArgs a = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], (uint32_t)v[10], v[11], (uint32_t)v[12],
                           v[13], v[14], v[15], v[16], (uint32_t)v[17], v[18]};
    mh::Msg m;
    const int rc = mh::windows_check(m, a);
    CHECK((rc == MH_OK) == (m.text[0] == 0));
    CHECK(rc == MH_OK || rc == MH_ERR_ARG);
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

static int layout(unsigned long long mode, unsigned long long rows, unsigned long long W, unsigned long long r,
                  unsigned long long n_win)
{
    CHECK(mode <= 1 && rows >= 1 && W >= 1 && r >= 1 && W < mh::kWinMax32 && r < mh::kWinMax32 && n_win < mh::kWinMax32);
    mh::WinLayout L;
    mh::windows_layout((uint32_t)mode, rows, W, r, n_win, &L);
    CHECK((unsigned long long)L.nb * r >= W && (unsigned long long)(L.nb - 1) * r < W);           // nb = ceil(W / r)
    CHECK(L.form == (r == 1 ? mh::kWinLane : r <= mh::kWinStageMaxR ? mh::kWinStage : mh::kWinWave));
    CHECK(L.tile_bins >= 1 && L.tiles >= 1);
    CHECK((unsigned long long)L.tiles * L.tile_bins >= L.nb);                                      // the tiles cover [0, nb)
    CHECK((unsigned long long)(L.tiles - 1) * L.tile_bins < L.nb);                                 // ... and none is empty
    if (L.tiles <= 4096) {                                                                         // ... each bin once
        unsigned long long covered = 0;
        for (uint32_t t = 0; t < L.tiles; ++t) {
            const uint32_t b0 = t * L.tile_bins, n = L.nb - b0 < L.tile_bins ? L.nb - b0 : L.tile_bins;
            CHECK(b0 == covered && n >= 1);
            covered += n;
        }
        CHECK(covered == L.nb);
    }
    if (L.form == mh::kWinLane) CHECK(L.tile_bins == mh::kWinLaneBytes && L.per_block == mh::kWinThreads);
    if (L.form == mh::kWinStage) {
        CHECK(L.tile_bins * r <= mh::kWinStageBytes && L.tile_bins >= 16 && L.tile_bins <= 64 * 16 / 2);
        CHECK((L.tile_bins + 1) * r > mh::kWinStageBytes);
    }
    if (L.form == mh::kWinWave) CHECK(L.tile_bins == 1 && L.tiles == L.nb);
    if (L.form != mh::kWinLane) CHECK(L.per_block == mh::kWinWaves && L.tile_bins <= 64 * 8);     // a lane per bin: see below
    CHECK(L.items == (mode == mh::kWinStack ? n_win : 1) * rows * L.tiles);
    CHECK(L.grid <= mh::kWinMaxBlocks);
    if (L.items == 0)
        CHECK(L.grid == 0 && mode == mh::kWinStack && n_win == 0);
    else
        CHECK(L.grid >= 1);
    if (L.grid < mh::kWinMaxBlocks)                                                                // below the cap: one trip
        CHECK((unsigned long long)L.grid * L.per_block >= L.items && (unsigned long long)(L.grid ? L.grid - 1 : 0) * L.per_block < L.items + (L.items == 0));
    printf("%u %u %u %u %llu %u %u %u\n", L.form, L.nb, L.tile_bins, L.tiles, (unsigned long long)L.items, L.per_block, L.grid,
           mh::kWinMaxBlocks);
    return 0;
}

int main()
{
    char word[16];
    while (scanf("%15s", word) == 1) {
        unsigned long long v[19];
        const int n = !strcmp(word, "check") ? 19 : !strcmp(word, "layout") ? 5 : 0;
        if (!n) return 3;
        for (int i = 0; i < n; ++i)
            if (scanf("%llu", &v[i]) != 1) return 3;
        const int rc = n == 19 ? check(v) : layout(v[0], v[1], v[2], v[3], v[4]);
        if (rc) return rc;
    }
    return 0;
}
