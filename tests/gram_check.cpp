// gram_check.cpp -- walks what csrc/mh_gram_layout.hpp decides for mhi_gram (the argument rules, the tiles, the runs of K
// slices, the capped grid and which (tile, run) a workgroup owns) as a plain host program: no HIP, no Python, so that it
// can be built with -fsanitize=address,undefined (tests/test_host_gram.py).  Reads lines from stdin:
//   check a a_row_stride a_rows b b_row_stride b_rows cols gram gram_row_stride sum_a sum_b accumulate
//         (pointers as plain numbers, 0 = NULL; nothing is read through them)
//     -> "ok", or "error <code> <message>"
//   layout a_rows b_rows cols symmetric       (arguments that pass the check)
//     -> nta ntb tiles slices run_slices runs items grid max_blocks longest_run
//        after checking what the kernel relies on: the runs cover [0, cols) once and none is longer than an int32
//        accumulator holds, every element of the result -- in the symmetric form every one with tile column >= tile row,
//        and no other -- is owned exactly once per run, the grid is a multiple of 8 under its cap, and the workgroups'
//        walks visit every item once.  What is too large to enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_gram_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

typedef unsigned long long ull;

static int check(const ull *v)
{
    const mh::GramArgs a = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], (uint32_t)v[11]};
    mh::Msg m;
    const int rc = mh::gram_check(m, a);
    CHECK((rc == MH_OK) == (m.text[0] == 0));
    CHECK(rc == MH_OK || rc == MH_ERR_ARG);
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

static mh::GramItem owner(const mh::GramLayout &L, uint64_t item)
{
    return mh::gram_owner(L.symmetric, L.nta, L.ntb, L.tiles, L.run_slices, L.cols, item);
}

// the tiles of one run: each (ti, tj) once, and in the symmetric form exactly those with tj >= ti
static int tiles_of_run(const mh::GramLayout &L, uint64_t run, uint64_t k0, uint64_t k1)
{
    std::vector<uint8_t> seen((size_t)L.nta * L.ntb, 0);
    for (uint64_t t = 0; t < L.tiles; ++t) {
        const mh::GramItem it = owner(L, run * L.tiles + t);
        CHECK(it.k0 == k0 && it.k1 == k1);
        CHECK(it.ti < L.nta && it.tj < L.ntb);
        if (L.symmetric) CHECK(it.tj >= it.ti);
        CHECK(seen[(size_t)it.ti * L.ntb + it.tj]++ == 0);
    }
    for (uint32_t i = 0; i < L.nta; ++i)
        for (uint32_t j = 0; j < L.ntb; ++j) CHECK(seen[(size_t)i * L.ntb + j] == (L.symmetric ? j >= i : 1));
    return 0;
}

static int layout(ull a_rows, ull b_rows, ull cols, ull symmetric)
{
    CHECK(a_rows >= 1 && b_rows >= 1 && cols >= 1 && cols < mh::kGramMaxCols && symmetric <= 1 && (!symmetric || a_rows == b_rows));
    mh::GramLayout L;
    mh::gram_layout(a_rows, b_rows, cols, symmetric != 0, &L);
    CHECK((ull)L.nta * mh::kGramTile >= a_rows && (ull)(L.nta - 1) * mh::kGramTile < a_rows);
    CHECK((ull)L.ntb * mh::kGramTile >= b_rows && (ull)(L.ntb - 1) * mh::kGramTile < b_rows);
    CHECK(L.tiles == (symmetric ? (ull)L.nta * (L.nta + 1) / 2 : (ull)L.nta * L.ntb));
    CHECK(L.slices * mh::kGramSlice >= cols && (L.slices - 1) * mh::kGramSlice < cols);
    CHECK(L.run_slices >= 1 && L.run_slices <= mh::kGramRunSlices);
    CHECK(L.runs * L.run_slices >= L.slices && (L.runs - 1) * L.run_slices < L.slices);
    CHECK(L.items == L.runs * L.tiles);
    const ull run_cols = (ull)L.run_slices * mh::kGramSlice;
    CHECK(run_cols <= mh::kGramInt32Cols && run_cols % mh::kGramStep == 0);
    // the runs cover [0, cols) once, none past the int32 bound: all of them, or the ends of the list
    ull longest = 0;
    const ull few = 4096;
    ull covered = 0;
    for (ull run = 0; run < L.runs; ++run) {
        if (run == few && L.runs > 2 * few) {
            run = L.runs - few;
            covered = run * run_cols;  // the runs in between are whole: k0 = run * run_cols is checked below
        }
        const mh::GramItem it = owner(L, run * L.tiles);
        CHECK(it.k0 == covered && it.k0 == run * run_cols && it.k1 > it.k0 && it.k1 <= cols);
        CHECK(it.k1 - it.k0 <= run_cols && (it.k1 - it.k0 == run_cols || run == L.runs - 1));
        CHECK(it.k1 - it.k0 <= mh::kGramInt32Cols);
        // the padded column count the MFMAs run over stays inside the bound too
        CHECK((it.k1 - it.k0 + mh::kGramStep - 1) / mh::kGramStep * mh::kGramStep <= mh::kGramInt32Cols);
        if (it.k1 - it.k0 > longest) longest = it.k1 - it.k0;
        covered = it.k1;
    }
    CHECK(covered == cols);
    // every tile once per run: the first and the last run
    if (L.tiles <= (1u << 16)) {
        const mh::GramItem first = owner(L, 0), last = owner(L, (L.runs - 1) * L.tiles);
        if (int rc = tiles_of_run(L, 0, first.k0, first.k1)) return rc;
        if (int rc = tiles_of_run(L, L.runs - 1, last.k0, last.k1)) return rc;
    }
    // the grid and the workgroups' walks
    CHECK(L.grid >= mh::kGramXcds && L.grid <= mh::kGramMaxBlocks && L.grid % mh::kGramXcds == 0);
    CHECK(L.grid >= (L.items < mh::kGramMaxBlocks ? L.items : mh::kGramMaxBlocks) && L.grid < L.items + mh::kGramXcds);
    {
        std::vector<uint8_t> start(L.grid, 0);
        for (uint32_t b = 0; b < L.grid; ++b) {
            const uint64_t f = mh::gram_first_item(b, L.grid);
            CHECK(f < L.grid && start[f]++ == 0);
            // the workgroups of one XCD (block % 8) start at a contiguous range of items
            CHECK(f / (L.grid / mh::kGramXcds) == b % mh::kGramXcds);
        }
    }
    if (L.items <= (1u << 20)) {
        std::vector<uint8_t> seen((size_t)L.items, 0);
        for (uint32_t b = 0; b < L.grid; ++b)
            for (uint64_t item = mh::gram_first_item(b, L.grid); item < L.items; item += L.grid) CHECK(seen[(size_t)item]++ == 0);
        for (uint64_t item = 0; item < L.items; ++item) CHECK(seen[(size_t)item] == 1);
    }
    printf("%u %u %llu %llu %u %llu %llu %u %u %llu\n", L.nta, L.ntb, (ull)L.tiles, (ull)L.slices, L.run_slices, (ull)L.runs,
           (ull)L.items, L.grid, mh::kGramMaxBlocks, longest);
    return 0;
}

int main()
{
    char word[16];
    while (scanf("%15s", word) == 1) {
        ull v[12];
        const int n = !strcmp(word, "check") ? 12 : !strcmp(word, "layout") ? 4 : 0;
        if (!n) return 3;
        for (int i = 0; i < n; ++i)
            if (scanf("%llu", &v[i]) != 1) return 3;
        const int rc = n == 12 ? check(v) : layout(v[0], v[1], v[2], v[3]);
        if (rc) return rc;
    }
    return 0;
}
