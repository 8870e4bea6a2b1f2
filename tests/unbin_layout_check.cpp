// unbin_layout_check.cpp -- prints the tile rule and the scratch layout of mhi_unbin_count / mhi_unbin_emit
// (csrc/mh_unbin_layout.hpp, the arithmetic the library runs before it launches) as a plain host program: no HIP, no
// Python, so that it can be built with -fsanitize=address,undefined (tests/test_host_unbin.py).  Reads "form rows cols"
// triples from stdin -- or takes one as arguments -- and prints per triple either "error <code>" or
//     tile group tiles_per_row tiles groups off_sum off_base off_partial bytes grid grid_scan
// after checking what the kernels rely on.  A line that starts with "check" asks for the verdict of an entry point's
// argument rules, every argument of the ABI but the stream as a number (pointers too, 0 = NULL; nothing is read through
// them), and prints "ok" or "error <code> <message>":
//   check scratch form rows cols bytes
//   check count form in row_off rows cols ev_off total scratch scratch_bytes
//   check emit form in row_off rows cols origin period phase out_ticks out_ch ch_bits capacity over scratch scratch_bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mh_unbin_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

static int one(unsigned long long form, unsigned long long rows, unsigned long long cols)
{
    mh::UnbinLayout L;
    const int rc = form > 0xFFFFFFFFull ? -1 : mh::unbin_layout((uint32_t)form, rows, cols, &L);
    if (rc) {
        printf("error %d\n", rc);
        return 0;
    }
    const unsigned __int128 bytes_in = (unsigned __int128)rows * cols;
    CHECK(L.tiles >= 1 && L.tiles <= mh::kUnbinMaxTiles);
    CHECK((L.tiles + mh::kUnbinWaves - 1) / mh::kUnbinWaves <= 0x7FFFFFFFull);        // a grid's first dimension
    if (form == mh::kUnbinCsr) {
        CHECK(L.tiles_per_row >= 1 && (unsigned __int128)L.tiles_per_row * mh::kUnbinTile >= cols);
        CHECK((unsigned __int128)(L.tiles_per_row - 1) * mh::kUnbinTile < cols);      // the tiles cover a row exactly
        CHECK((unsigned __int128)L.tiles_per_row * rows == L.tiles);
    } else {
        CHECK(L.tiles_per_row == 0);
        CHECK((unsigned __int128)L.tiles * mh::kUnbinTile >= bytes_in);
        CHECK((unsigned __int128)(L.tiles - 1) * mh::kUnbinTile < bytes_in);
    }
    CHECK(L.groups >= 1 && L.groups * mh::kUnbinGroup >= L.tiles && (L.groups - 1) * mh::kUnbinGroup < L.tiles);
    CHECK(L.groups <= 0x7FFFFFFFull);
    CHECK(L.off_sum % 16 == 0 && L.off_base % 16 == 0 && L.off_partial % 16 == 0 && L.bytes % 16 == 0 && L.bytes);
    CHECK(L.off_sum + L.tiles * 4 <= L.off_base);                                     // sections in order, disjoint
    CHECK(L.off_base + L.tiles * 8 <= L.off_partial);
    CHECK(L.off_partial + (L.groups + 1) * 8 <= L.bytes);                             // + the total
    CHECK((unsigned long long)L.grid * mh::kUnbinWaves >= L.tiles && (unsigned long long)(L.grid - 1) * mh::kUnbinWaves < L.tiles);
    CHECK(L.grid_scan == L.groups);
    printf("%u %u %llu %llu %llu %llu %llu %llu %llu %u %u\n", mh::kUnbinTile, mh::kUnbinGroup, (unsigned long long)L.tiles_per_row,
           (unsigned long long)L.tiles, (unsigned long long)L.groups, (unsigned long long)L.off_sum,
           (unsigned long long)L.off_base, (unsigned long long)L.off_partial, (unsigned long long)L.bytes, L.grid, L.grid_scan);
    return 0;
}

static int verdict(int rc, const mh::Msg &m)
{
    CHECK((rc == MH_OK) == (m.text[0] == 0));
    CHECK(rc == MH_OK || rc == MH_ERR_ARG);
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

// "check <what> <numbers>": 3 when the line is not understood
static int check()
{
    char what[16];
    unsigned long long v[15];
    if (scanf("%15s", what) != 1) return 3;
    const int n = !strcmp(what, "scratch") ? 4 : !strcmp(what, "count") ? 9 : !strcmp(what, "emit") ? 15 : 0;
    if (!n) return 3;
    for (int i = 0; i < n; ++i)
        if (scanf("%llu", &v[i]) != 1) return 3;
    mh::Msg m;
    mh::UnbinLayout L;
    const mh::UnbinArgs s = {(uint32_t)v[0], v[1], v[2], v[3], v[4], v[n - 2], v[n - 1]};
    if (n == 4) return verdict(mh::unbin_scratch_check(m, (uint32_t)v[0], v[1], v[2], v[3], &L), m);
    if (n == 9) return verdict(mh::unbin_count_check(m, mh::UnbinCountArgs{s, v[5], v[6]}, &L), m);
    return verdict(mh::unbin_emit_check(m, mh::UnbinEmitArgs{s, v[5], v[6], v[7], v[8], v[9], (uint32_t)v[10], v[11], v[12]}, &L), m);
}

int main(int argc, char **argv)
{
    if (argc == 4)
        return one(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    char word[24];
    while (scanf("%23s", word) == 1) {
        unsigned long long r, c;
        int rc;
        if (!strcmp(word, "check")) {
            rc = check();
        } else {
            if (scanf("%llu %llu", &r, &c) != 2) return 3;
            rc = one(strtoull(word, nullptr, 10), r, c);
        }
        if (rc) return rc;
    }
    return 0;
}
