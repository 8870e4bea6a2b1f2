// aer_layout_check.cpp -- prints the tile rule and the scratch layout of mhi_aer_to_csr (csrc/mh_aer_layout.hpp, the
// arithmetic the library runs before it launches) as a plain host program: no HIP, no Python, so that it can be built
// with -fsanitize=address,undefined (tests/test_host_aer.py).  Reads "n C" pairs from stdin -- or takes one pair as
// arguments -- and prints per pair either "error <code>" or
//     run waves tile nbits lds_bytes rows groups rows_alloc groups_alloc off_matrix off_partial off_drop bytes grid_tiles
//     grid_cols_x grid_cols_y
// after checking what the kernels rely on.  A line that starts with "check" asks for the verdict of an entry point's
// argument rules, every argument of the ABI but the stream as a number (pointers too, 0 = NULL; nothing is read through
// them), and prints "ok" or "error <code> <message>":
//   check scratch n C bytes
//   check to_csr ticks channels ch_bits n C out_ticks ev_off dropped scratch scratch_bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mh_aer_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

static int one(unsigned long long n, unsigned long long c)
{
    mh::AerLayout L;
    const int rc = c > 0xFFFFFFFFull ? -1 : mh::aer_layout(n, (uint32_t)c, &L);
    if (rc) {
        printf("error %d\n", rc);
        return 0;
    }
    const uint32_t C = (uint32_t)c;
    CHECK(L.run % 64 == 0 && L.run >= mh::kAerMinRun && L.run <= 65536);
    CHECK(L.waves >= 1 && L.waves <= 4 && L.tile == L.waves * L.run);
    CHECK(L.lds_bytes == L.waves * C * 4 && L.lds_bytes <= 65536);
    CHECK((1ull << L.nbits) >= C && (L.nbits == 0 || (1ull << (L.nbits - 1)) < C));
    CHECK(L.rows * L.run >= n && (L.rows == 0 || (L.rows - 1) * L.run < n));       // the rows cover the list exactly
    CHECK(L.groups * mh::kAerGroupRows >= L.rows && L.groups <= 65535);             // a grid's second dimension
    CHECK((L.rows + L.waves - 1) / L.waves <= 0x7FFFFFFFull);
    CHECK(L.rows <= L.rows_alloc && L.groups <= L.groups_alloc);
    CHECK(L.off_matrix % 16 == 0 && L.off_partial % 16 == 0 && L.off_drop % 16 == 0 && L.bytes % 16 == 0 && L.bytes);
    CHECK(L.off_matrix + L.rows * C * 4 <= L.off_partial);                         // sections in order, disjoint
    CHECK(L.off_partial + (L.groups + 1) * C * 4 <= L.off_drop);                   // + the row of totals
    CHECK(L.off_drop + L.rows * 4 <= L.bytes);
    CHECK((unsigned long long)L.grid_tiles * L.waves >= L.rows && (L.rows == 0 || (unsigned long long)(L.grid_tiles - 1) * L.waves < L.rows));
    CHECK(L.grid_cols_x >= 1 && L.grid_cols_x * mh::kAerLayoutColThreads >= C && (L.grid_cols_x - 1) * mh::kAerLayoutColThreads < C);
    CHECK(L.grid_cols_y == L.groups);
    printf("%u %u %u %u %u %llu %llu %llu %llu %llu %llu %llu %llu %u %u %u\n", L.run, L.waves, L.tile, L.nbits, L.lds_bytes,
           (unsigned long long)L.rows, (unsigned long long)L.groups, (unsigned long long)L.rows_alloc,
           (unsigned long long)L.groups_alloc, (unsigned long long)L.off_matrix, (unsigned long long)L.off_partial,
           (unsigned long long)L.off_drop, (unsigned long long)L.bytes, L.grid_tiles, L.grid_cols_x, L.grid_cols_y);
    return 0;
}

// "check <what> <numbers>": 3 when the line is not understood
static int check()
{
    char what[16];
    unsigned long long v[10];
    if (scanf("%15s", what) != 1) return 3;
    const int n = !strcmp(what, "scratch") ? 3 : !strcmp(what, "to_csr") ? 10 : 0;
    if (!n) return 3;
    for (int i = 0; i < n; ++i)
        if (scanf("%llu", &v[i]) != 1) return 3;
    mh::Msg m;
    mh::AerLayout L;
    const mh::AerArgs a = {v[0], v[1], (uint32_t)v[2], v[3], (uint32_t)v[4], v[5], v[6], v[7], v[8], v[9]};
    const int rc = n == 3 ? mh::aer_scratch_check(m, v[0], (uint32_t)v[1], v[2], &L) : mh::aer_check(m, a, &L);
    CHECK((rc == MH_OK) == (m.text[0] == 0));
    CHECK(rc == MH_OK || rc == MH_ERR_ARG);
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return one(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10));
    char word[24];
    while (scanf("%23s", word) == 1) {
        unsigned long long c;
        int rc;
        if (!strcmp(word, "check")) {
            rc = check();
        } else {
            if (scanf("%llu", &c) != 1) return 3;
            rc = one(strtoull(word, nullptr, 10), c);
        }
        if (rc) return rc;
    }
    return 0;
}
