// unbin_layout_check.cpp -- prints the tile rule and the scratch layout of mhi_unbin_count / mhi_unbin_emit
// (csrc/mh_unbin_layout.hpp, the arithmetic the library runs before it launches) as a plain host program: no HIP, no
// Python, so that it can be built with -fsanitize=address,undefined (tests/test_host_unbin.py).  Reads "form rows cols"
// triples from stdin -- or takes one as arguments -- and prints per triple either "error <code>" or
//     tile group tiles_per_row tiles groups off_sum off_base off_partial bytes
// after checking what the kernels rely on.
#include <cstdio>
#include <cstdlib>

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
    printf("%u %u %llu %llu %llu %llu %llu %llu %llu\n", mh::kUnbinTile, mh::kUnbinGroup, (unsigned long long)L.tiles_per_row,
           (unsigned long long)L.tiles, (unsigned long long)L.groups, (unsigned long long)L.off_sum,
           (unsigned long long)L.off_base, (unsigned long long)L.off_partial, (unsigned long long)L.bytes);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4)
        return one(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    unsigned long long f, r, c;
    while (scanf("%llu %llu %llu", &f, &r, &c) == 3) {
        const int rc = one(f, r, c);
        if (rc) return rc;
    }
    return 0;
}
