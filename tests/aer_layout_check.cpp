// aer_layout_check.cpp -- prints the tile rule and the scratch layout of mhi_aer_to_csr (csrc/mh_aer_layout.hpp, the
// arithmetic the library runs before it launches) as a plain host program: no HIP, no Python, so that it can be built
// with -fsanitize=address,undefined (tests/test_host_aer.py).  Reads "n C" pairs from stdin -- or takes one pair as
// arguments -- and prints per pair either "error <code>" or
//     run waves tile nbits lds_bytes rows groups rows_alloc groups_alloc off_matrix off_partial off_drop bytes
// after checking what the kernels rely on.
#include <cstdio>
#include <cstdlib>

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
    printf("%u %u %u %u %u %llu %llu %llu %llu %llu %llu %llu %llu\n", L.run, L.waves, L.tile, L.nbits, L.lds_bytes,
           (unsigned long long)L.rows, (unsigned long long)L.groups, (unsigned long long)L.rows_alloc,
           (unsigned long long)L.groups_alloc, (unsigned long long)L.off_matrix, (unsigned long long)L.off_partial,
           (unsigned long long)L.off_drop, (unsigned long long)L.bytes);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return one(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10));
    unsigned long long n, c;
    while (scanf("%llu %llu", &n, &c) == 2) {
        const int rc = one(n, c);
        if (rc) return rc;
    }
    return 0;
}
