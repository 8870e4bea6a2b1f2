// excess_layout_check.cpp -- prints the piece rule and the scratch layout of mhi_excess_count / mhi_excess_emit
// (csrc/mh_excess_layout.hpp, the arithmetic the library runs before it launches) as a plain host program: no HIP, no
// Python, so that it can be built with -fsanitize=address,undefined (tests/test_host_excess.py).  Reads "form rows cols"
// triples from stdin -- or takes one as arguments -- and prints per triple either "error <code>" or
//     tile tile_t strip channels length per_channel pieces groups strips off_sum off_base off_partial bytes waves grid
//     grid_scan
// after checking what the kernels rely on.  A fourth kind of line, "apply start stop r lead", prints apply_elements.
// A line that starts with "check" asks for the verdict of an entry point's argument rules, every argument of the ABI
// but the stream as a number (pointers too, 0 = NULL; nothing is read through them), and prints "ok" -- "ok <elements>
// <runs>" for apply -- or "error <code> <message>":
//   check scratch form rows cols bytes
//   check count form in row_off lo hi rows cols threshold exc_off total scratch scratch_bytes
//   check emit form in row_off lo hi rows cols threshold pos val capacity over scratch scratch_bytes
//   check apply pos val n_entries first last n_rows start stop r lead out out_bits row_stride col_stride
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mh_excess_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

static int one(unsigned long long form, unsigned long long rows, unsigned long long cols)
{
    mh::ExcessLayout L;
    const int rc = form > 0xFFFFFFFFull ? -1 : mh::excess_layout((uint32_t)form, rows, cols, &L);
    if (rc) {
        printf("error %d\n", rc);
        return 0;
    }
    CHECK(L.pieces >= 1 && L.pieces <= mh::kExcessMaxPieces);
    CHECK(L.length < mh::kExcessMaxLen && L.channels >= 1 && L.per_channel >= 1);          // a position is 32-bit
    CHECK((unsigned __int128)L.channels * L.per_channel == L.pieces);
    const unsigned long long piece = form == mh::kExcessRows ? mh::kUnbinTile : mh::kExcessTileT;
    CHECK((unsigned __int128)L.per_channel * piece >= L.length);                            // the pieces cover a channel
    CHECK((unsigned __int128)(L.per_channel - 1) * piece < L.length);                       // ... exactly
    if (form == mh::kExcessRows) {
        CHECK(L.channels == rows && L.length == cols && L.strips == 0);
        CHECK((L.pieces + mh::kExcessWaves - 1) / mh::kExcessWaves <= 0x7FFFFFFFull);      // a grid's first dimension
    } else {
        CHECK(L.channels == cols && L.length == rows);
        CHECK(L.strips * mh::kExcessStrip >= cols && (L.strips - 1) * mh::kExcessStrip < cols);
        CHECK((unsigned __int128)L.strips * L.per_channel <= L.pieces);                     // never more waves than cells
        CHECK((L.strips * L.per_channel + mh::kExcessWaves - 1) / mh::kExcessWaves <= 0x7FFFFFFFull);
    }
    CHECK(L.groups >= 1 && L.groups * mh::kUnbinGroup >= L.pieces && (L.groups - 1) * mh::kUnbinGroup < L.pieces);
    CHECK(L.groups <= 0x7FFFFFFFull);
    CHECK(L.off_sum % 16 == 0 && L.off_base % 16 == 0 && L.off_partial % 16 == 0 && L.bytes % 16 == 0 && L.bytes);
    CHECK(L.off_sum + L.pieces * 4 <= L.off_base);                                          // sections in order, disjoint
    CHECK(L.off_base + L.pieces * 8 <= L.off_partial);
    CHECK(L.off_partial + (L.groups + 1) * 8 <= L.bytes);                                   // + the total
    CHECK(L.waves == L.strips * L.per_channel && L.grid_scan == L.groups);
    const unsigned long long owners = form == mh::kExcessRows ? L.pieces : L.waves;           // the grid holds every owner
    CHECK((unsigned long long)L.grid * mh::kExcessWaves >= owners && (unsigned long long)(L.grid - 1) * mh::kExcessWaves < owners);
    printf("%u %u %u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %u\n", mh::kUnbinTile, mh::kExcessTileT, mh::kExcessStrip,
           (unsigned long long)L.channels, (unsigned long long)L.length, (unsigned long long)L.per_channel,
           (unsigned long long)L.pieces, (unsigned long long)L.groups, (unsigned long long)L.strips,
           (unsigned long long)L.off_sum, (unsigned long long)L.off_base, (unsigned long long)L.off_partial,
           (unsigned long long)L.bytes, (unsigned long long)L.waves, L.grid, L.grid_scan);
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
    unsigned long long v[14];
    if (scanf("%15s", what) != 1) return 3;
    const bool is_apply = !strcmp(what, "apply");
    const int n = !strcmp(what, "scratch") ? 4 : !strcmp(what, "count") ? 12 : !strcmp(what, "emit") || is_apply ? 14 : 0;
    if (!n) return 3;
    for (int i = 0; i < n; ++i)
        if (scanf("%llu", &v[i]) != 1) return 3;
    mh::Msg m;
    if (is_apply) {
        const mh::ApplyArgs a = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], (uint32_t)v[11], v[12], v[13]};
        mh::ApplyLayout A;
        const int rc = mh::excess_apply_check(m, a, &A);
        if (rc) return verdict(rc, m);
        CHECK(m.text[0] == 0);
        const bool nothing = a.n_rows == 0 || a.n_entries == 0 || a.start == a.stop;
        CHECK(nothing ? A.elements == 0 && A.runs == 0 : A.elements >= 1 && A.runs == (A.elements + mh::kApplyRun - 1) / mh::kApplyRun);
        CHECK(nothing || A.elements == mh::apply_elements(a.start, a.stop, a.r, a.lead));
        printf("ok %llu %llu\n", (unsigned long long)A.elements, (unsigned long long)A.runs);
        return 0;
    }
    mh::ExcessLayout L;
    if (n == 4) return verdict(mh::excess_scratch_check(m, (uint32_t)v[0], v[1], v[2], v[3], &L), m);
    const mh::ExcessArgs s = {(uint32_t)v[0], v[1], v[2], v[3], v[4], v[5], v[6], (uint32_t)v[7], v[n - 2], v[n - 1]};
    if (n == 12) return verdict(mh::excess_count_check(m, mh::ExcessCountArgs{s, v[8], v[9]}, &L), m);
    return verdict(mh::excess_emit_check(m, mh::ExcessEmitArgs{s, v[8], v[9], v[10], v[11]}, &L), m);
}

static int apply(unsigned long long start, unsigned long long stop, unsigned long long r, unsigned long long lead)
{
    CHECK(start <= stop && stop <= mh::kExcessMaxLen && r >= 1 && r <= mh::kExcessMaxLen && lead < mh::kExcessMaxLen);
    const uint64_t n = mh::apply_elements(start, stop, r, lead);
    CHECK((unsigned __int128)n * r >= stop - start + lead);
    CHECK(n == 0 || (unsigned __int128)(n - 1) * r < stop - start + lead);
    printf("%llu\n", (unsigned long long)n);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4)
        return one(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    char word[16];
    while (scanf("%15s", word) == 1) {
        unsigned long long a, b, c, d;
        int rc;
        if (!strcmp(word, "apply")) {
            if (scanf("%llu %llu %llu %llu", &a, &b, &c, &d) != 4) return 3;
            rc = apply(a, b, c, d);
        } else if (!strcmp(word, "check")) {
            rc = check();
        } else {
            a = strtoull(word, nullptr, 10);
            if (scanf("%llu %llu", &b, &c) != 2) return 3;
            rc = one(a, b, c);
        }
        if (rc) return rc;
    }
    return 0;
}
