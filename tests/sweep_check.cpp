// sweep_check.cpp -- walks what csrc/mh_sweep_layout.hpp decides for mhq_gram_clips and mhq_xty_clips (the argument rules,
// the runs of the ranges, the items and the capped grids) as a plain host program: no HIP, no Python, so that it can be
// built with -fsanitize=address,undefined (tests/test_host_sweep.py).  Reads lines from stdin; device pointers are plain
// numbers (0 = NULL; nothing is read through them), the host arrays follow every line: `listed_r` ranges as pairs and
// `listed_c` clips, in heap blocks of exactly that size (has_r / has_c = 0 passes NULL instead):
//   gram x x_row_stride rows cols lags gram sums n_ranges n_clips has_r has_c listed_r listed_c  a b a b ...  q q ...
//   xty x x_row_stride rows cols lags lead y y_row_stride k out scratch scratch_bytes n_ranges n_clips has_r has_c
//       listed_r listed_c  a b ...  q ...
//   scratch rows cols lags k n_ranges n_clips bytes_ptr
//     -> "ok" (scratch: "ok <bytes>"), or "error <code> <message>"
//   layout x x_row_stride rows cols lags lead k n_ranges n_clips  a b ...  q ...       (arguments that pass both checks)
//     -> gram_runs gram_items gram_grid xty_runs xty_items xty_grid elements sum_grid scratch_bytes
//        after checking what the kernels rely on: every (range, run, clip, d, tile) has one owner, d = 0 only the tiles on
//        or above the diagonal; the runs of a range start at multiples of the run length from its own start, never cross
//        its end, never exceed kGramRunCols / kXtyRun and cover it; the capped grids reach every item once; no byte before
//        column ranges[0] - (lags-1) or at or after column cols of a row is addressed, no float of y at or after cols; the
//        runs of mhq_xty_clips are those of mhw_xty on the range alone; scratch_bytes covers what k_xty_clips writes and
//        k_xty_clips_sum reads.  What is too large to enumerate is sampled at both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mh_sweep_layout.hpp"

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

// the host arrays of a line, in heap blocks of exactly the listed size: a read past them is ASan's to report
struct Host {
    std::unique_ptr<uint64_t[]> r;
    std::unique_ptr<uint32_t[]> c;
    int take(const std::vector<ull> &v, size_t at, ull listed_r, ull listed_c)
    {
        CHECK(v.size() == at + 2 * listed_r + listed_c);
        r.reset(new uint64_t[2 * listed_r]);
        c.reset(new uint32_t[listed_c]);
        for (ull i = 0; i < 2 * listed_r; ++i) r[i] = v[at + i];
        for (ull i = 0; i < listed_c; ++i) c[i] = (uint32_t)v[at + 2 * listed_r + i];
        return 0;
    }
};

static int check_gram(const std::vector<ull> &v)
{
    CHECK(v.size() >= 13);
    Host h;
    if (int rc = h.take(v, 13, v[11], v[12])) return rc;
    const mh::GramClipsArgs a = {v[0], v[1], v[2], v[3], v[9] ? h.r.get() : nullptr, (uint32_t)v[7], v[10] ? h.c.get() : nullptr,
                                 (uint32_t)v[8], (uint32_t)v[4], v[5], v[6]};
    mh::Msg m;
    return report(mh::gram_clips_check(m, a), m);
}

static int check_xty(const std::vector<ull> &v)
{
    CHECK(v.size() >= 18);
    Host h;
    if (int rc = h.take(v, 18, v[16], v[17])) return rc;
    const mh::XtyClipsArgs a = {v[0], v[1], v[2], v[3], v[14] ? h.r.get() : nullptr, (uint32_t)v[12], v[15] ? h.c.get() : nullptr,
                                (uint32_t)v[13], (uint32_t)v[4], (uint32_t)v[5], v[6], v[7], (uint32_t)v[8], v[9], v[10], v[11]};
    mh::Msg m;
    return report(mh::xty_clips_check(m, a), m);
}

static int check_scratch(const std::vector<ull> &v)
{
    CHECK(v.size() == 7);
    mh::Msg m;
    const int rc = mh::xty_clips_scratch_check(m, v[0], v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], v[6]);
    if (rc) return report(rc, m);
    printf("ok %llu\n", (ull)mh::xty_clips_scratch_bytes(v[0], v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]));
    return 0;
}

// the items [0, n) as the capped grid of k_gram_clips walks them: every one once
static int gram_grid_walk(ull n, uint32_t grid)
{
    const ull want = n < mh::kSweepMaxBlocks ? n : mh::kSweepMaxBlocks;
    CHECK(grid % mh::kGramXcds == 0 && grid <= mh::kSweepMaxBlocks && grid >= want && grid < want + mh::kGramXcds);
    if (n <= (1u << 22)) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (uint32_t b = 0; b < grid; ++b)
            for (ull i = mh::gram_first_item(b, grid); i < n; i += grid) CHECK(seen[(size_t)i]++ == 0);
        for (ull i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
    } else {  // the first items of the blocks are a permutation of [0, grid): item i belongs to the block that starts at i % grid
        std::vector<uint8_t> first(grid, 0);
        for (uint32_t b = 0; b < grid; ++b) {
            const ull f = mh::gram_first_item(b, grid);
            CHECK(f < grid && first[(size_t)f]++ == 0);
        }
    }
    return 0;
}

static int strided(ull n, ull walkers)
{
    if (n == 0) return 0;
    CHECK(walkers >= 1 && walkers <= n);
    if (n <= (1u << 22)) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (ull b = 0; b < walkers; ++b)
            for (ull i = b; i < n; i += walkers) CHECK(seen[(size_t)i]++ == 0);
        for (ull i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
    }
    return 0;
}

// one item of k_gram_clips: where it lies and what it addresses
static int walk_gram_item(const mh::GramClipsArgs &a, const mh::GramClipsLayout &L, ull item, std::vector<uint8_t> *seen)
{
    const mh::SweepRanges &R = L.ranges;
    const mh::GramClipsItem it = mh::gram_clips_owner(R, a.n_clips, L.nt, L.tiles0, L.tiles1, L.dt, item);
    CHECK(it.r < a.n_ranges && it.n < a.n_clips && it.d < a.lags && it.ti < L.nt && it.tj < L.nt);
    CHECK(it.d != 0 || it.tj >= it.ti);
    CHECK(R.first[it.r] == a.ranges[2 * it.r] && R.last[it.r] == a.ranges[2 * it.r + 1] && L.clips.q[it.n] == a.clips[it.n]);
    CHECK(it.k0 < it.k1 && it.k0 >= R.first[it.r] && it.k1 <= R.last[it.r]);
    CHECK(it.k1 - it.k0 <= mh::kGramRunCols && (it.k0 - R.first[it.r]) % mh::kGramRunCols == 0);
    CHECK(it.k1 == R.last[it.r] || it.k1 - it.k0 == mh::kGramRunCols);
    const ull run = R.run_first[it.r] + (it.k0 - R.first[it.r]) / mh::kGramRunCols;
    CHECK(run < R.run_first[it.r + 1]);
    // the bytes: the a rows at [k0, k1), the b rows at [k0 - d, k1 - d); the last row is the farthest
    CHECK(it.k0 >= it.d && it.k0 - it.d >= a.ranges[0] - (a.lags - 1) && it.k1 <= a.cols);
    const ull stride = a.rows > 1 ? a.x_row_stride : 0;
    const ull lo = a.x + 0 * stride + it.k0 - it.d, hi = a.x + (a.rows - 1) * stride + it.k1;
    CHECK(lo >= a.x + a.ranges[0] - (a.lags - 1) && hi <= a.x + (a.rows - 1) * stride + a.cols);
    if (seen) {
        const ull cell = (((run * a.n_clips + it.n) * a.lags + it.d) * L.nt + it.ti) * L.nt + it.tj;
        CHECK(cell < seen->size() && (*seen)[(size_t)cell]++ == 0);
    }
    return 0;
}

static int layout(const std::vector<ull> &v)
{
    CHECK(v.size() >= 9);
    const ull x = v[0], xs = v[1], rows = v[2], cols = v[3];
    const uint32_t lags = (uint32_t)v[4], lead = (uint32_t)v[5], k = (uint32_t)v[6], nr = (uint32_t)v[7], nc = (uint32_t)v[8];
    Host h;
    if (int rc = h.take(v, 9, nr, nc)) return rc;
    const ull far = 1ull << 62;
    mh::Msg m;
    // ---- mhq_gram_clips
    const mh::GramClipsArgs a = {x, xs, rows, cols, h.r.get(), nr, h.c.get(), nc, lags, far, far + (1ull << 60)};
    CHECK(mh::gram_clips_check(m, a) == MH_OK);
    mh::GramClipsLayout L;
    mh::gram_clips_layout(a, &L);
    ull runs = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        CHECK(L.ranges.run_first[r] == runs);
        runs += (h.r[2 * r + 1] - h.r[2 * r] + mh::kGramRunCols - 1) / mh::kGramRunCols;
    }
    for (uint32_t r = nr; r <= mh::kSweepMaxRanges; ++r) CHECK(L.ranges.run_first[r] == runs);
    CHECK(L.runs == runs && L.nt == (rows + mh::kGramTile - 1) / mh::kGramTile);
    CHECK(L.tiles0 == (ull)L.nt * (L.nt + 1) / 2 && L.tiles1 == (ull)L.nt * L.nt && L.dt == L.tiles0 + (lags - 1) * L.tiles1);
    CHECK(L.items == runs * nc * L.dt && (runs == 0) == (L.grid == 0));
    if (L.items) {
        if (int rc = gram_grid_walk(L.items, L.grid)) return rc;
        if (L.items <= (1u << 21) && runs * nc * lags * L.nt * L.nt <= (1u << 24)) {
            std::vector<uint8_t> seen((size_t)(runs * nc * lags * L.nt * L.nt), 0);
            for (ull i = 0; i < L.items; ++i)
                if (int rc = walk_gram_item(a, L, i, &seen)) return rc;
            for (ull run = 0; run < runs; ++run)
                for (uint32_t n = 0; n < nc; ++n)
                    for (uint32_t d = 0; d < lags; ++d)
                        for (uint32_t ti = 0; ti < L.nt; ++ti)
                            for (uint32_t tj = 0; tj < L.nt; ++tj)
                                CHECK(seen[(size_t)((((run * nc + n) * lags + d) * L.nt + ti) * L.nt + tj)] == (d == 0 && tj < ti ? 0 : 1));
        } else {
            for (ull i = 0; i < 4096 && i < L.items; ++i) {
                if (int rc = walk_gram_item(a, L, i, nullptr)) return rc;
                if (int rc = walk_gram_item(a, L, L.items - 1 - i, nullptr)) return rc;
            }
        }
    }
    // ---- mhq_xty_clips
    const ull need = mh::xty_clips_scratch_bytes(rows, cols, lags, k, nr, nc);
    const mh::XtyClipsArgs b = {x, xs, rows, cols, h.r.get(), nr, h.c.get(), nc, lags, lead, 1ull << 40, 4 * cols, k, far, far + (1ull << 60), need};
    CHECK(mh::xty_clips_check(m, b) == MH_OK);
    mh::XtyClipsArgs less = b;
    less.scratch_bytes = need - 1;
    CHECK(mh::xty_clips_check(m, less) == MH_ERR_ARG);
    m.text[0] = 0;
    mh::XtyClipsLayout X;
    mh::xty_clips_layout(b, &X);
    ull xruns = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        const ull len = h.r[2 * r + 1] - h.r[2 * r];
        CHECK(X.ranges.run_first[r] == xruns);
        if (len) {  // the runs of mhw_xty on this range alone
            mh::XtyLayout W;
            mh::xty_layout(rows, len, lags, k, &W);
            CHECK(W.runs == (len + mh::kXtyRun - 1) / mh::kXtyRun && W.per_item == lags * k);
            xruns += W.runs;
        }
    }
    CHECK(X.runs == xruns && X.ranges.run_first[mh::kSweepMaxRanges] == xruns);
    CHECK(X.items == xruns * nc * rows && X.per_item == lags * k && X.elements == (ull)nr * nc * rows * lags * k);
    CHECK(X.grid == (X.items < mh::kSweepXtyMaxBlocks ? X.items : mh::kSweepXtyMaxBlocks));
    CHECK(X.sum_grid >= 1 && X.sum_grid <= mh::kSweepXtyMaxBlocks);
    CHECK(X.items * X.per_item * 8 <= need);  // every partial sum that is written, and every one that is read, lies inside
    if (int rc = strided(X.items, X.grid)) return rc;
    const bool all = X.items <= (1u << 21);
    std::vector<uint8_t> xseen(all ? (size_t)X.items : 0, 0);
    for (ull s = 0; s < (all ? X.items : 8192); ++s) {
        const ull item = all ? s : (s < 4096 ? s : X.items - 1 - (s - 4096));
        const mh::XtyClipsItem it = mh::xty_clips_owner(X.ranges, nc, (uint32_t)rows, item);
        CHECK(it.r < nr && it.n < nc && it.c < rows);
        const ull first = h.r[2 * it.r], last = h.r[2 * it.r + 1], len = last - first;
        CHECK(it.c0 < it.c1 && it.c1 <= len && it.c1 - it.c0 <= mh::kXtyRun && it.c0 % mh::kXtyRun == 0);
        CHECK(it.c1 == len || it.c1 - it.c0 == mh::kXtyRun);
        uint64_t w0, w1;  // mhw_xty's own cut of the same run
        mh::xty_run_cols(it.c0 / mh::kXtyRun, len, &w0, &w1);
        CHECK(w0 == it.c0 && w1 == it.c1);
        // x: the columns first - (lags-1) + t + off, off 0..lags-1; y: the floats first + lead + t
        CHECK(first - (lags - 1) + it.c0 >= h.r[0] - (lags - 1) && first + it.c1 - 1 < cols - lead && first + lead + it.c1 - 1 < cols);
        const ull run = X.ranges.run_first[it.r] + it.c0 / mh::kXtyRun;
        CHECK(((run * nc + it.n) * rows + it.c) == item && (item + 1) * X.per_item * 8 <= need);
        if (all) CHECK(xseen[(size_t)item]++ == 0);
    }
    printf("%llu %llu %u %llu %llu %u %llu %u %llu\n", (ull)L.runs, (ull)L.items, L.grid, (ull)X.runs, (ull)X.items, X.grid, (ull)X.elements,
           X.sum_grid, need);
    return 0;
}

int main()
{
    static char line[1 << 14];
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
        if (wl == 4 && !strncmp(s, "gram", 4))
            rc = check_gram(v);
        else if (wl == 3 && !strncmp(s, "xty", 3))
            rc = check_xty(v);
        else if (wl == 7 && !strncmp(s, "scratch", 7))
            rc = check_scratch(v);
        else if (wl == 6 && !strncmp(s, "layout", 6))
            rc = layout(v);
        else
            return 3;
        if (rc) return rc;
    }
    return 0;
}
