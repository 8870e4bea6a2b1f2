// train_check.cpp -- walks what csrc/mh_train_layout.hpp decides for mht_loss_grad (the argument rules, the clamp of the window
// indices, the scratch, the tiles and the capped grids) as a plain host program: no HIP, no Python, so that it can be built
// with -fsanitize=address,undefined (tests/test_host_train.py).  Reads lines from stdin:
//   loss_grad x x_row_stride rows cols clip mean inv idx batch lags units k lead wx bias wh wd bd y y_row_stride scale
//             scratch out loss dwx dbias dwh dwd dbd
//         (pointers as plain numbers, 0 = NULL; nothing is read through them; scale as a decimal, "nan" or "inf")
//     -> "ok", or "error <code> <message>"
//   layout rows batch lags units k                     (a shape that passes the checks)
//     -> R gtiles in_items in_grid tiles rec_grid ksteps ublocks ctiles wx_items wh_items sum_items grad_items grad_grid
//        scratch_bytes
//        after checking what the kernels rely on: the parts of the scratch lie back to back inside scratch_bytes; the clamp
//        keeps every bin of a window and its target inside the recording for any idx; k_train_inproj's items store every
//        (row, pre-activation) of act once and nothing else; the window tiles partition the minibatch and their rows lie
//        inside the tapes; k_train_forward's dispatch matches windows_layout; k_train_backward's two halves name every
//        pre-activation once, its LDS reads stay inside the image, its threads name every (unit, window) once and the image
//        fits the LDS of a workgroup; k_train_wgrad's items store every entry of dwx (first and last tiles when large), dwh,
//        dbias, dwd and dbd once; every grid is under its cap and the stride loops reach every item once.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mh_train_layout.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

typedef unsigned long long ull;

static int check_loss_grad(const std::vector<ull> &v, float scale)
{
    CHECK(v.size() == 29);
    mh::LossGradArgs a;
    a.x = v[0], a.x_row_stride = v[1], a.rows = v[2], a.cols = v[3], a.clip = (uint32_t)v[4], a.mean = v[5], a.inv = v[6], a.idx = v[7];
    a.batch = (uint32_t)v[8], a.lags = (uint32_t)v[9], a.units = (uint32_t)v[10], a.k = (uint32_t)v[11], a.lead = v[12];
    a.wx = v[13], a.bias = v[14], a.wh = v[15], a.wd = v[16], a.bd = v[17], a.y = v[18], a.y_row_stride = v[19], a.scale = scale;
    a.scratch = v[21], a.out = v[22], a.loss = v[23], a.dwx = v[24], a.dbias = v[25], a.dwh = v[26], a.dwd = v[27], a.dbd = v[28];
    mh::Msg m;
    const int rc = mh::loss_grad_check(m, a);
    CHECK((rc == MH_OK) == (m.text[0] == 0));
    CHECK(rc == MH_OK || rc == MH_ERR_ARG);
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

// the indices [0, n) that `walkers` walkers reach, walker b taking b, b + walkers, ...: all of them once
static int strided(ull n, ull walkers)
{
    CHECK(walkers >= 1 && n <= (1u << 22));
    std::vector<uint8_t> seen((size_t)n, 0);
    for (ull b = 0; b < walkers && b < n; ++b)
        for (ull i = b; i < n; i += walkers) CHECK(seen[(size_t)i]++ == 0);
    for (ull i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
    return 0;
}

static int layout(const std::vector<ull> &v)
{
    CHECK(v.size() == 5);
    const ull rows = v[0];
    const uint32_t batch = (uint32_t)v[1], lags = (uint32_t)v[2], units = (uint32_t)v[3], k = (uint32_t)v[4];
    const ull U = units, G = 4 * U, cols = 100000, lead = 3;
    {   // the shape passes, with stand-in pointers far from each other
        mh::LossGradArgs a = {1ull << 32, cols, rows, cols, 255, 1ull << 50, 2ull << 50, 3ull << 50, batch, lags, units, k, lead, 4ull << 50,
                              5ull << 50, 6ull << 50, 7ull << 50, 8ull << 50, 9ull << 50, 4 * cols, 0.5f, 10ull << 50, 11ull << 50,
                              12ull << 50, 13ull << 50, 14ull << 50, 15ull << 50, 16ull << 50, 17ull << 50};
        mh::Msg m;
        CHECK(mh::loss_grad_check(m, a) == MH_OK);
    }
    mh::TrainLayout L;
    mh::loss_grad_layout(rows, batch, lags, units, k, &L);
    const ull R = (ull)batch * lags;
    CHECK(L.R == R && R * G < (1ull << 32));   // k_train_forward's 32-bit offsets into the tapes
    // the scratch: five parts back to back
    const mh::TrainScratch s = mh::train_scratch(batch, lags, units);
    CHECK(s.act == 0 && s.dz == s.act + R * G && s.c == s.dz + R * G && s.h == s.c + R * U && s.dout == s.h + R * U);
    CHECK(s.floats == s.dout + (ull)batch * mh::kTrainDoutPitch && mh::scratch_bytes(batch, lags, units) == 4 * s.floats);
    CHECK(mh::kTrainDoutPitch >= mh::kLstmMaxK && k <= mh::kLstmMaxK);
    // the clamp: any idx gives a window and a target inside the recording
    const ull shapes[3][2] = {{(ull)lags + lead, lead}, {cols, lead}, {(ull)lags, 0}};
    for (const auto &sh : shapes) {
        const int64_t big = INT64_MAX, ids[10] = {INT64_MIN, -1, 0, (int64_t)lags - 2, (int64_t)lags - 1, (int64_t)(sh[0] - 1 - sh[1]),
                                                 (int64_t)(sh[0] - sh[1]), (int64_t)sh[0], big - 1, big};
        for (int64_t id : ids) {
            const ull t = mh::train_bin(id, lags, sh[0], sh[1]);
            CHECK(t + 1 >= lags && t + sh[1] < sh[0]);
            if (id >= (int64_t)lags - 1 && id <= (int64_t)(sh[0] - 1 - sh[1])) CHECK(t == (ull)id);
        }
    }
    // k_train_inproj: items of (128 rows, 32 pre-activations)
    CHECK(L.gtiles * mh::kGradTile >= G && (L.gtiles - 1) * mh::kGradTile < G);
    const ull rblocks = (R + mh::kTrainInRows - 1) / mh::kTrainInRows;
    CHECK(L.in_items == rblocks * L.gtiles && mh::kTrainInRows == 32 * (mh::kTrainInThreads / 64));
    CHECK(L.in_grid >= 1 && L.in_grid == (L.in_items < mh::kTrainInMaxBlocks ? L.in_items : mh::kTrainInMaxBlocks));
    {
        const ull rbs[3] = {0, rblocks > 1 ? 1ull : 0ull, rblocks - 1};
        const uint32_t gts[2] = {0, L.gtiles - 1};
        for (ull rb : rbs)
            for (uint32_t gt : gts) {
                std::vector<uint8_t> seen(mh::kTrainInRows * mh::kGradTile, 0);
                for (uint32_t tid = 0; tid < mh::kTrainInThreads; ++tid) {
                    const uint32_t lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
                    const ull g = (ull)gt * mh::kGradTile + col;
                    for (uint32_t i = 0; i < 16; ++i) {
                        const uint32_t w = wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                        const ull r = rb * mh::kTrainInRows + w;
                        CHECK(w < mh::kTrainInRows && seen[w * mh::kGradTile + col]++ == 0);
                        if (r < R && g < G) CHECK(s.act + r * G + g < s.dz);
                    }
                }
                for (uint8_t e : seen) CHECK(e == 1);
            }
        if (int rc = strided(L.in_items, L.in_grid)) return rc;
    }
    // the recurrences: tiles of 32 windows
    CHECK((ull)L.tiles * mh::kWinTile >= batch && (ull)(L.tiles - 1) * mh::kWinTile < batch);
    CHECK(L.rec_grid >= 1 && L.rec_grid == (L.tiles < mh::kTrainMaxTiles ? L.tiles : mh::kTrainMaxTiles));
    for (uint32_t tile : {0u, L.tiles - 1})
        for (uint32_t n = 0; n < mh::kWinTile; ++n) {
            const ull b = (ull)tile * mh::kWinTile + n;
            if (b >= batch) continue;
            for (uint32_t st = 0; st < lags; ++st) {
                const ull r = b * lags + st;
                CHECK(r < R && s.c + (r + 1) * U <= s.h && s.h + (r + 1) * U <= s.dout && s.dz + (r + 1) * G <= s.c);
            }
            CHECK(s.dout + (b + 1) * mh::kTrainDoutPitch <= s.floats);
        }
    mh::WinLayout W;
    mh::windows_layout(lags, lags, units, &W);
    CHECK(L.ksteps == W.ksteps && (W.per_wave == 1) == (L.ksteps <= 32) && L.ksteps % mh::kWinKGroup == 0 && L.ksteps <= 64);
    CHECK(mh::kWinTile * mh::kLstmMaxK <= mh::kWinThreads);      // the dense layer: one thread per (output, window)
    if (int rc = strided(L.tiles, L.rec_grid)) return rc;
    // k_train_backward<UB>
    const uint32_t UB = L.ublocks, KS = mh::kBwdKSteps * UB;
    CHECK(UB >= 1 && UB <= 4 && 32 * UB >= units && 32 * (UB - 1) < units && KS >= units);
    CHECK(mh::kBwdThreads == 512 && mh::kBwdThreads / 16 == mh::kWinTile);
    CHECK((4ull * KS + 2 * 32 * UB) * mh::kBwdPitch * 4 <= 160 * 1024);   // dz, dh and dc of a tile: the LDS of a workgroup
    {
        std::vector<uint8_t> seen((size_t)G, 0);
        for (uint32_t rh = 0; rh < 2; ++rh)
            for (uint32_t ks = 0; ks < KS; ++ks)
                for (uint32_t hh = 0; hh < 2; ++hh) {
                    const uint32_t g = rh * 2 * units + 2 * ks + hh;   // the row of the LDS image a lane reads
                    CHECK(g < 4 * KS);
                    if (ks < units) CHECK(g < G && seen[g]++ == 0);    // past units the A fragment and the B value are zero
                }
        for (uint8_t e : seen) CHECK(e == 1);
        std::vector<uint8_t> el((size_t)(32 * UB) * 32, 0);
        for (uint32_t tid = 0; tid < mh::kBwdThreads; ++tid)
            for (uint32_t vv = tid & 15; vv < units; vv += 16) CHECK((tid >> 4) < 32 && vv < 32 * UB && el[vv * 32 + (tid >> 4)]++ == 0);
        for (uint32_t vv = 0; vv < units; ++vv)
            for (uint32_t n = 0; n < 32; ++n) CHECK(el[vv * 32 + n] == 1);
        for (uint32_t mb = 0; mb < UB; ++mb)
            for (uint32_t hh = 0; hh < 2; ++hh)
                for (uint32_t r = 0; r < 16; ++r) CHECK(32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hh < 32 * UB);
    }
    // k_train_wgrad: the items
    CHECK((ull)L.ctiles * mh::kGradTile >= rows && (ull)(L.ctiles - 1) * mh::kGradTile < rows);
    CHECK(L.wx_items == (ull)L.gtiles * L.ctiles && L.wh_items == L.gtiles * UB);
    const uint32_t sums = 4 * units + k * units + k;
    CHECK(L.sum_items * mh::kGradThreads >= sums && (L.sum_items - 1) * mh::kGradThreads < sums);
    CHECK(L.grad_items == L.wx_items + L.wh_items + L.sum_items);
    CHECK(L.grad_grid >= 1 && L.grad_grid == (L.grad_items < mh::kGradMaxBlocks ? L.grad_items : mh::kGradMaxBlocks));
    for (int which = 0; which < 2; ++which) {
        const ull nmax = which ? U : rows, ntiles = which ? UB : L.ctiles, items = which ? L.wh_items : L.wx_items;
        std::vector<uint8_t> seen;
        const bool all = G * nmax <= (1u << 22);
        if (all) seen.assign((size_t)(G * nmax), 0);
        for (ull it = 0; it < items; ++it) {
            if (!all && it >= 2 * ntiles && it + 2 * ntiles < items) continue;
            const ull gt = it / ntiles, nt = it - gt * ntiles;
            CHECK(gt < L.gtiles);
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint32_t i = 0; i < 16; ++i) {
                    const ull gg = gt * mh::kGradTile + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), nn = nt * mh::kGradTile + (lane & 31);
                    if (gg < G && nn < nmax) {
                        CHECK((gg * nmax + nn + 1) * 4 <= 4 * G * nmax);
                        if (all) CHECK(seen[(size_t)(gg * nmax + nn)]++ == 0);
                    }
                }
        }
        for (uint8_t e : seen) CHECK(e == 1);
    }
    {
        std::vector<uint8_t> seen(sums, 0);
        for (uint32_t it = 0; it < L.sum_items; ++it)
            for (uint32_t lane = 0; lane < mh::kGradThreads; ++lane) {
                const uint32_t o = it * mh::kGradThreads + lane;
                if (o < sums) CHECK(seen[o]++ == 0);
            }
        for (uint8_t e : seen) CHECK(e == 1);
    }
    if (int rc = strided(L.grad_items, L.grad_grid)) return rc;
    printf("%llu %u %llu %u %u %u %u %u %u %llu %u %u %llu %u %llu\n", (ull)L.R, L.gtiles, (ull)L.in_items, L.in_grid, L.tiles, L.rec_grid, L.ksteps,
           L.ublocks, L.ctiles, (ull)L.wx_items, L.wh_items, L.sum_items, (ull)L.grad_items, L.grad_grid, (ull)mh::scratch_bytes(batch, lags, units));
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
        float scale = 0.f;
        for (char *q = end;;) {
            char *nx, *nd;
            const double d = strtod(q, &nd);
            if (nd == q) break;
            const ull x = strtoull(q, &nx, 10);
            if (v.size() == 20) scale = (float)d;   // the one argument that is no integer
            v.push_back(nx == q ? 0 : x);
            q = nd;
        }
        int rc;
        if (wl == 9 && !strncmp(s, "loss_grad", 9))
            rc = check_loss_grad(v, scale);
        else if (wl == 6 && !strncmp(s, "layout", 6))
            rc = layout(v);
        else
            return 3;
        if (rc) return rc;
    }
    return 0;
}
