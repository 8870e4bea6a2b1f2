// planner_check.cpp -- runs the product's host planner (csrc/mh_planner.hpp, the code mh_plan_create
// executes before its uploads) as a plain host program, so that it can be built with
// -fsanitize=address,undefined.  Reads cases from stdin:
//     C S h mode window K seg_chunks  len[0..C)  sclv[0..K*S)
// checks the planner's internal invariants and prints, per case, the directory for the test to
// compare with the CPU oracle's:  "nseg cap seg_chunks wave_tasks" then four lines ch / first / n / off.
// With --cells (tests/kernel_cells.py) each case carries input_bits after seg_chunks,
//     C S h mode window K seg_chunks input_bits  len[0..C)  sclv[0..K*S)
// and the program prints only where the kernel selection (csrc/mh_select.hpp, what mh_plan_create resolves) lands, fields
// separated by '|':  "maxlen wave_tasks W", then instance name and dynamic-LDS bytes of the plan's encoder, of its decoder
// (PO = 0 for a byte plan, PO = input_bits for a packed one; "-" and 0 where mh_decode_packed refuses the plan) and, for
// byte plans, of its k_decode_range and k_decode_rebin<..., true> instances.
// With --forms (tests/async_table.py) the same input gives the form of the plan, which decides what each call enqueues:
// "wave_tasks measure_fused fused_calibration tickets_fit cal_tiles head_segments skipped short_channels".
// With --tiles (tests/test_host_misaligned.py) the same input gives what cuts a plan's histogram work:
// "kHistTileBytes kCalDirect window_tiles cal_tiles", then the window tiles' sample counts on one line.
// With --tasks (tests/test_host_big_codec.py) a case in the first format gives "K ntask ntile ncaltile seg_src_stride slot_full",
// one line "G src_off dst_off n_last ch seg0 nseg" per workgroup task, "H ch start n" per window tile and "P ch start n" per
// calibration tile.
// With --worklist (tests/test_host_worklist.py) a case in the first format is followed by a query count and that many
// queries  n_sel sel[0..n_sel) t0 t1 r out_pitch  (r = 0: mh_decode_range's list, else mh_decode_rebin's), built by
// csrc/mh_worklist.hpp as the library builds them.  Output: "D nseg" and the directory's ch / first / n lines, then per
// query "L ntask nwg nfix nfill naux max_fill" + the blob offsets of the workgroup, fix and fill sections + its size,
// and one line per record: T (task fields in struct order, without padding), W task0 ntask ch, X off slot, F off n.
// With --arena (tests/test_planner_sanitized.py) the --cells input gives the device layout of the plan (csrc/mh_plan_arena.hpp,
// what mh_plan_create allocates and uploads): "A tables_bytes scratch_bytes nregions", one line "R name part present off
// bytes elems elem_size" per region (part T or S; elems: what PlanHost and the plan's form say the region holds, counted
// here and not by the header), "K" + the staged 16-byte SCLV rows as words, and "P n" + n lines "ch start n" of the
// staged calibration tiles where the header builds them (a packed plan without planner tiles; n = 0 otherwise).  The
// staged blob is compared with the planner's vectors byte for byte here.
// With --validate (tests/test_host_validate.py) the walk of a stored stream (csrc/mh_validate.hpp, what mh_validate_stream
// and mh_validate_segments run behind their NULL checks).  A case is a plan line in the first format, then
//     n_segments seg_words[0..n_segments)  peak[0..C) enc[0..C)  payload_words <payload>  n_walks <walk>...
// <payload>: the words in decimal ("-" for none), or @FILE, a raw little-endian file of them; <walk>: null n_idx seg_idx[0..n_idx)
// seg_off[0..n_segments), null = 1 passing a NULL payload.  The payload sits in a heap block of EXACTLY payload_words
// words, so a read of one word behind it stops the program.  Output: "S rc message" for the stream walk, then
// "G rc message" per segment walk (rc and message: what the ABI call returns and leaves in mh_last_error).
// With --sweep (tests/test_host_sweep_planner.py) the planner of mh_sweep_create (csrc/mh_sweep_planner.hpp), cases
//     C nh hist_bits[0..nh) len[0..C)
// Output: "error rc" for refused arguments, else "W ni ntiles tables_bytes scratch_bytes", "B" + the C * (ni + 1)
// bounds, "L" + the C * ni slot lengths and one line "T ch slot start n" per tile; sweep_arena's staged blob is compared
// with the vectors here, as --arena does.
// With --geometry (tests/test_host_launch_geometry.py) the capped launch grids of csrc/mh_launch.hpp, one launch per
// line: synth max_len C | rebin max_len C r | fills max_fill per_block nfill | transposed T C tpw | items n |
// compact nseg | bin_events C T period | seg_crc32 n_list | excess_apply1 n_entries n_rows | excess_apply n_rows runs |
// chunk_stride stride bits.  Output per line: the name, the
// grid and the derived kernel arguments, or "name error rc message".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mh_launch.hpp"
#include "mh_plan_arena.hpp"
#include "mh_planner.hpp"
#include "mh_select.hpp"
#include "mh_sweep_planner.hpp"
#include "mh_validate.hpp"
#include "mh_worklist.hpp"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "invariant failed: %s (line %d)\n", #cond, __LINE__); \
            return 2;                                                  \
        }                                                              \
    } while (0)

// The arguments of one plan case from stdin (with_bits: input_bits after seg_chunks).  1: read; 0: end of input; -1: malformed.
struct PlanArgs {
    unsigned C, S, h, mode, window, K, sc, bits = 8;
    std::vector<uint64_t> len, off;
    std::vector<uint8_t> sclv;
};

static int read_plan_args(bool with_bits, PlanArgs &a)
{
    if (scanf("%u %u %u %u %u %u %u", &a.C, &a.S, &a.h, &a.mode, &a.window, &a.K, &a.sc) != 7) return 0;
    a.bits = 8;
    if (with_bits && scanf("%u", &a.bits) != 1) return -1;
    a.len.assign(a.C, 0), a.off.assign(a.C, 0);
    a.sclv.assign((size_t)a.K * a.S, 0);
    uint64_t o = 0;
    for (unsigned c = 0; c < a.C; ++c) {
        unsigned long long v;
        if (scanf("%llu", &v) != 1) return -1;
        a.len[c] = v;
        a.off[c] = o;
        o += (v + 15) & ~15ull;
    }
    for (auto &b : a.sclv) {
        unsigned v;
        if (scanf("%u", &v) != 1) return -1;
        b = (uint8_t)v;
    }
    return 1;
}

// One plan case from stdin -> p.  1: built; 2: the arguments were rejected ("error <code>" printed); 0: end of input;
// -1: a malformed case.
static int read_plan(bool with_bits, mh::PlanHost &p)
{
    PlanArgs a;
    if (const int got = read_plan_args(with_bits, a); got <= 0) return got;
    const char *msg = "";
    uint32_t arg = 0, maxlen = 0;
    const int rc = mh::plan_check_args(a.len.data(), a.C, a.S, a.h, a.mode, a.window, a.sclv.data(), a.K, &maxlen, &msg, &arg);
    if (rc != MH_OK) {
        printf("error %d\n", rc);
        return 2;
    }
    p = mh::PlanHost();
    p.info.C = a.C; p.info.S = a.S; p.info.h = a.h; p.info.mode = a.mode; p.info.window = a.window;
    p.info.K = a.K; p.info.seg_chunks = a.sc; p.info.maxlen = maxlen;
    p.input_bits = a.bits;
    mh::plan_host_build(p, a.off.data(), a.len.data(), a.sclv.data());
    return 1;
}

// --tasks: what the kernels index a long channel by -- the workgroup tasks and the histogram tiles of a plan
static int tasks()
{
    mh::PlanHost p;
    int got;
    while ((got = read_plan(false, p)) > 0) {
        if (got == 2) continue;
        printf("K %zu %zu %zu %llu %llu\n", p.wg_tasks.size(), p.tile_start.size(), p.cal_tile_start.size(),
               (unsigned long long)p.seg_src_stride, (unsigned long long)p.slot_full);
        for (const mh::WgTask &w : p.wg_tasks)
            printf("G %llu %llu %u %u %u %u\n", (unsigned long long)w.src_off, (unsigned long long)w.dst_off, w.n_last, w.ch, w.seg0, w.nseg);
        for (size_t i = 0; i < p.tile_start.size(); ++i) printf("H %u %llu %u\n", p.tile_ch[i], (unsigned long long)p.tile_start[i], p.tile_n[i]);
        for (size_t i = 0; i < p.cal_tile_start.size(); ++i)
            printf("P %u %llu %u\n", p.cal_tile_ch[i], (unsigned long long)p.cal_tile_start[i], p.cal_tile_n[i]);
    }
    return got < 0;
}

static int cells(bool forms, bool tiles = false)
{
    mh::PlanHost p;
    int got;
    while ((got = read_plan(true, p)) > 0) {
        if (got == 2) continue;
        const unsigned C = p.info.C, h = p.info.h, window = p.info.window;
        const std::vector<uint64_t> &len = p.ch_len;
        if (tiles) {
            printf("%u %llu %zu %zu\n", mh::kHistTileBytes, (unsigned long long)mh::kCalDirect, p.tile_ch.size(), p.cal_tile_ch.size());
            for (uint32_t n : p.tile_n) printf("%u ", n);
            printf("\n");
            continue;
        }
        if (forms) {
            unsigned heads = 0, shorter = 0;
            for (unsigned c = 0; c < C; ++c) {
                heads += mh::head_samples(p.w0[c], p.w1[c], window) ? 1u : 0u;
                shorter += len[c] < ((uint64_t)1 << h) ? 1u : 0u;
            }
            printf("%d %d %d %d %zu %u %llu %u\n", (int)p.use_wave_tasks, (int)p.measure_fused, (int)p.fused_calibration,
                   (int)p.tickets_fit, p.cal_tile_ch.size(), heads, (unsigned long long)p.info.n_skipped, shorter);
            continue;
        }
        const uint32_t L = p.info.maxlen, bits = p.input_bits;
        const bool wave = p.use_wave_tasks;
        const mh::EncPick e = mh::enc_pick(L, p.info.S, bits, wave);
        const size_t ntask = wave ? p.wave_tasks.size() : p.wg_tasks.size();
        printf("%u %d %u|%s|%zu", L, (int)wave, p.W, mh::enc_name(e).c_str(), mh::enc_lds_bytes(e, L, (uint32_t)ntask));
        if (bits == 8 || bits == mh::packed_out_bits(p.info.S)) {
            const mh::DecPick d = mh::dec_pick(L, p.W, wave, bits == 8 ? 0 : bits);
            printf("|%s|%zu", mh::dec_name(d).c_str(), mh::dec_lds_bytes(d, p.W));
        } else {
            printf("|-|0");
        }
        if (bits == 8) {
            const mh::DecRungId r = mh::dec_pick(L, p.W, false, 0).rung;
            for (mh::DecForm f : {mh::kDecodeRange, mh::kDecodeRebinSat}) {
                const mh::DecPick d{r, f, 0};
                printf("|%s|%zu", mh::dec_name(d).c_str(), mh::dec_lds_bytes(d, p.W));
            }
        }
        printf("\n");
    }
    return got < 0;
}

// --worklist: every record of a packed list, read back from the blob at its section offsets
static void print_list(const mh::WorkList &w, bool rebin)
{
    const size_t o_wg = w.b_task, o_fix = o_wg + w.b_wg, o_fill = o_fix + w.b_fix;
    printf("L %zu %zu %zu %zu %u %llu %zu %zu %zu %zu\n", w.ntask, w.nwg, w.nfix, w.nfill, w.naux,
           (unsigned long long)w.max_fill, o_wg, o_fix, o_fill, w.blob.size());
    const uint8_t *b = w.blob.data();
    for (size_t i = 0; i < w.ntask; ++i) {
        if (rebin) {
            mh::RebinTask t;
            memcpy(&t, b + i * sizeof(t), sizeof(t));
            printf("T %lld %u %u %u %u %u %u %u %u %u %u\n", (long long)t.dst, t.seg, t.skip, t.n, t.lo, t.hi, t.ph, t.jfirst,
                   t.jlast, t.head, t.tail);
        } else {
            mh::RangeTask t;
            memcpy(&t, b + i * sizeof(t), sizeof(t));
            printf("T %lld %u %u %u %u %u %u %u\n", (long long)t.dst, t.seg, t.skip, t.ncnk, t.n, t.lo, t.hi, t.scr);
        }
    }
    for (size_t i = 0; i < w.nwg; ++i) {
        mh::RangeWg g;
        memcpy(&g, b + o_wg + i * sizeof(g), sizeof(g));
        printf("W %u %u %u\n", g.task0, g.ntask, g.ch);
    }
    for (size_t i = 0; i < w.nfix; ++i) {
        mh::RebinFix x;
        memcpy(&x, b + o_fix + i * sizeof(x), sizeof(x));
        printf("X %llu %u\n", (unsigned long long)x.off, x.slot);
    }
    for (size_t i = 0; i < w.nfill; ++i) {
        mh::RangeFill f;
        memcpy(&f, b + o_fill + i * sizeof(f), sizeof(f));
        printf("F %llu %llu\n", (unsigned long long)f.off, (unsigned long long)f.n);
    }
}

static int worklist()
{
    mh::PlanHost p;
    int got;
    while ((got = read_plan(false, p)) > 0) {
        if (got == 2) continue;
        const size_t n = p.seg_ch.size();
        printf("D %zu\n", n);
        for (size_t s = 0; s < n; ++s) printf("%u ", p.seg_ch[s]);
        printf("\n");
        for (size_t s = 0; s < n; ++s) printf("%llu ", (unsigned long long)p.seg_first[s]);
        printf("\n");
        for (size_t s = 0; s < n; ++s) printf("%llu ", (unsigned long long)p.seg_n[s]);
        printf("\n");
        unsigned nq;
        if (scanf("%u", &nq) != 1) return 1;
        for (unsigned q = 0; q < nq; ++q) {
            unsigned n_sel, r;
            unsigned long long t0, t1, pitch;
            if (scanf("%u", &n_sel) != 1) return 1;
            std::vector<uint32_t> sel(n_sel);
            for (auto &c : sel)
                if (scanf("%u", &c) != 1 || c >= p.info.C) return 1;
            if (scanf("%llu %llu %u %llu", &t0, &t1, &r, &pitch) != 4) return 1;
            // what mh_decode_range / mh_decode_rebin check before they build a list (but r <= 4096: the limit of the
            // kernels' division, not of the builder -- a bin longer than a segment is how one bin meets three tasks)
            const unsigned long long nb = r ? (t1 - t0 + r - 1) / r : t1 - t0;
            if (t0 >= t1 || t1 > p.max_T || (r && t0 % r) || n_sel == 0 || pitch < nb) return 1;
            if (r) print_list(mh::rebin_work_list(p, sel.data(), n_sel, t0, t1, r, pitch), true);
            else print_list(mh::range_work_list(p, sel.data(), n_sel, t0, t1, pitch), false);
        }
    }
    return got < 0;
}

// the staged bytes of a table equal the vector it was laid out from
template <class T>
static bool staged(const mh::Arena &a, const mh::Region &r, const std::vector<T> &v)
{
    return r.present && r.bytes == v.size() * sizeof(T) && r.off + r.bytes <= a.tables_bytes &&
           (v.empty() || !memcmp(a.tables.get() + r.off, v.data(), r.bytes));
}

static int arena()
{
    mh::PlanHost p;
    int got;
    while ((got = read_plan(true, p)) > 0) {
        if (got == 2) continue;
        const mh::PlanArena a = mh::plan_arena(p);
        const size_t C = p.info.C, nseg = p.seg_ch.size(), ntile = p.tile_ch.size();
        const bool wave = p.use_wave_tasks, built = p.input_bits != 8 && p.cal_tile_ch.empty();
        const bool cal = built || !p.cal_tile_ch.empty();
        const size_t ncal = built ? C : p.cal_tile_ch.size();
        CHECK(staged(a, a.tile_cnt, p.tile_cnt) && staged(a, a.ch_off, p.ch_off) && staged(a, a.ch_len, p.ch_len));
        CHECK(staged(a, a.w0, p.w0) && staged(a, a.w1, p.w1) && staged(a, a.skip, p.skip) && staged(a, a.sclv, p.sclv));
        CHECK(staged(a, a.codes, p.codes) && staged(a, a.seg_ch, p.seg_ch) && staged(a, a.seg_first, p.seg_first));
        CHECK(staged(a, a.seg_n, p.seg_n) && staged(a, a.seg_off, p.seg_off) && staged(a, a.tile_ch, p.tile_ch));
        CHECK(staged(a, a.tile_n, p.tile_n) && staged(a, a.tile_start, p.tile_start) && staged(a, a.wg_tasks, p.wg_tasks));
        CHECK(wave ? staged(a, a.wave_tasks, p.wave_tasks) : !a.wave_tasks.present);
        if (!p.cal_tile_ch.empty())
            CHECK(staged(a, a.cal_tile_ch, p.cal_tile_ch) && staged(a, a.cal_tile_n, p.cal_tile_n) &&
                  staged(a, a.cal_tile_start, p.cal_tile_start));
        CHECK(a.n_cal_tiles == ncal);
        // what each region holds, in the header's layout order: elements (-1: absent) and their size
        const struct { const char *name; long long elems; size_t size; } want[] = {
            {"sclv16", (long long)p.info.K * 4, 4}, {"tile_cnt", (long long)C, 4}, {"ch_off", (long long)C, 8},
            {"ch_len", (long long)C, 8}, {"w0", (long long)C, 8}, {"w1", (long long)C, 8}, {"skip", (long long)C, 1},
            {"sclv", (long long)p.info.K * p.info.S, 1}, {"codes", (long long)p.info.K * 16, 4}, {"seg_ch", (long long)nseg, 4},
            {"seg_first", (long long)nseg, 8}, {"seg_n", (long long)nseg, 8}, {"seg_off", (long long)nseg, 8},
            {"tile_ch", (long long)ntile, 4}, {"tile_n", (long long)ntile, 4}, {"tile_start", (long long)ntile, 8},
            {"wg_tasks", (long long)p.wg_tasks.size(), sizeof(mh::WgTask)},
            {"wave_tasks", wave ? (long long)p.wave_tasks.size() : -1, sizeof(mh::WaveTask)},
            {"cal_tile_ch", cal ? (long long)ncal : -1, 4}, {"cal_tile_n", cal ? (long long)ncal : -1, 4},
            {"cal_tile_start", cal ? (long long)ncal : -1, 8},
            {"tile_done", (long long)C, 4}, {"hist", (long long)C * 16, 8}, {"peak", (long long)C, 1}, {"enc", (long long)C, 1},
            {"lut", (long long)C * 16, 8}, {"scan", (long long)(nseg / 2048 + 2), 8}, {"err", 1, 4},
            {"acc", wave ? (long long)C : -1, 8}, {"calhist", cal ? (long long)C * 16 : -1, 8}};
        const size_t nwant = sizeof(want) / sizeof(want[0]);
        CHECK(a.regions.size() == nwant);
        printf("A %zu %zu %zu\n", a.tables_bytes, a.scratch_bytes, nwant);
        for (size_t i = 0; i < nwant; ++i) {
            const mh::Arena::Named &g = a.regions[i];
            CHECK(!strcmp(g.name, want[i].name));
            printf("R %s %c %d %zu %zu %lld %zu\n", g.name, g.scratch ? 'S' : 'T', (int)g.r.present, g.r.off, g.r.bytes,
                   want[i].elems, want[i].size);
        }
        CHECK(a.sclv16.present && a.sclv16.bytes == (size_t)p.info.K * 16);
        printf("K");
        for (size_t i = 0; i < (size_t)p.info.K * 4; ++i) {
            uint32_t w;
            memcpy(&w, a.tables.get() + a.sclv16.off + 4 * i, 4);
            printf(" %u", w);
        }
        printf("\nP %zu\n", built ? C : (size_t)0);
        for (size_t c = 0; built && c < C; ++c) {
            uint32_t ch, n;
            uint64_t start;
            memcpy(&ch, a.tables.get() + a.cal_tile_ch.off + 4 * c, 4);
            memcpy(&n, a.tables.get() + a.cal_tile_n.off + 4 * c, 4);
            memcpy(&start, a.tables.get() + a.cal_tile_start.off + 8 * c, 8);
            printf("%u %llu %u\n", ch, (unsigned long long)start, n);
        }
    }
    return got < 0;
}

static bool read_u64s(std::vector<uint64_t> &v)
{
    for (auto &x : v) {
        unsigned long long t;
        if (scanf("%llu", &t) != 1) return false;
        x = t;
    }
    return true;
}

static bool read_u8s(std::vector<uint8_t> &v)
{
    for (auto &x : v) {
        unsigned t;
        if (scanf("%u", &t) != 1) return false;
        x = (uint8_t)t;
    }
    return true;
}

static int validate()
{
    PlanArgs a;
    int got;
    while ((got = read_plan_args(false, a)) > 0) {
        unsigned long long nseg, nwords, nwalks;
        if (scanf("%llu", &nseg) != 1) return 1;
        std::vector<uint64_t> seg_words(nseg);
        std::vector<uint8_t> peak(a.C), enc(a.C);
        if (!read_u64s(seg_words) || !read_u8s(peak) || !read_u8s(enc) || scanf("%llu", &nwords) != 1) return 1;
        const std::unique_ptr<uint32_t[]> payload(new uint32_t[nwords]);  // exactly the words: nothing behind them is readable
        char tok[4096];
        for (unsigned long long i = 0; i < nwords || i == 0; ++i) {
            if (scanf("%4095s", tok) != 1) return 1;
            if (i == 0 && tok[0] == '@') {
                FILE *f = fopen(tok + 1, "rb");
                if (!f) return 1;
                const size_t n = fread(payload.get(), 4, nwords, f);
                const bool whole = n == nwords && fgetc(f) == EOF;
                fclose(f);
                if (!whole) return 1;
                break;
            }
            if (i >= nwords) {  // no words: "-"
                if (strcmp(tok, "-")) return 1;
                break;
            }
            payload[i] = (uint32_t)strtoul(tok, nullptr, 10);
        }
        {   // mh_validate_stream
            mh::PlanHost H;
            mh::Msg m;
            int rc = mh::stored_plan_host(m, "mh_validate_stream", a.len.data(), a.C, a.S, a.h, a.mode, a.window, a.sclv.data(),
                                           a.K, a.sc, nseg, H);
            if (!rc) rc = mh::validate_stream(m, H, payload.get(), nwords, seg_words.data(), peak.data(), enc.data());
            printf("S %d %s\n", rc, m.text);
        }
        if (scanf("%llu", &nwalks) != 1) return 1;
        for (unsigned long long k = 0; k < nwalks; ++k) {  // mh_validate_segments
            unsigned null;
            unsigned long long n_idx;
            if (scanf("%u %llu", &null, &n_idx) != 2 || (null && n_idx)) return 1;
            std::vector<uint64_t> seg_idx(n_idx), seg_off(nseg);
            if (!read_u64s(seg_idx) || !read_u64s(seg_off)) return 1;
            mh::PlanHost H;
            mh::Msg m;
            int rc = mh::stored_plan_host(m, "mh_validate_segments", a.len.data(), a.C, a.S, a.h, a.mode, a.window,
                                           a.sclv.data(), a.K, a.sc, nseg, H);
            if (!rc)
                rc = mh::validate_segments(m, "mh_validate_segments", H, null ? nullptr : payload.get(), nwords, seg_off.data(),
                                           seg_words.data(), seg_idx.data(), n_idx, peak.data(), enc.data());
            printf("G %d %s\n", rc, m.text);
        }
    }
    return got < 0;
}

static int sweep()
{
    unsigned C, nh;
    while (scanf("%u %u", &C, &nh) == 2) {
        if (C > (1u << 20) || nh > 64) return 1;
        std::vector<uint32_t> bits(nh);
        for (auto &b : bits)
            if (scanf("%u", &b) != 1) return 1;
        std::vector<uint64_t> len(C), off(C);
        if (!read_u64s(len)) return 1;
        uint64_t o = 0;
        for (unsigned c = 0; c < C; ++c) {
            off[c] = o;
            o += (len[c] + 15) & ~15ull;
        }
        mh::Msg m;
        if (const int rc = mh::sweep_check_args(m, len.data(), C, bits.data(), nh)) {
            printf("error %d\n", rc);
            continue;
        }
        mh::SweepHost w;
        mh::sweep_host_build(w, off.data(), len.data(), C, bits.data(), nh);
        const size_t nt = w.tile_ch.size();
        CHECK(w.C == C && w.nh == nh && w.ni == 2 * nh + 1 && w.ch_off == off);
        CHECK(w.bounds.size() == (size_t)C * (w.ni + 1) && w.slot_len.size() == (size_t)C * w.ni);
        CHECK(w.tile_n.size() == nt && w.tile_slot.size() == nt && w.tile_start.size() == nt);
        const mh::SweepArena a = mh::sweep_arena(w);
        CHECK(staged(a, a.ch_off, w.ch_off) && staged(a, a.tile_ch, w.tile_ch) && staged(a, a.tile_n, w.tile_n));
        CHECK(staged(a, a.tile_slot, w.tile_slot) && staged(a, a.tile_start, w.tile_start) && staged(a, a.slot_len, w.slot_len));
        CHECK(a.regions.size() == 7 && a.hist.present && a.hist.off >= a.tables_bytes && a.hist.bytes == w.slot_len.size() * 16 * 8);
        CHECK(a.hist.off + a.hist.bytes <= a.bytes() && a.tables_bytes % mh::kArenaAlign == 0 && a.scratch_bytes % mh::kArenaAlign == 0);
        printf("W %u %zu %zu %zu\nB", w.ni, nt, a.tables_bytes, a.scratch_bytes);
        for (uint64_t b : w.bounds) printf(" %llu", (unsigned long long)b);
        printf("\nL");
        for (uint64_t l : w.slot_len) printf(" %llu", (unsigned long long)l);
        printf("\n");
        for (size_t t = 0; t < nt; ++t)
            printf("T %u %u %llu %u\n", w.tile_ch[t], w.tile_slot[t], (unsigned long long)w.tile_start[t], w.tile_n[t]);
    }
    return !feof(stdin);
}

static int geometry()
{
    char name[32];
    while (scanf("%31s", name) == 1) {
        unsigned long long v[3] = {0, 0, 0};
        const bool two = !strcmp(name, "synth") || !strcmp(name, "chunk_stride") || !strcmp(name, "excess_apply1") || !strcmp(name, "excess_apply");
        const bool one = !strcmp(name, "items") || !strcmp(name, "compact") || !strcmp(name, "seg_crc32");
        for (int i = 0; i < (one ? 1 : two ? 2 : 3); ++i)
            if (scanf("%llu", &v[i]) != 1) return 1;
        mh::Msg m;
        int rc = MH_OK;
        if (!strcmp(name, "synth")) {
            const mh::GridXY g = mh::synth_grid(v[0], (uint32_t)v[1]);
            printf("synth %u %u\n", g.x, g.y);
        } else if (!strcmp(name, "rebin")) {
            if (v[2] < 1 || v[2] > 4096) return 1;  // (what mh_rebin refuses before it looks at a grid)
            if (v[2] < 4) {
                const mh::GridXY g = mh::rebin2_grid(v[0], (uint32_t)v[1], (uint32_t)v[2]);
                printf("rebin %u %u\n", g.x, g.y);
            } else {
                const mh::Rebin3Launch l = mh::rebin3_launch(v[0], (uint32_t)v[1], (uint32_t)v[2]);
                printf("rebin %u %u %u %u %u %u\n", l.grid.x, l.grid.y, l.g, l.u, l.upt, l.tpw);
            }
        } else if (!strcmp(name, "fills")) {
            if (v[1] == 0) return 1;
            printf("fills %u", mh::fill_grid_x(v[0], v[1]));
            for (uint64_t f = 0; f < v[2]; f += mh::kFillMaxRecords) printf(" %u", mh::fill_grid_y(v[2], f));
            printf("\n");
        } else if (!strcmp(name, "transposed")) {
            if (v[1] == 0 || v[2] == 0) return 1;
            uint32_t grid = 0;
            if (!(rc = mh::transposed_grid(m, "transposed", v[0], (uint32_t)v[1], (uint32_t)v[2], &grid))) printf("transposed %u\n", grid);
        } else if (!strcmp(name, "items")) {
            uint32_t grid = 0;
            if (!(rc = mh::per_item_grid(m, "items", "items", v[0], &grid))) printf("items %u\n", grid);
        } else if (!strcmp(name, "compact")) {
            const uint32_t blocks = mh::compact_scan_blocks(v[0]);
            printf("compact %d %u %u\n", (int)(blocks <= 1), blocks, mh::compact_groups(v[0]));
        } else if (!strcmp(name, "bin_events")) {
            if (v[0] == 0 || v[1] == 0 || v[2] == 0) return 1;
            mh::BinLaunch l;
            if (!(rc = mh::bin_events_launch(m, (uint32_t)v[0], v[1], v[2], &l)))
                printf("bin_events %u %llu %llu %llu %u\n", l.grid, (unsigned long long)l.nchunks, (unsigned long long)l.span,
                       (unsigned long long)l.nspans, l.div_mode);
        } else if (!strcmp(name, "seg_crc32")) {
            printf("seg_crc32 %u\n", mh::seg_crc_grid(v[0]));
        } else if (!strcmp(name, "excess_apply1")) {
            if (v[0] == 0 || v[1] == 0) return 1;  // (mhi_excess_apply returns before it looks at a grid)
            const mh::GridXY g = mh::excess_apply1_grid(v[0], v[1]);
            printf("excess_apply1 %u %u\n", g.x, g.y);
        } else if (!strcmp(name, "excess_apply")) {
            if (v[0] == 0 || v[1] == 0 || (unsigned __int128)v[0] * v[1] >= ((unsigned __int128)1 << 63)) return 1;  // (refused)
            printf("excess_apply %u\n", mh::excess_apply_grid(v[0], v[1]));
        } else if (!strcmp(name, "chunk_stride")) {
            printf("chunk_stride %d\n", (int)mh::chunk_stride_ok(v[0], (uint32_t)v[1]));
        } else {
            return 1;
        }
        if (rc) printf("%s error %d %s\n", name, rc, m.text);
    }
    return !feof(stdin);
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--validate")) return validate();
    if (argc > 1 && !strcmp(argv[1], "--sweep")) return sweep();
    if (argc > 1 && !strcmp(argv[1], "--geometry")) return geometry();
    if (argc > 1 && !strcmp(argv[1], "--arena")) return arena();
    if (argc > 1 && !strcmp(argv[1], "--cells")) return cells(false);
    if (argc > 1 && !strcmp(argv[1], "--forms")) return cells(true);
    if (argc > 1 && !strcmp(argv[1], "--tiles")) return cells(false, true);
    if (argc > 1 && !strcmp(argv[1], "--worklist")) return worklist();
    if (argc > 1 && !strcmp(argv[1], "--tasks")) return tasks();
    mh::PlanHost p;
    int got;
    while ((got = read_plan(false, p)) > 0) {
        if (got == 2) continue;
        const unsigned C = p.info.C, h = p.info.h;
        const uint32_t maxlen = p.info.maxlen;
        const std::vector<uint64_t> &len = p.ch_len, &off = p.ch_off;
        const size_t n = p.seg_ch.size();
        CHECK(p.info.n_segments == n && p.seg_first.size() == n && p.seg_n.size() == n && p.seg_off.size() == n);
        // segments tile every window exactly, in order; slots do not overlap and fit the capacity
        uint64_t samples = 0;
        for (size_t s = 0; s < n; ++s) {
            const uint32_t c = p.seg_ch[s];
            CHECK(c < C && p.seg_n[s] > 0 && p.seg_n[s] <= (uint64_t)p.info.seg_chunks * MH_CHUNK);
            CHECK(p.seg_first[s] + p.seg_n[s] <= p.w1[c] - p.w0[c]);
            if (s + 1 < n) CHECK(p.seg_off[s] + mh::slot_words(p.seg_n[s], maxlen) == p.seg_off[s + 1]);
            CHECK(p.seg_off[s] % 32 == 0);
            samples += p.seg_n[s];
        }
        CHECK(samples == p.info.window_samples);
        // each channel's run of the directory
        CHECK(p.ch_seg0.size() == (size_t)C + 1 && p.ch_seg0[0] == 0 && p.ch_seg0[C] == n);
        for (unsigned c = 0; c < C; ++c) {
            CHECK(p.ch_seg0[c] <= p.ch_seg0[c + 1]);
            for (uint64_t s = p.ch_seg0[c]; s < p.ch_seg0[c + 1]; ++s) CHECK(p.seg_ch[s] == c);
        }
        if (n) CHECK(p.seg_off[n - 1] + mh::slot_words(p.seg_n[n - 1], maxlen) + 4 == p.info.payload_cap_words);
        // shared-table tasks: every segment once in directory order, 1..4 consecutive ones of one channel, a head segment
        // alone; what a wave derives from the record by arithmetic equals the directory
        const uint64_t seg_samples = (uint64_t)p.info.seg_chunks * MH_CHUNK;
        CHECK(p.seg_src_stride == seg_samples && p.slot_full == mh::slot_words(seg_samples, maxlen));
        size_t covered = 0;
        for (size_t t = 0; t < p.wg_tasks.size(); ++t) {
            const mh::WgTask &w = p.wg_tasks[t];
            CHECK(w.seg0 == covered && w.nseg >= 1 && w.nseg <= 4 && covered + w.nseg <= n && w.ch == p.seg_ch[w.seg0]);
            covered += w.nseg;
            const bool head = p.seg_first[w.seg0] == 0 && mh::head_samples(p.w0[w.ch], p.w1[w.ch], p.info.window) != 0;
            if (head) CHECK(w.nseg == 1 && w.n_last == mh::head_samples(p.w0[w.ch], p.w1[w.ch], p.info.window));
            for (uint32_t k = 0; k < w.nseg; ++k) {
                const size_t sg = (size_t)w.seg0 + k;
                CHECK(p.seg_ch[sg] == w.ch);
                CHECK(w.src_off + k * p.seg_src_stride == off[w.ch] + p.w0[w.ch] + p.seg_first[sg]);
                CHECK(w.dst_off + k * p.slot_full == p.seg_off[sg]);
                CHECK((k + 1 < w.nseg ? seg_samples : (uint64_t)w.n_last) == p.seg_n[sg]);
            }
        }
        CHECK(covered == n);
        if (p.use_wave_tasks) {  // every segment once, longest first, then one record per channel without segments
            std::vector<uint8_t> seen(n, 0);
            std::vector<uint32_t> per_ch(C, 0), first_ch(C, 0);
            size_t nreal = 0;
            for (size_t i = 0; i < p.wave_tasks.size(); ++i) {
                const mh::WaveTask &t = p.wave_tasks[i];
                CHECK(t.ch < C && t.cal_off == off[t.ch]);
                CHECK(t.cal_n == (len[t.ch] < ((uint64_t)1 << h) ? len[t.ch] : (((uint64_t)1 << h) <= mh::kCalDirect ? ((uint64_t)1 << h) : 0)));
                CHECK(((t.flags >> 1) & 1u) == p.skip[t.ch]);
                ++per_ch[t.ch];
                first_ch[t.ch] += t.flags & 1u;
                if (t.n == 0) continue;
                CHECK(nreal == i);  // real work first
                ++nreal;
                CHECK(t.seg < n && !seen[t.seg]);
                seen[t.seg] = 1;
                CHECK(t.ch == p.seg_ch[t.seg] && t.n == p.seg_n[t.seg] && t.dst_off == p.seg_off[t.seg]);
                CHECK(t.src_off == off[t.ch] + p.w0[t.ch] + p.seg_first[t.seg]);  // byte input
                CHECK(t.src_off + t.n <= off[t.ch] + len[t.ch]);
                CHECK((t.flags & 1u) == (p.seg_first[t.seg] == 0 ? 1u : 0u));
                if (i) CHECK(p.wave_tasks[i - 1].n >= t.n);
            }
            CHECK(nreal == n);
            for (unsigned c = 0; c < C; ++c) CHECK(per_ch[c] >= 1 && first_ch[c] == 1);
            for (const mh::WaveTask &t : p.wave_tasks) CHECK(t.nseg_ch == per_ch[t.ch]);
            CHECK(p.fused_calibration == (((uint64_t)1 << h) <= mh::kCalDirect));
        }
        // histogram tiles cover the windows; calibration tiles cover min(2^h, T) when it is long
        uint64_t tiled = 0;
        std::vector<unsigned> tiles_of(C, 0);
        for (size_t t = 0; t < p.tile_ch.size(); ++t) {
            const unsigned c = p.tile_ch[t];
            CHECK(c < C && p.tile_n[t] <= mh::kHistTileBytes);
            CHECK(p.tile_n[t] > 0 || p.w0[c] == p.w1[c]);  // an empty tile only for an empty window
            CHECK(p.tile_start[t] + p.tile_n[t] <= p.w1[c]);
            tiled += p.tile_n[t];
            ++tiles_of[c];
        }
        CHECK(tiled == p.info.window_samples);
        CHECK(p.tile_cnt.size() == C);  // every channel has a tile: its last tile's workgroup finishes the channel
        for (unsigned c = 0; c < C; ++c) CHECK(tiles_of[c] >= 1 && tiles_of[c] == p.tile_cnt[c]);
        uint64_t cal = 0, cal_want = 0;
        for (size_t t = 0; t < p.cal_tile_ch.size(); ++t) cal += p.cal_tile_n[t];
        if (((uint64_t)1 << h) > mh::kCalDirect)
            for (unsigned c = 0; c < C; ++c) cal_want += len[c] < ((uint64_t)1 << h) ? len[c] : ((uint64_t)1 << h);
        CHECK(cal == cal_want);
        CHECK(p.W >= maxlen && p.W <= 12);
        printf("%zu %llu %u %d %d\n", n, (unsigned long long)p.info.payload_cap_words, p.info.seg_chunks, (int)p.use_wave_tasks,
               (int)p.tickets_fit);
        for (size_t s = 0; s < n; ++s) printf("%u ", p.seg_ch[s]);
        printf("\n");
        for (size_t s = 0; s < n; ++s) printf("%llu ", (unsigned long long)p.seg_first[s]);
        printf("\n");
        for (size_t s = 0; s < n; ++s) printf("%llu ", (unsigned long long)p.seg_n[s]);
        printf("\n");
        for (size_t s = 0; s < n; ++s) printf("%llu ", (unsigned long long)p.seg_off[s]);
        printf("\n");
    }
    return got < 0;
}
