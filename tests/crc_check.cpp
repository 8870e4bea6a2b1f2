// crc_check.cpp -- csrc/mh_crc_tables.hpp built alone as a plain host program: no HIP, no Python, so that it can be
// built with -fsanitize=address,undefined (tests/test_host_checksum.py).  Reads byte strings from stdin, one per line
// in hex (an empty line is the empty string), and prints per line
//     <crc32_ref> <wave form>
// in hex: the byte-at-a-time reference, and the piece / row / lane arithmetic of k_seg_crc32 (csrc/mh_crc.hpp) done by
// 64 lanes in a loop over the same tables -- rows laid from the segment's end, the cut piece at the head read word by
// word, the first word complemented, one carry-less multiply per lane, the 64 remainders xor-ed.  The wave form takes
// whole words only ("-" for other lengths) and a segment of 0 words is 0 by definition.  The words sit in a heap block
// of exactly their size, so a read in front of or behind the segment stops the program.
// A line that starts with "check" asks csrc/mh_ingest_check.hpp -- the argument rules of mhi_seg_crc32 and of
// mhi_bin_events, built into the same program -- for a verdict, every argument of the ABI but the stream as a number
// (pointers too, 0 = NULL), and prints "ok" or "error <code> <message>":
//   check crc payload payload_words seg_off seg_words n_segments seg_idx n_idx crc expect bad
//   check bin_events ticks ev_off C origin period T bits out out_off chunk_stride where n entry*n
//     where: 0 device, 1 both, 2 host only (kWhere*); the n entries are what out_off[0 .. n) holds
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mh_crc_tables.hpp"
#include "mh_ingest_check.hpp"

static constexpr mh::CrcTables kTables = mh::make_crc_tables();
static_assert(kTables.slice[0][1] == 0x77073096u && kTables.lane[63] == mh::kCrcOne, "the byte table is zlib's");

static uint32_t wave_form(const uint32_t *seg, uint64_t n)
{
    if (n == 0) return 0;
    const uint64_t rows = mh::crc_rows(n);
    uint32_t total = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const int64_t w = (int64_t)n - (int64_t)(256 * rows) + 4 * (int64_t)lane;
        uint32_t a = 0, b = 0, c = 0, d = 0;
        if (w >= 0) {
            a = seg[w], b = seg[w + 1], c = seg[w + 2], d = seg[w + 3];
        } else if (w > -4) {
            if (w + 1 >= 0) b = seg[w + 1];
            if (w + 2 >= 0) c = seg[w + 2];
            d = seg[w + 3];
        }
        if (w == 0) a = ~a;
        if (w == -1) b = ~b;
        if (w == -2) c = ~c;
        if (w == -3) d = ~d;
        uint32_t acc = mh::crc_piece(kTables, a, b, c, d);
        for (uint64_t r = 1; r < rows; ++r) {
            const uint32_t *p = seg + (w + (int64_t)(256 * r));
            acc = mh::crc_next_row(kTables, acc) ^ mh::crc_piece(kTables, p[0], p[1], p[2], p[3]);
        }
        total ^= mh::crc_mulmod(acc, kTables.lane[lane]);
    }
    return ~total;
}

// "crc <10 numbers>" / "bin_events <10 numbers> where n entry ...": the verdict of csrc/mh_ingest_check.hpp.  The n entries
// stand for out_off[0 .. n) in a heap block of exactly their size, so a read behind them stops the program; with n == 0
// out_off is the number given, which only says NULL or not and must not be read through.
static int check(const char *text)
{
    char what[16];
    int used = 0;
    if (sscanf(text, "%15s%n", what, &used) != 1) return 3;
    text += used;
    std::vector<unsigned long long> v;
    unsigned long long x;
    while (sscanf(text, "%llu%n", &x, &used) == 1) v.push_back(x), text += used;
    mh::Msg m;
    int rc;
    if (!strcmp(what, "crc") && v.size() == 10) {
        const mh::CrcArgs a = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
        mh::CrcLaunch l = {~0ull, ~0u};
        rc = mh::seg_crc_check(m, a, &l);
        if (rc == MH_OK && (l.n_list != (a.seg_idx ? a.n_idx : a.n_segments) || (l.grid == 0) != (l.n_list == 0) || l.grid > mh::kCrcMaxX))
            return 2;
    } else if (!strcmp(what, "bin_events") && v.size() >= 12 && v.size() == 12 + v[11]) {
        const std::vector<uint64_t> table(v.begin() + 12, v.end());
        const mh::BinArgs a = {v[0], v[1], (uint32_t)v[2], v[3], v[4], v[5], (uint32_t)v[6], v[7],
                               v[8] && !table.empty() ? (uint64_t)(uintptr_t)table.data() : v[8], v[9]};
        mh::BinLaunch l;
        rc = mh::bin_events_check(m, a);
        if (rc == MH_OK) rc = mh::bin_events_table_check(m, a, (uint32_t)v[10], &l);
    } else {
        return 3;
    }
    if ((rc == MH_OK) != (m.text[0] == 0) || (rc != MH_OK && rc != MH_ERR_ARG)) return 2;
    if (rc)
        printf("error %d %s\n", rc, m.text);
    else
        printf("ok\n");
    return 0;
}

static int nibble(int ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1; }

int main()
{
    std::string line;
    int ch;
    bool any = false;
    while ((ch = getchar()) != EOF || any) {
        if (ch != '\n' && ch != EOF) {
            line.push_back((char)ch);
            any = true;
            continue;
        }
        if (line.compare(0, 6, "check ") == 0) {
            if (int rc = check(line.c_str() + 6)) return rc;
            line.clear();
            any = false;
            if (ch == EOF) break;
            continue;
        }
        if (line.size() % 2) return 2;
        std::vector<uint8_t> bytes(line.size() / 2);
        for (size_t i = 0; i < bytes.size(); ++i) {
            const int hi = nibble(line[2 * i]), lo = nibble(line[2 * i + 1]);
            if (hi < 0 || lo < 0) return 2;
            bytes[i] = (uint8_t)(hi * 16 + lo);
        }
        printf("%08x ", mh::crc32_ref(kTables, bytes.data(), bytes.size()));
        if (bytes.size() % 4 == 0) {
            std::vector<uint32_t> words(bytes.size() / 4);  // little-endian words, as the payload holds them
            for (size_t i = 0; i < words.size(); ++i)
                words[i] = (uint32_t)bytes[4 * i] | (uint32_t)bytes[4 * i + 1] << 8 | (uint32_t)bytes[4 * i + 2] << 16 |
                           (uint32_t)bytes[4 * i + 3] << 24;
            printf("%08x\n", wave_form(words.data(), words.size()));
        } else {
            printf("-\n");
        }
        line.clear();
        any = false;
        if (ch == EOF) break;
    }
    return 0;
}
