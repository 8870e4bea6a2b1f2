// mh_crc_tables.hpp -- CRC-32 (zlib / IEEE 802.3: reflected polynomial 0xEDB88320, initial value and final xor
// 0xFFFFFFFF, crc32("123456789") = 0xCBF43926) as k_seg_crc32 (mh_crc.hpp) computes it: the lookup tables, the shift
// constants, the carry-less multiply and a byte-at-a-time reference.  Host-only: no HIP here, so that
// tests/crc_check.cpp builds it alone under the sanitizers; every table is made by constexpr arithmetic from the
// polynomial, nothing is pasted in.
//
// Notation: raw(M) is the remainder with a ZERO initial value and no final xor, a polynomial over GF(2) of degree < 32
// held reflected (bit 31 = x^0, bit 0 = x^31).  raw is linear, raw of leading zero bytes is 0, and feeding k zero
// bytes multiplies the remainder by x^(8k) mod P, so for a message cut into pieces
//     raw(M) = XOR over pieces p of raw(p) * x^(8 * bytes of M behind p)
// and, for a message of at least 4 bytes, the initial value is the same as complementing its first 4 bytes:
//     crc32(M) = raw(M with its first word complemented) ^ 0xFFFFFFFF.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mh {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;    // the polynomial 1
constexpr uint32_t kCrcPiece = 16;           // bytes a lane takes per row
constexpr uint32_t kCrcRow = 64 * kCrcPiece; // bytes a wave takes per row

// a * b mod P (both reflected).  Branch-free, 32 steps: the kernel runs it once per lane and segment.
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {  // bit i of a: the coefficient of x^(31 - i)
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

struct CrcTables {
    uint32_t slice[16][256];  // slice[k][b] = raw(byte b followed by k zero bytes)
    uint32_t row[4][256];     // row[j][b] = (b << 8j) * x^(8 * kCrcRow): a remainder moved one row ahead, byte by byte
    uint32_t lane[64];        // lane[l] = x^(8 * kCrcPiece * (63 - l)): from the end of lane l's piece to the row's end
};

constexpr CrcTables make_crc_tables()
{
    CrcTables t{};
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t v = b;
        for (int i = 0; i < 8; ++i) v = (v >> 1) ^ (kCrcPoly & (0u - (v & 1u)));
        t.slice[0][b] = v;
    }
    for (int k = 1; k < 16; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t v = t.slice[k - 1][b];
            t.slice[k][b] = (v >> 8) ^ t.slice[0][v & 0xFFu];
        }
    uint32_t x_piece = kCrcOne >> 1;  // x, squared until it is x^(8 * kCrcPiece), then on to x^(8 * kCrcRow)
    for (uint32_t e = 1; e < 8 * kCrcPiece; e *= 2) x_piece = crc_mulmod(x_piece, x_piece);
    uint32_t x_row = x_piece;
    for (uint32_t e = kCrcPiece; e < kCrcRow; e *= 2) x_row = crc_mulmod(x_row, x_row);
    for (int j = 0; j < 4; ++j) {
        t.row[j][0] = 0;
        for (uint32_t b = 1; b < 256; ++b) {  // linear: the entry without b's lowest set bit, plus that bit's image
            const uint32_t low = b & (0u - b);
            t.row[j][b] = b == low ? crc_mulmod(b << (8 * j), x_row) : t.row[j][b ^ low] ^ t.row[j][low];
        }
    }
    t.lane[63] = kCrcOne;
    for (int l = 62; l >= 0; --l) t.lane[l] = crc_mulmod(t.lane[l + 1], x_piece);
    return t;
}

// the reference: one byte at a time over slice[0]
inline uint32_t crc32_ref(const CrcTables &t, const uint8_t *bytes, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = (c >> 8) ^ t.slice[0][(c ^ bytes[i]) & 0xFFu];
    return c ^ 0xFFFFFFFFu;
}

// ---- the kernel's arithmetic, one lane's share (constexpr: host and device alike) -------------------------------
// raw of one 16-byte piece, words in memory order (little-endian bytes): 16 lookups
template <typename T>
constexpr uint32_t crc_piece(const T &t, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    return t.slice[15][w0 & 0xFFu] ^ t.slice[14][(w0 >> 8) & 0xFFu] ^ t.slice[13][(w0 >> 16) & 0xFFu] ^ t.slice[12][w0 >> 24] ^
           t.slice[11][w1 & 0xFFu] ^ t.slice[10][(w1 >> 8) & 0xFFu] ^ t.slice[9][(w1 >> 16) & 0xFFu] ^ t.slice[8][w1 >> 24] ^
           t.slice[7][w2 & 0xFFu] ^ t.slice[6][(w2 >> 8) & 0xFFu] ^ t.slice[5][(w2 >> 16) & 0xFFu] ^ t.slice[4][w2 >> 24] ^
           t.slice[3][w3 & 0xFFu] ^ t.slice[2][(w3 >> 8) & 0xFFu] ^ t.slice[1][(w3 >> 16) & 0xFFu] ^ t.slice[0][w3 >> 24];
}

// a remainder moved one row (kCrcRow bytes) ahead: 4 lookups
template <typename T>
constexpr uint32_t crc_next_row(const T &t, uint32_t acc)
{
    return t.row[0][acc & 0xFFu] ^ t.row[1][(acc >> 8) & 0xFFu] ^ t.row[2][(acc >> 16) & 0xFFu] ^ t.row[3][acc >> 24];
}

// Rows are laid from the END of the segment: with n words and R = ceil(n / 256) rows, lane l's piece of row r
// (r = 0 first) begins at word n - 256 (R - r) + 4 l, which is negative only in row 0 -- the words in front of the
// segment count as zero bytes, which raw() ignores, so the cut piece is at the HEAD and every piece ends a whole
// number of pieces in front of the segment's end.
constexpr uint64_t crc_rows(uint64_t n_words) { return (n_words + 255) / 256; }

}  // namespace mh
