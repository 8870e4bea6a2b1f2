// mh_rows.hpp -- what the companions' layout headers share: the bounds of a matrix of byte rows, the extent of strided rows,
// the overlap test, the argument rules whose text is the same in every library, and how 4 bytes of a row at any alignment
// are read.  Pure C++ as mh_msg.hpp (no HIP on the host, no state); the one device function is behind __HIPCC__.  The
// ORDER in which a *_check() tests its rules decides which message a caller sees and stays with each check function:
// here are only the bodies of single rules.
#pragma once
#include <stdint.h>

#include "mh_msg.hpp"
#include "muahuff.h"

#if defined(__HIPCC__)
#define MH_HD __host__ __device__
#else
#define MH_HD
#endif

namespace mh {

constexpr uint64_t kMaxCols = 1ull << 40;    // cols is below this
constexpr uint64_t kMaxStride = 1ull << 48;  // a row stride is below this: rows * stride stays inside 64 bits

inline bool ranges_overlap(uint64_t a, uint64_t a_end, uint64_t b, uint64_t b_end) { return a < b_end && b < a_end; }

// the end of n rows of row_bytes bytes, `stride` bytes apart, from `base` on; the stride of a single row is not looked at
inline uint64_t strided_end(uint64_t base, uint64_t n, uint64_t stride, uint64_t row_bytes)
{
    return base + (n - 1) * (n > 1 ? stride : 0) + row_bytes;
}

// the rules with one text everywhere: MH_OK, or MH_ERR_ARG with the text in m.  `fn` names the entry point.
inline int k_rule(Msg &m, const char *fn, uint32_t k, uint32_t max)
{
    return k < 1 || k > max ? m.set(MH_ERR_ARG, "%s: k=%u outside 1..%u", fn, k, max) : MH_OK;
}

inline int rows_rule(Msg &m, const char *fn, uint64_t rows, uint64_t max)
{
    return rows < 1 || rows > max ? m.set(MH_ERR_ARG, "%s: rows=%llu outside 1..%llu", fn, (unsigned long long)rows, (unsigned long long)max)
                                  : MH_OK;
}

inline int cols_rule(Msg &m, const char *fn, uint64_t cols)
{
    return cols < 1 || cols >= kMaxCols ? m.set(MH_ERR_ARG, "%s: cols=%llu outside 1..2^40-1", fn, (unsigned long long)cols) : MH_OK;
}

inline int clip_rule(Msg &m, const char *fn, uint32_t clip)
{
    return clip < 1 || clip > 255 ? m.set(MH_ERR_ARG, "%s: clip=%u outside 1..255", fn, clip) : MH_OK;
}

// May the 4 columns from t on (t a multiple of 4, t < cols) of a row whose first byte sits `sh` = 0..3 bytes behind a dword
// boundary be taken from aligned dwords?  They lie in the dword at byte t - sh of the row and, with sh > 0, the next one:
// both must lie inside the row's cols bytes.
MH_HD inline bool dwords_ok(uint64_t t, uint32_t sh, uint64_t cols)
{
    return sh == 0 ? t + 4 <= cols : (t >= sh && t - sh + 8 <= cols);
}

#if defined(__HIPCC__)
// the bytes of the columns t .. t + 3 (t a multiple of 4, below cols) of a row as one dword, byte b in bits 8 b: from the
// aligned dwords that hold them where those lie inside the row (dwords_ok), byte by byte otherwise (columns from cols on
// read as 0).  Nothing outside the row's cols bytes is read.
__device__ inline uint32_t load4(const uint8_t *row, uint64_t t, uint64_t cols)
{
    const uint32_t sh = (uint32_t)((uintptr_t)row & 3);
    if (dwords_ok(t, sh, cols)) {
        const uint32_t *const a0 = reinterpret_cast<const uint32_t *>(row + t - sh);
        const uint32_t lo = a0[0];
        if (sh == 0) return lo;
        return (uint32_t)((((uint64_t)a0[1] << 32) | lo) >> (8 * sh));
    }
    uint32_t d = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if (t + b < cols) d |= (uint32_t)row[t + b] << (8 * b);
    return d;
}
#endif

}  // namespace mh
