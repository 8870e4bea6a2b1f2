// mh_crc.hpp -- k_seg_crc32: zlib's CRC-32 of every listed directory segment of a payload, one value per segment
// (include/muahuff_ingest.h, mhi_seg_crc32).  The arithmetic and its tables are mh_crc_tables.hpp's.
//
// One wave per segment, four per workgroup (as k_compact: a segment is a few KiB), the grid capped at kCrcMaxGroups
// with a stride loop over the list.  A wave reads its segment in rows of 1 KiB, 16 bytes per lane, laid from the
// segment's END (crc_rows): a lane keeps one remainder, moved one row ahead per row (4 lookups) and joined with the raw
// remainder of its next piece (16 lookups, slice-by-16); behind the last row lane l's remainder is 16 (63 - l) bytes
// short of the segment's end -- one carry-less multiply by x^(128 (63 - l)) -- and the 64 are xor-ed together.  The
// initial value 0xFFFFFFFF is the complement of the segment's first word.  After mh_compact a segment starts at any
// word, so the 16-byte loads are the unaligned ones (u32x4_u); the head row's cut piece is read word by word and
// nothing in front of the segment is touched.  Tables: 20.25 KiB of LDS per workgroup, copied at its start.
#pragma once
#include "mh_crc_tables.hpp"
#include "mh_device.hpp"

namespace mh {

constexpr uint32_t kCrcWaves = 4;          // segments in flight per workgroup
constexpr uint32_t kCrcMaxGroups = 2048;   // 8 per CU; a longer list is walked in strides of 4 * gridDim.x
constexpr uint32_t kCrcAhead = 4;          // rows a wave loads before it folds them in

__device__ const CrcTables d_crc_tables = make_crc_tables();

// the CRC-32 of words [0, n) at seg, n >= 1, in every lane
__device__ __forceinline__ uint32_t wave_crc32(const CrcTables &t, const uint32_t *seg, uint64_t n, uint32_t lane)
{
    const uint64_t rows = crc_rows(n);
    // head row: lane l's piece begins at word w, before the segment when w < 0
    const int64_t w = (int64_t)n - (int64_t)(256 * rows) + 4 * (int64_t)lane;
    uint32_t a = 0, b = 0, c = 0, d = 0;
    if (w >= 0) {
        const u32x4 v = *reinterpret_cast<const u32x4_u *>(seg + w);
        a = v.x, b = v.y, c = v.z, d = v.w;
    } else if (w > -4) {  // words w + 1 .. w + 3, those at or behind word 0
        if (w + 1 >= 0) b = seg[w + 1];
        if (w + 2 >= 0) c = seg[w + 2];
        d = seg[w + 3];
    }
    // the first word of the segment, complemented (n >= 1: exactly one lane holds it)
    if (w == 0) a = ~a;
    if (w == -1) b = ~b;
    if (w == -2) c = ~c;
    if (w == -3) d = ~d;
    uint32_t acc = crc_piece(t, a, b, c, d);
    const uint32_t *p = seg + (w + 256);  // row 1 on: whole rows inside the segment
    for (uint64_t r = 1; r < rows; r += kCrcAhead) {
        u32x4 v[kCrcAhead];
#pragma unroll
        for (uint32_t j = 0; j < kCrcAhead; ++j)
            if (r + j < rows) v[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u *>(p + 256 * j));
#pragma unroll
        for (uint32_t j = 0; j < kCrcAhead; ++j)
            if (r + j < rows) acc = crc_next_row(t, acc) ^ crc_piece(t, v[j].x, v[j].y, v[j].z, v[j].w);
        p += 256 * kCrcAhead;
    }
    acc = crc_mulmod(acc, t.lane[lane]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc ^= (uint32_t)__shfl_xor((int)acc, s, 64);
    return ~acc;
}

// list: n_list directory indices (NULL: 0 .. n_list - 1, the caller passes n_segments).  crc (may be NULL with
// expect): indexed by segment.  expect / bad: the verify form.  No value read from memory is trusted: an index is
// compared with nseg, a segment with the payload (subtractively: off + words cannot wrap past the test).
__global__ __launch_bounds__(256) void k_seg_crc32(const uint32_t *__restrict__ payload, uint64_t payload_words,
                                                   const uint64_t *__restrict__ seg_off, const uint64_t *__restrict__ seg_words,
                                                   uint64_t nseg, const uint64_t *__restrict__ list, uint64_t n_list,
                                                   uint32_t *__restrict__ crc, const uint32_t *__restrict__ expect,
                                                   unsigned long long *bad)
{
    __shared__ CrcTables t;
    static_assert(sizeof(CrcTables) % 16 == 0, "copied in 16-byte pieces");
    {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(&d_crc_tables);
        u32x4 *dst = reinterpret_cast<u32x4 *>(&t);
        for (uint32_t i = threadIdx.x; i < sizeof(CrcTables) / 16; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * kCrcWaves + wave; j < n_list; j += (uint64_t)gridDim.x * kCrcWaves) {
        const uint64_t s = list ? list[j] : j;
        bool readable = s < nseg;
        uint32_t value = 0;
        if (readable) {
            const uint64_t off = seg_off[s], n = seg_words[s];
            readable = n <= payload_words && off <= payload_words - n;
            if (readable && n) value = wave_crc32(t, payload + off, n, lane);
        }
        if (lane == 0) {
            if (crc && s < nseg) crc[s] = value;
            if (expect && (!readable || value != expect[s])) {
                atomicAdd(&bad[0], 1ull);
                atomicMin(&bad[1], (unsigned long long)s);
            }
        }
    }
}

}  // namespace mh
