// mh_packed_measure.hpp -- mh_measure on the PACKED pieces of a packed plan (mh_plan_create_packed): the window and
// calibration histograms counted straight from the 2- / 4-bit fields, never through byte-per-sample form.
//
//   k_hist_packed<2, 3>    2-bit pieces (S <= 4): per dword n1 = fields with bit 0 set, n2 = bit 1 set, n3 = both -- two
//                          masks, one and, three v_bcnt_u32_b32 (7 VALU ops per 16 samples, whatever S); the bins follow
//                          per TILE: #0 = n - n1 - n2 + n3, #1 = n1 - n3, #2 = n2 - n3
//   k_hist_packed<4, NS>   4-bit pieces, NS = S - 1 counted levels: "nibble != s" flags at bit 3 of every nibble, built
//                          from four low-bit-pair terms and three high-bit-pair terms shared by all levels (12 ops), then
//                          one or and one v_bcnt per level: 12 + 2 * NS ops per 8 samples (S = 5: 17 after dead terms)
// Both read 16 bytes per lane and request a batch of eight vectors before the first is counted, reduce per wave with
// the DPP ladder (wave_sum_u32) and add bins 0 .. S-2 of the tile to hist[channel]; the top bin is the window length
// minus the rest, as in the byte kernels (k_finalize, calibrate_channel's pre_hist form).  Tiles are the planner's
// (kHistTileBytes samples = 8 chunks, chunk-aligned), so a tile is whole chunks -- `stride` bytes apart -- plus at most
// one cut chunk at the end of the channel.  The cut chunk is read dword by dword: only dwords of pieces that exist, and
// the padding fields of the last piece are masked out before counting (mh_deinterleave_packed zero-pads them; a
// caller's own pieces may hold anything there).
#pragma once
#include "mh_kernels.hpp"

namespace mh {

typedef uint32_t u32_u __attribute__((aligned(1)));

struct PackedHistArgs {
    const uint8_t *data;
    const uint64_t *ch_off;
    const uint32_t *tile_ch;
    const uint64_t *tile_start;  // samples from the channel's first one, a multiple of MH_CHUNK
    const uint32_t *tile_n;      // samples (<= kHistTileBytes)
    unsigned long long *hist;    // [C][kHistStride], zeroed before the launch
    uint64_t stride;             // bytes between consecutive chunks of a channel (chunk_stride, or the chunk's own size)
    uint32_t S;
};

// 16 two-bit fields: acc = {n1, n2, n3}
__host__ __device__ __forceinline__ void count_fields2(uint32_t x, uint32_t (&acc)[3])
{
    const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
    acc[0] += (uint32_t)__builtin_popcount(lo);
    acc[1] += (uint32_t)__builtin_popcount(hi);
    acc[2] += (uint32_t)__builtin_popcount(lo & hi);
}

// 8 nibbles: acc[s] += 32 - #(nibble == s).  Flag bit = bit 3 of a nibble, set when the nibble differs from s; every
// other bit of the word is forced to 1 (the constant 24), which saves masking each level.
template <int NS>
__host__ __device__ __forceinline__ void count_nibbles(uint32_t x, uint32_t (&acc)[NS])
{
    const uint32_t nx = ~x;
    const uint32_t x3 = x << 3, nx3 = nx << 3;
    const uint32_t lo[4] = {(x << 2) | x3, (x << 2) | nx3, (nx << 2) | x3, (nx << 2) | nx3};  // bits 1..0 differ from 0..3
    const uint32_t xm = x | 0x77777777u, nxm = nx | 0x77777777u;
    const uint32_t hi[3] = {(x << 1) | xm, (nx << 1) | xm, (x << 1) | nxm};                    // bits 3..2 differ from 0..2
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] += (uint32_t)__builtin_popcount(lo[s & 3] | hi[s >> 2]);
}

template <int BITS, int NS>
__global__ __launch_bounds__(256) void k_hist_packed(PackedHistArgs a)
{
    static_assert((BITS == 2 && NS == 3) || (BITS == 4 && NS >= 1 && NS <= 9), "2-bit: {n1, n2, n3}; 4-bit: levels 0 .. S-2");
    constexpr uint32_t kVecSamples = 128 / BITS;                      // samples of one 16-byte vector: 64 / 32
    constexpr uint32_t kRowsPerChunk = MH_CHUNK / kVecSamples / 256;  // vectors per thread and chunk: 1 / 2
    constexpr uint32_t kDwSamples = 32 / BITS;
    constexpr uint32_t kBatch = 8;
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t ch = a.tile_ch[tile];
    const uint32_t n = a.tile_n[tile];
    const uint8_t *base = a.data + a.ch_off[ch] + (a.tile_start[tile] / MH_CHUNK) * a.stride;
    const uint32_t nfull = n / MH_CHUNK, rem = n % MH_CHUNK;
    const uint32_t nrows = nfull * kRowsPerChunk;  // <= 8 / 16
    uint32_t acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0;
    uint32_t ndw = nrows * 4;  // dwords this thread counts (4-bit: what the level counters are subtracted from)
    for (uint32_t r0 = 0; r0 < nrows; r0 += kBatch) {
        u32x4 xs[kBatch];
#pragma unroll
        for (uint32_t u = 0; u < kBatch; ++u) {
            const uint32_t r = r0 + u < nrows ? r0 + u : r0;  // (past the end: row r0 again, not counted)
            const uint8_t *q = base + (uint64_t)(r / kRowsPerChunk) * a.stride + ((r % kRowsPerChunk) * 256u + tid) * 16u;
            xs[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u *>(q));
        }
#pragma unroll
        for (uint32_t u = 0; u < kBatch; ++u)
            if (r0 + u < nrows) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    if constexpr (BITS == 2) count_fields2(xs[u][d], acc);
                    else count_nibbles<NS>(xs[u][d], acc);
                }
            }
    }
    if (rem) {  // the channel's cut last chunk
        const uint8_t *cb = base + (uint64_t)nfull * a.stride;
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerChunk; ++k) {
            const uint32_t v = k * 256u + tid, s0 = v * kVecSamples;
            if (s0 < rem) {
                const uint32_t nv = rem - s0 < kVecSamples ? rem - s0 : kVecSamples;
                const u32_u *w = reinterpret_cast<const u32_u *>(cb + (size_t)v * 16u);
#pragma unroll
                for (uint32_t d = 0; d < 4; ++d)
                    if (d * kDwSamples < nv) {  // the dword's piece holds a sample: it exists
                        const uint32_t m = nv - d * kDwSamples;  // its samples (>= 1); fields behind them are padding
                        uint32_t x = w[d];
                        if (m < kDwSamples) {
                            const uint32_t valid = (1u << (m * BITS)) - 1u;
                            x = BITS == 2 ? x & valid : x | ~valid;  // padding counts as 0 resp. 15: in no counter
                        }
                        if constexpr (BITS == 2) count_fields2(x, acc);
                        else count_nibbles<NS>(x, acc);
                        ++ndw;
                    }
            }
        }
    }
    if constexpr (BITS == 4) {
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = 32u * ndw - acc[s];
    }
    __shared__ uint32_t red[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t v = wave_sum_u32(acc[s]);
        if ((tid & 63) == 0) red[s][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < a.S - 1 && tid < (uint32_t)NS) {
        uint32_t t[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) t[s] = red[s][0] + red[s][1] + red[s][2] + red[s][3];
        uint32_t v = 0;
        if constexpr (BITS == 2) {
            v = tid == 0 ? n - t[0] - t[1] + t[2] : tid == 1 ? t[0] - t[2] : t[1] - t[2];
        } else {
#pragma unroll
            for (int s = 0; s < NS; ++s) v = (uint32_t)s == tid ? t[s] : v;
        }
        if (v) hist_add(&a.hist[(size_t)ch * kHistStride + tid], v, false);
    }
}

}  // namespace mh
