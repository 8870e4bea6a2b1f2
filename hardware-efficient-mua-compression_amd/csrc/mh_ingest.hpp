// mh_ingest.hpp -- the front-end kernel of libmuahuff_ingest.so (include/muahuff_ingest.h).
//
//   k_bin_events<BITS>  per-channel sorted event time stamps (CSR) -> binned counts, as bytes (BITS = 8, min(n, 255)) or
//                       directly as the packed 4- / 2-bit pieces of the stream path (min(n, 15) / min(n, 3)), in the
//                       layout k_deinterleave_p writes (mh_layout.hpp), contiguous or chunk-blocked.
//                       Ref: Data/Load_and_bin_Sabes_store_as_mat_file.m:30-54 (histogram2 + uint8()) and the RTL's
//                       binner_f (FPGA implementation/1_binner_final.v:19-21), in the RTL's integer ticks.
//
// A workgroup owns `span` consecutive 16384-bin chunks of ONE channel -- a chunk is the unit of the chunk-blocked layout,
// so each is one contiguous output region in either layout -- and walks the channel's event list once:
//   start   : the first event at or after the span's first tick, by ONE cooperative 256-ary search (each thread probes the
//             end of its 256th of the range, a ballot count narrows it: three rounds for 1e7 events where a binary
//             search takes 24 dependent loads).  Later chunks need no search: the list is sorted, the cursor is there.
//   pass    : 256 events from the cursor, one per thread (coalesced 8-byte loads).  An event is IN the chunk when
//             ts <= tick < te, the chunk's tick bounds (origin + b * period: no division per probe); its bin is
//             (tick - ts) / period -- exact: a subtraction for period 1, a 32-bit divide while 16384 * period < 2^32,
//             else a 64-bit divide (events are sparse).  The in-chunk events of a pass are a prefix of it, their count
//             (ballots + four LDS words) advances the cursor, and a pass that is not full ends the chunk.
//   count   : equal bins are consecutive.  The LAST event of a run (bin != next lane's) knows the run's first event -- the
//             highest head (bin != previous lane's) at or below it in the wave's ballot, or, for a run that began in an
//             earlier wave, a binary search of the pass's bins in LDS -- and adds the run length to the bin's byte
//             counter in the LDS tile, saturating at the cap: one plain byte read-modify-write per bin and pass, no
//             atomics (no two runs of a pass share a bin), no packed adds that could carry.  A run that straddles two
//             passes adds twice, a barrier apart.
//   store   : the tile leaves as whole 16-byte vectors per lane, packed in registers for 4 / 2 bits, and is zeroed on
//             the way; only a cut last vector is written in dwords (bytes for BITS = 8).  A chunk without events never
//             touches the tile: zeros from registers.  Plain stores: the encoder reads the pieces next.
// Unsorted input: every index and every bin is range-checked on its own, so stores stay in the chunk's region; counts
// are then whatever the run logic makes of it.
#pragma once
#include "mh_device.hpp"

namespace mh {

constexpr uint32_t kBinThreads = 256;
constexpr uint32_t kBinNone = 0xFFFFFFFFu;  // the "bin" of a lane without an in-chunk event

struct BinLds {
    uint32_t tile[kChunk / 4];        // one byte counter per bin of the chunk
    uint32_t bins[2][kBinThreads];    // the bins of a pass (double-buffered: one barrier per pass)
    uint32_t cnt[2][kBinThreads / 64];
};

// sum of a per-lane predicate over the workgroup; one barrier, `par` picks the buffer and flips
__device__ __forceinline__ uint32_t bin_group_count(BinLds &s, bool p, uint32_t &par)
{
    const unsigned long long m = __ballot(p);
    if ((threadIdx.x & 63u) == 0) s.cnt[par][threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    const uint32_t n = s.cnt[par][0] + s.cnt[par][1] + s.cnt[par][2] + s.cnt[par][3];
    par ^= 1u;
    return n;
}

// first index in [lo, hi) whose tick is >= x (hi if none), found by the whole workgroup
__device__ __forceinline__ uint64_t bin_lower_bound(const uint64_t *__restrict__ ticks, uint64_t lo, uint64_t hi, uint64_t x,
                                                    BinLds &s, uint32_t &par)
{
    while (hi > lo) {
        const uint64_t step = (hi - lo + kBinThreads - 1) / kBinThreads;
        const uint64_t idx = lo + (uint64_t)(threadIdx.x + 1) * step - 1;  // last element of this thread's part
        const uint32_t below = bin_group_count(s, idx < hi && ticks[idx] < x, par);
        lo = lo + below * step < hi ? lo + below * step : hi;
        hi = lo + step - 1 < hi ? lo + step - 1 : hi;  // that part's last element is >= x (or past the end)
    }
    return lo;
}

__device__ __forceinline__ uint32_t pack_nibbles(uint32_t d)  // four bytes <= 15 -> 16 bits
{
    d = (d | (d >> 4)) & 0x00FF00FFu;
    return (d | (d >> 8)) & 0xFFFFu;
}

__device__ __forceinline__ uint32_t pack_crumbs(uint32_t d)  // four bytes <= 3 -> 8 bits
{
    d = (d | (d >> 6)) & 0x000F000Fu;
    return (d | (d >> 12)) & 0xFFu;
}

__device__ __forceinline__ uint32_t pack_nibbles2(uint32_t a, uint32_t b) { return pack_nibbles(a) | (pack_nibbles(b) << 16); }
__device__ __forceinline__ uint32_t pack_crumbs4(u32x4 v)
{
    return pack_crumbs(v.x) | (pack_crumbs(v.y) << 8) | (pack_crumbs(v.z) << 16) | (pack_crumbs(v.w) << 24);
}

// the chunk's nb bins -> dst; any = false: the tile was not touched (all zeros)
template <int BITS>
__device__ __forceinline__ void bin_store_chunk(BinLds &s, bool any, uint8_t *__restrict__ dst, uint32_t nb)
{
    constexpr uint32_t kVecs = 8 / BITS;  // 16-byte LDS vectors of counters behind 16 output bytes
    const uint32_t out_bytes = BITS == 8 ? nb : ((nb + 15u) >> 4) * (2u * BITS);
    const uint32_t items = (out_bytes + 15u) >> 4;
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (uint32_t it = threadIdx.x; it < items; it += kBinThreads) {
        u32x4 o = z;
        if (any) {
            u32x4 *p = reinterpret_cast<u32x4 *>(s.tile) + it * kVecs;
            u32x4 v[kVecs];
#pragma unroll
            for (uint32_t k = 0; k < kVecs; ++k) {
                v[k] = p[k];
                p[k] = z;
            }
            if constexpr (BITS == 8) {
                o = v[0];
            } else if constexpr (BITS == 4) {
                o.x = pack_nibbles2(v[0].x, v[0].y);
                o.y = pack_nibbles2(v[0].z, v[0].w);
                o.z = pack_nibbles2(v[1].x, v[1].y);
                o.w = pack_nibbles2(v[1].z, v[1].w);
            } else {
                o.x = pack_crumbs4(v[0]);
                o.y = pack_crumbs4(v[1]);
                o.z = pack_crumbs4(v[2]);
                o.w = pack_crumbs4(v[3]);
            }
        }
        const uint32_t off = it << 4, n = out_bytes - off;
        if (n >= 16u) {
            *reinterpret_cast<u32x4_u *>(dst + off) = o;
        } else if (BITS == 8) {  // the channel's last bins: bytes
            for (uint32_t k = 0; k < n; ++k) dst[off + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
        } else {                 // the last piece(s): 4 / 8 / 12 bytes
            for (uint32_t k = 0; k < (n >> 2); ++k) *reinterpret_cast<uint32_t *>(dst + off + 4 * k) = o[k];
        }
    }
}

// div_mode: 0 = period 1, 1 = 16384 * period < 2^32, 2 = any period
template <int BITS>
__global__ __launch_bounds__(256) void k_bin_events(const uint64_t *__restrict__ ticks, const uint64_t *__restrict__ ev_off,
                                                    uint64_t origin, uint64_t period, uint64_t T, uint64_t nchunks,
                                                    uint64_t span, uint64_t nspans, uint32_t div_mode,
                                                    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                                                    uint64_t chunk_stride)
{
    constexpr uint32_t kCap = (1u << BITS) - 1u;
    __shared__ __attribute__((aligned(16))) BinLds s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t ch = blockIdx.x / nspans, sp = blockIdx.x % nspans;
    const uint64_t e0 = ev_off[ch];
    const uint64_t e1 = ev_off[ch + 1] > e0 ? ev_off[ch + 1] : e0;
    const uint64_t j0 = sp * span, j1 = j0 + span < nchunks ? j0 + span : nchunks;
    uint8_t *const base = out + out_off[ch];
    const uint64_t stride = chunk_stride ? chunk_stride : (uint64_t)kChunk * BITS / 8;

    const u32x4 z = {0u, 0u, 0u, 0u};
    for (uint32_t i = tid; i < (uint32_t)kChunk / 16; i += kBinThreads) reinterpret_cast<u32x4 *>(s.tile)[i] = z;
    uint32_t par = 0;
    // (with events in the channel the search passes at least one barrier: the zeroed tile is in place before any count)
    uint64_t cursor = bin_lower_bound(ticks, e0, e1, origin + j0 * kChunk * period, s, par);

    for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t b0 = j * kChunk;
        const uint32_t nb = T - b0 < (uint64_t)kChunk ? (uint32_t)(T - b0) : (uint32_t)kChunk;
        const uint64_t ts = origin + b0 * period, te = ts + (uint64_t)nb * period;  // <= origin + T * period <= 2^63
        bool any = false;
        for (;;) {
            const uint64_t i = cursor + tid;
            uint32_t bin = kBinNone;
            if (i < e1) {
                const uint64_t tk = ticks[i];
                if (tk >= ts && tk < te) {
                    const uint64_t rel = tk - ts;
                    const uint32_t q = div_mode == 0 ? (uint32_t)rel
                                     : div_mode == 1 ? (uint32_t)rel / (uint32_t)period
                                                     : (uint32_t)(rel / period);
                    if (q < nb) bin = q;
                }
            }
            const bool v = bin != kBinNone;
            uint32_t *const pb = s.bins[par];
            pb[tid] = bin;
            const uint32_t nvalid = bin_group_count(s, v, par);  // barrier: the pass's bins are in LDS
            if (nvalid) {
                any = true;
                const uint32_t prev = tid ? pb[tid - 1] : kBinNone, next = tid + 1 < kBinThreads ? pb[tid + 1] : kBinNone;
                const unsigned long long heads = __ballot(v && bin != prev);
                if (v && bin != next) {  // last event of a run
                    const unsigned long long below = heads & (~0ull >> (63u - lane));
                    uint32_t first;
                    if (below) {
                        first = wave * 64u + 63u - (uint32_t)__clzll((long long)below);
                    } else {  // the run began in an earlier wave of the pass
                        uint32_t lo = 0, hi = wave * 64u;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (pb[mid] < bin)
                                lo = mid + 1;
                            else
                                hi = mid;
                        }
                        first = lo;
                    }
                    uint8_t *const cell = reinterpret_cast<uint8_t *>(s.tile) + bin;
                    const uint32_t sum = (uint32_t)*cell + (tid - first + 1u);
                    *cell = (uint8_t)(sum > kCap ? kCap : sum);
                }
            }
            cursor += nvalid;
            if (nvalid < kBinThreads) break;
        }
        if (any) __syncthreads();  // every count of the chunk is in the tile
        bin_store_chunk<BITS>(s, any, base + j * stride, nb);
        // (the zeros written back are ordered before the next chunk's counts by that chunk's first pass barrier)
    }
}

}  // namespace mh
