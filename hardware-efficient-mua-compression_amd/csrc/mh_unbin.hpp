// mh_unbin.hpp -- the kernels of mhi_unbin_count / mhi_unbin_emit (include/muahuff_ingest.h): a matrix of uint8 counts
// back to spike events, the inverse of the binner (mh_ingest.hpp).  Element (i, j) with count k emits k entries, in
// row-major order; the tile rule and the scratch layout are host arithmetic (mh_unbin_layout.hpp).
// Ref: the loaders bin spike times into counts (Data/Load_and_bin_Sabes_store_as_mat_file.m:30-54); this is the way
// back, to the bin's start + phase.
//
//   k_unbin_count      one WAVE per tile (16 wave rows of 1 KiB, 16 bytes per lane and load, unaligned dwordx4 as in
//                      mh_crc.hpp): v_sad_u8 against 0 sums a dword's four counts, a DPP reduction the wave -> sums[t].
//   k_unbin_group_sum  partial[g] = the sum of the 1024 tile sums of group g (below 2^32), 64-bit.
//   k_unbin_scan       ONE workgroup: exclusive scan of the group sums in 64 bits, in place; total[0], the entry behind
//                      the partials and, in the CSR form, ev_off[rows].
//   k_unbin_bases      base[t] = partial[group] + the tiles of the group before t, 64-bit; a tile that begins a CSR row
//                      also writes the row's ev_off.
//   k_unbin_emit       one wave per tile again.  Per wave row: the lane sums, their DPP scan, and every lane writes the
//                      16-bit place (within the tile) of each of its events into the wave's staging array in LDS, at
//                      the scan's position.  The staging holds 2048 events: it takes wave row after wave row and is
//                      stored when the next row would not fit -- sparse data leaves a tile in ONE run of coalesced
//                      stores, 64 consecutive ticks per instruction -- and a row that is larger than the room left
//                      (up to 261 120 events at counts of 255) goes through it in windows: the lanes stage the events
//                      of the window only, the wave stores, the next window follows.  A store turns a place into a
//                      tick (and a channel) as it leaves.
// LDS operations of one wave execute in program order and the staging array is the wave's own: no workgroup barrier,
// no atomic on an output position, no inter-workgroup ordering (wave-scope compiler barriers only).
// Memory safety: the emit pass sizes its staging from ITS OWN loads -- the lane sums it has just taken -- and trusts
// the scratch for the tile's base alone, where every store is compared with `capacity` first: if the input changed
// between the passes the output is unspecified but stays inside out[0 .. capacity).  No byte outside a tile's span is
// loaded: a cut 16-byte piece is read bytewise.
#pragma once
#include "mh_device.hpp"
#include "mh_unbin_layout.hpp"

namespace mh {

constexpr uint32_t kUnbinScanThreads = 1024;
constexpr uint32_t kUnbinBaseThreads = 256;
static_assert(kUnbinBaseThreads * 4 == kUnbinGroup, "a thread of the group kernels owns four tiles");

__device__ __forceinline__ void unbin_wave_phase()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct UnbinSpan {
    const uint8_t *p;  // first byte of the tile
    uint32_t len;      // 1 .. kUnbinTile
    uint32_t row, k;   // CSR form: the row and the tile's number within it
};

// the span of tile t < tiles; uniform over the wave
template <uint32_t FORM>
__device__ __forceinline__ UnbinSpan unbin_span(const uint8_t *__restrict__ in, const uint64_t *__restrict__ row_off,
                                                uint64_t cols, uint32_t tpr, uint64_t total_bytes, uint32_t t)
{
    UnbinSpan s;
    if (FORM == kUnbinCsr) {
        s.row = t / tpr;
        s.k = t - s.row * tpr;
        const uint64_t at = (uint64_t)s.k * kUnbinTile, left = cols - at;
        s.p = in + row_off[s.row] + at;
        s.len = left < kUnbinTile ? (uint32_t)left : kUnbinTile;
    } else {
        s.row = s.k = 0;
        const uint64_t at = (uint64_t)t * kUnbinTile, left = total_bytes - at;
        s.p = in + at;
        s.len = left < kUnbinTile ? (uint32_t)left : kUnbinTile;
    }
    return s;
}

// the 16 bytes at p + off of a span of len bytes; bytes at or behind len read as 0 and are not touched
__device__ __forceinline__ u32x4 unbin_load(const uint8_t *__restrict__ p, uint32_t len, uint32_t off)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (off + 16u <= len) {
        v = *reinterpret_cast<const u32x4_u *>(p + off);
    } else if (off < len) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b)
            if (off + b < len) w[b >> 2] |= (uint32_t)p[off + b] << (8u * (b & 3u));
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    }
    return v;
}

__device__ __forceinline__ uint32_t unbin_sum16(const u32x4 v)
{
    uint32_t s = __builtin_amdgcn_sad_u8(v.x, 0u, 0u);
    s = __builtin_amdgcn_sad_u8(v.y, 0u, s);
    s = __builtin_amdgcn_sad_u8(v.z, 0u, s);
    return __builtin_amdgcn_sad_u8(v.w, 0u, s);
}

template <uint32_t FORM>
__global__ __launch_bounds__(64 * kUnbinWaves) void k_unbin_count(const uint8_t *__restrict__ in,
                                                                  const uint64_t *__restrict__ row_off, uint64_t cols,
                                                                  uint32_t tpr, uint64_t total_bytes, uint32_t tiles,
                                                                  uint32_t *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t64 = (uint64_t)blockIdx.x * kUnbinWaves + wave;
    if (t64 >= tiles) return;  // whole waves leave; nothing below synchronises across waves
    const uint32_t t = (uint32_t)t64;
    const UnbinSpan sp = unbin_span<FORM>(in, row_off, cols, tpr, total_bytes, t);
    uint32_t s = 0;
    if (sp.len == kUnbinTile) {  // a whole tile: every load is issued before the first sum
        u32x4 v[kUnbinTileRows];
#pragma unroll
        for (uint32_t r = 0; r < kUnbinTileRows; ++r)
            v[r] = *reinterpret_cast<const u32x4_u *>(sp.p + r * kUnbinRowBytes + lane * 16u);
#pragma unroll
        for (uint32_t r = 0; r < kUnbinTileRows; ++r) s += unbin_sum16(v[r]);
    } else {
        for (uint32_t r = 0; r * kUnbinRowBytes < sp.len; ++r)
            s += unbin_sum16(unbin_load(sp.p, sp.len, r * kUnbinRowBytes + lane * 16u));
    }
    s = wave_sum_u32(s);
    if (lane == 0) sums[t] = s;
}

__global__ __launch_bounds__(kUnbinBaseThreads) void k_unbin_group_sum(const uint32_t *__restrict__ sums, uint32_t tiles,
                                                                       uint64_t *__restrict__ partial)
{
    __shared__ uint32_t wsum[kUnbinBaseThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * kUnbinGroup + tid * 4u;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i)
        if (t0 + i < tiles) mine += sums[t0 + i];
    mine = wave_sum_u32(mine);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        uint64_t g = 0;
        for (uint32_t w = 0; w < kUnbinBaseThreads / 64; ++w) g += wsum[w];
        partial[blockIdx.x] = g;
    }
}

// ev_off: the CSR form's, or NULL
__global__ __launch_bounds__(kUnbinScanThreads) void k_unbin_scan(uint64_t *__restrict__ partial, uint64_t groups,
                                                                  uint64_t *__restrict__ total, uint64_t *__restrict__ ev_off,
                                                                  uint64_t rows)
{
    __shared__ uint64_t wsum[kUnbinScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry = 0;  // the same in every thread
    for (uint64_t g0 = 0; g0 < groups; g0 += kUnbinScanThreads) {
        const uint64_t g = g0 + tid;
        const uint64_t v = g < groups ? partial[g] : 0ull;  // below 2^32: scanned as two 16-bit halves in 32 bits
        const uint64_t incl = (uint64_t)wave_scan_incl_dpp((uint32_t)v & 0xFFFFu) +
                              ((uint64_t)wave_scan_incl_dpp((uint32_t)(v >> 16)) << 16);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t before = carry + incl - v, all = 0;
        for (uint32_t w = 0; w < kUnbinScanThreads / 64; ++w) {
            const uint64_t x = wsum[w];
            if (w < wave) before += x;
            all += x;
        }
        if (g < groups) partial[g] = before;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        partial[groups] = carry;
        total[0] = carry;
        if (ev_off) ev_off[rows] = carry;
    }
}

// tpr: tiles per row of the CSR form, 0 in the AER form (no ev_off then)
__global__ __launch_bounds__(kUnbinBaseThreads) void k_unbin_bases(const uint32_t *__restrict__ sums, uint32_t tiles,
                                                                   const uint64_t *__restrict__ partial,
                                                                   uint64_t *__restrict__ base, uint32_t tpr,
                                                                   uint64_t *__restrict__ ev_off)
{
    __shared__ uint32_t wsum[kUnbinBaseThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * kUnbinGroup + tid * 4u;
    uint32_t s[4], mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        s[i] = t0 + i < tiles ? sums[t0 + i] : 0u;
        mine += s[i];
    }
    const uint32_t incl = wave_scan_incl_dpp(mine);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t at = partial[blockIdx.x] + (incl - mine);
    for (uint32_t w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (t0 + i < tiles) {
            base[t0 + i] = at;
            if (tpr && ev_off) {
                const uint32_t t = (uint32_t)(t0 + i), row = t / tpr;
                if (row * tpr == t) ev_off[row] = at;
            }
        }
        at += s[i];
    }
}

// The events of one lane's 16 bytes whose number within the wave row lies in [w0, w1) go to stage[shift + number];
// first = the number of the lane's first event, place = the tile-relative place of its first byte.
__device__ __forceinline__ void unbin_stage_lane(uint16_t *stage, const u32x4 v, uint32_t first, uint32_t w0, uint32_t w1,
                                                 int32_t shift, uint32_t place)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t p = first;
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {
        if (w[d] == 0u) continue;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t c = (w[d] >> (8u * b)) & 0xFFu;
            const uint32_t lo = p > w0 ? p : w0, hi = p + c < w1 ? p + c : w1;
            for (uint32_t e = lo; e < hi; ++e) stage[(int32_t)e + shift] = (uint16_t)(place + 4u * d + b);
            p += c;
        }
    }
}

template <uint32_t FORM, typename CH>
__global__ __launch_bounds__(64 * kUnbinWaves) void k_unbin_emit(const uint8_t *__restrict__ in,
                                                                 const uint64_t *__restrict__ row_off, uint64_t cols,
                                                                 uint32_t tpr, uint64_t total_bytes, uint32_t tiles,
                                                                 uint64_t first_tick, uint64_t period,
                                                                 const uint64_t *__restrict__ base,
                                                                 uint64_t *__restrict__ out_ticks, CH *__restrict__ out_ch,
                                                                 uint64_t capacity, unsigned long long *over)
{
    __shared__ uint16_t stage_all[kUnbinWaves][kUnbinStage];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t64 = (uint64_t)blockIdx.x * kUnbinWaves + wave;
    if (t64 >= tiles) return;
    const uint32_t t = (uint32_t)t64;
    uint16_t *const stage = stage_all[wave];
    const UnbinSpan sp = unbin_span<FORM>(in, row_off, cols, tpr, total_bytes, t);
    // what a staged place becomes: CSR tick0 + place * period; AER the element j0 + place of time step i0
    uint64_t tick0, j0 = 0;
    if (FORM == kUnbinCsr) {
        tick0 = first_tick + (uint64_t)sp.k * kUnbinTile * period;
    } else {
        const uint64_t f0 = (uint64_t)t * kUnbinTile, i0 = f0 / cols;
        j0 = f0 - i0 * cols;
        tick0 = first_tick + i0 * period;
    }
    const bool wide = cols >= kUnbinTile;  // AER: then a tile crosses at most one row end
    uint64_t pos = base[t];                // the output position of stage[0]
    uint32_t filled = 0, lost = 0;

    const auto flush = [&]() {
        unbin_wave_phase();
        for (uint32_t i = lane; i < filled; i += 64u) {
            const uint32_t place = stage[i];
            uint64_t tick;
            uint32_t ch = 0;
            if (FORM == kUnbinCsr) {
                tick = tick0 + (uint64_t)place * period;
            } else {
                const uint64_t u = j0 + place;
                uint32_t q;
                if (wide) {
                    q = u >= cols ? 1u : 0u;
                    ch = (uint32_t)(q ? u - cols : u);
                } else {  // u < 2 * kUnbinTile
                    q = (uint32_t)u / (uint32_t)cols;
                    ch = (uint32_t)u - q * (uint32_t)cols;
                }
                tick = tick0 + (uint64_t)q * period;
            }
            const uint64_t o = pos + i;
            if (o < capacity) {
                out_ticks[o] = tick;
                if (FORM == kUnbinAer) out_ch[o] = (CH)ch;
            } else {
                ++lost;
            }
        }
        unbin_wave_phase();
        pos += filled;
        filled = 0;
    };

    // three wave rows are in flight while one is staged (unbin_load gives zeros behind the tile's end and loads nothing)
    u32x4 a = unbin_load(sp.p, sp.len, lane * 16u);
    u32x4 b = unbin_load(sp.p, sp.len, kUnbinRowBytes + lane * 16u);
    u32x4 c = unbin_load(sp.p, sp.len, 2u * kUnbinRowBytes + lane * 16u);
    for (uint32_t r = 0; r * kUnbinRowBytes < sp.len; ++r) {
        const uint32_t place = r * kUnbinRowBytes + lane * 16u;
        const u32x4 v = a;
        a = b;
        b = c;
        c = unbin_load(sp.p, sp.len, place + 3u * kUnbinRowBytes);
        const uint32_t s = unbin_sum16(v);
        const uint32_t incl = wave_scan_incl_dpp(s), first = incl - s;
        const uint32_t all = wave_last(incl);  // at most 64 * 16 * 255
        uint32_t done = 0;                      // events of this wave row that are staged; uniform, as filled
        while (done < all) {
            if (filled == kUnbinStage) flush();
            const uint32_t room = kUnbinStage - filled, take = all - done < room ? all - done : room;
            if (s && first < done + take && first + s > done)
                unbin_stage_lane(stage, v, first, done, done + take, (int32_t)filled - (int32_t)done, place);
            filled += take;
            done += take;
        }
    }
    flush();
    lost = wave_sum_u32(lost);
    if (lane == 0 && lost) atomicAdd(over, (unsigned long long)lost);
}

}  // namespace mh
