// mh_aer.hpp -- the kernels of mhi_aer_to_csr (include/muahuff_ingest.h): a stable partition of a merged list of
// (tick, channel) pairs by channel, the form the binner reads.  One digit (the channel), so count / scan / scatter
// and no general sort; the tile rule and the scratch layout are host arithmetic (mh_aer_layout.hpp).
// Ref: the merged MUA_vec of the loaders (Data/Load_and_bin_Sabes_store_as_mat_file.m), which histogram2 bins by
// channel; here the list is first brought into the per-channel form of mhi_bin_events.
//
//   k_aer_count<CH>    one WAVE per sub-run of W pairs (row r of the count matrix): zeroes its own C counters in LDS,
//                      reads the channel column only -- 16 bytes per lane and load -- adds with ds_add_u32, and writes
//                      the row.  Pairs whose channel is >= C are counted per row (drop[r]) and nowhere else.
//   k_aer_group_sum    partial[g][c] = sum of the rows of group g (64 rows), thread = channel: coalesced row reads.
//   k_aer_scan         ONE workgroup: per channel an exclusive scan of the partials over the groups (in place) and the
//                      channel's total (kept in the row behind the partials); an exclusive scan of the totals over
//                      the channels -> ev_off[0..C]; the sum of drop[] -> dropped[0].  With n == 0 this is the only kernel launched.
//   k_aer_bases        row r of the matrix becomes the output position of the row's first pair of each channel:
//                      ev_off[c] + partial[g][c] + the rows of the group before r.  Thread = channel again.
//   k_aer_scatter<CH>  one wave per sub-run, as in the count: its row of positions is its cursor array in LDS, and it
//                      walks the sub-run 64 pairs at a time, in order.  The lanes that hold the same channel are found
//                      with ceil(log2 C) ballots; a pair goes to cursor + (lower lanes of its group), the group's
//                      highest lane advances the cursor by the group's size.  LDS operations of one wave execute in
//                      program order, the cursors are the wave's own, and rows are disjoint by the scan: no workgroup
//                      barrier, no atomic, no device fence (wave-scope compiler barriers only), and the order inside a channel is the input order.  The next step's pair is
//                      loaded before the current one is ranked.
// Memory safety: a tick is never looked at.  Every index is formed from a channel that was compared with C first and
// from counts of such channels, the SAME comparison in both passes over the same column; an unsorted list is
// partitioned like any other.  Positions are 32-bit (n < 2^32, checked on the host).
#pragma once
#include "mh_device.hpp"

namespace mh {

constexpr uint32_t kAerScanThreads = 1024;
constexpr uint32_t kAerColThreads = 256;

template <typename CH>
__device__ __forceinline__ uint32_t aer_load_channel(const CH *__restrict__ ch, uint64_t i)
{
    return (uint32_t)ch[i];
}

// the compiler must not move LDS accesses of the wave's phases across each other (the hardware keeps their order)
__device__ __forceinline__ void aer_wave_phase()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <typename CH>
__global__ __launch_bounds__(256) void k_aer_count(const CH *__restrict__ channels, uint64_t n, uint32_t C, uint32_t run,
                                                   uint64_t rows, uint32_t *__restrict__ matrix,
                                                   uint32_t *__restrict__ drop)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t aer_lds[];
    constexpr uint32_t kPer = 16 / sizeof(CH);  // channels per 16-byte load
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint64_t row = (uint64_t)blockIdx.x * waves + wave;
    if (row >= rows) return;  // whole waves leave; nothing below synchronises across waves
    uint32_t *const cnt = aer_lds + (size_t)wave * C;
    for (uint32_t c = lane; c < C; c += 64u) cnt[c] = 0u;
    aer_wave_phase();
    const uint64_t s = row * run, e = s + run < n ? s + run : n;
    uint32_t bad = 0;
    uint64_t i = s + (uint64_t)lane * kPer;
    for (; i + kPer <= e; i += 64u * kPer) {
        const u32x4 v = *reinterpret_cast<const u32x4_u *>(channels + i);
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t w = v[k * sizeof(CH) / 4];
            const uint32_t c = sizeof(CH) == 2 ? (w >> (16u * (k & 1u))) & 0xFFFFu : w;
            if (c < C)
                atomicAdd(&cnt[c], 1u);
            else
                ++bad;
        }
    }
    for (; i < e; ++i) {  // the cut vector of the list's end: one lane
        const uint32_t c = aer_load_channel(channels, i);
        if (c < C)
            atomicAdd(&cnt[c], 1u);
        else
            ++bad;
    }
    aer_wave_phase();
    uint32_t *const out = matrix + row * C;
    for (uint32_t c = lane; c < C; c += 64u) out[c] = cnt[c];
    bad = wave_sum_u32(bad);
    if (lane == 0) drop[row] = bad;
}

__global__ __launch_bounds__(256) void k_aer_group_sum(const uint32_t *__restrict__ matrix, uint32_t C, uint64_t rows,
                                                       uint32_t group_rows, uint32_t *__restrict__ partial)
{
    const uint32_t c = blockIdx.x * kAerColThreads + threadIdx.x;
    if (c >= C) return;
    const uint64_t g = blockIdx.y, r0 = g * group_rows, r1 = r0 + group_rows < rows ? r0 + group_rows : rows;
    uint32_t sum = 0;
    for (uint64_t r = r0; r < r1; ++r) sum += matrix[r * C + c];
    partial[g * C + c] = sum;
}

__global__ __launch_bounds__(1024) void k_aer_scan(uint32_t *__restrict__ partial, const uint32_t *__restrict__ drop,
                                                   uint32_t C, uint64_t rows, uint64_t groups,
                                                   uint64_t *__restrict__ ev_off, uint64_t *__restrict__ dropped)
{
    uint32_t *const total = partial + groups * C;  // the row behind the partials (mh_aer_layout.hpp), this workgroup's own
    __shared__ uint32_t wsum[kAerScanThreads / 64];
    __shared__ uint32_t wdrop[kAerScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t c = tid; c < C; c += kAerScanThreads) {
        uint32_t run = 0;
        for (uint64_t g = 0; g < groups; ++g) {
            const uint32_t t = partial[g * C + c];
            partial[g * C + c] = run;
            run += t;
        }
        total[c] = run;
    }
    uint32_t bad = 0;
    for (uint64_t r = tid; r < rows; r += kAerScanThreads) bad += drop[r];
    bad = wave_sum_u32(bad);
    if (lane == 0) wdrop[wave] = bad;
    __syncthreads();
    // thread t owns channels [t * per, (t + 1) * per): its sum, a scan over the workgroup, then its channels in order
    const uint32_t per = (C + kAerScanThreads - 1) / kAerScanThreads;
    const uint32_t c0 = tid * per < C ? tid * per : C, c1 = c0 + per < C ? c0 + per : C;
    uint32_t mine = 0;
    for (uint32_t c = c0; c < c1; ++c) mine += total[c];
    const uint32_t incl = wave_scan_incl_dpp(mine);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    for (uint32_t c = c0; c < c1; ++c) {
        ev_off[c] = before;
        before += total[c];
    }
    if (tid == kAerScanThreads - 1) {  // it has passed every channel, owned or not
        ev_off[C] = before;
        uint64_t d = 0;
        for (uint32_t w = 0; w < kAerScanThreads / 64; ++w) d += wdrop[w];
        dropped[0] = d;
    }
}

__global__ __launch_bounds__(256) void k_aer_bases(uint32_t *__restrict__ matrix, const uint32_t *__restrict__ partial,
                                                   const uint64_t *__restrict__ ev_off, uint32_t C, uint64_t rows,
                                                   uint32_t group_rows)
{
    const uint32_t c = blockIdx.x * kAerColThreads + threadIdx.x;
    if (c >= C) return;
    const uint64_t g = blockIdx.y, r0 = g * group_rows, r1 = r0 + group_rows < rows ? r0 + group_rows : rows;
    uint32_t pos = (uint32_t)ev_off[c] + partial[g * C + c];
    for (uint64_t r = r0; r < r1; ++r) {
        const uint32_t t = matrix[r * C + c];
        matrix[r * C + c] = pos;
        pos += t;
    }
}

template <typename CH>
__global__ __launch_bounds__(256) void k_aer_scatter(const uint64_t *__restrict__ ticks, const CH *__restrict__ channels,
                                                     uint64_t n, uint32_t C, uint32_t nbits, uint32_t run, uint64_t rows,
                                                     const uint32_t *__restrict__ matrix, uint64_t *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t aer_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint64_t row = (uint64_t)blockIdx.x * waves + wave;
    if (row >= rows) return;
    uint32_t *const cur = aer_lds + (size_t)wave * C;
    const uint32_t *const base = matrix + row * C;
    for (uint32_t c = lane; c < C; c += 64u) cur[c] = base[c];
    aer_wave_phase();
    const uint64_t s = row * run, e = s + run < n ? s + run : n;
    const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
    uint64_t i = s + lane;
    uint32_t ch = i < e ? aer_load_channel(channels, i) : 0xFFFFFFFFu;
    uint64_t tk = i < e ? ticks[i] : 0ull;
    for (uint64_t at = s; at < e; at += 64u) {  // `at` is the same in every lane: the ballots are wave-wide
        const uint32_t c = ch;
        const uint64_t t = tk;
        i += 64u;
        ch = i < e ? aer_load_channel(channels, i) : 0xFFFFFFFFu;
        tk = i < e ? ticks[i] : 0ull;
        const bool ok = c < C;  // also false for the lanes past the end
        unsigned long long same = __ballot(ok);
        for (uint32_t b = 0; b < nbits; ++b) {
            const bool bit = (c >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        if (ok) {
            const uint32_t p = cur[c] + (uint32_t)__popcll(same & below);
            out[p] = t;
            if ((same & ~upto) == 0ull) cur[c] = p + 1u;  // the group's highest lane: cursor + size of the group
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace mh
