// mh_excess.hpp -- the kernels of mhi_excess_count / mhi_excess_emit / mhi_excess_apply (include/muahuff_ingest.h): what
// the codec's clip at S-1 drops, kept as a sparse list.  An element x > threshold of channel c at sample p is the entry
// (pos = p, val = x - threshold); the list is channel-major, ascending in pos inside a channel, with a CSR index.
// Ref: the clip itself is the reference's (Compressing data/get_BR_with_approx_sort.py:143,164 price min(x, S-1)); the
// side list is this project's.  The piece rule and the scratch layout are host arithmetic (mh_excess_layout.hpp); the
// scan between the passes is mh_unbin.hpp's (k_unbin_group_sum, k_unbin_scan, k_unbin_bases) on the pieces' counts.
//
//   k_excess_rows_count  one WAVE per tile of a channel's row (16 wave rows of 1 KiB, unaligned dwordx4 loads, the cut
//                        tail bytewise, as k_unbin_count): a byte-parallel compare leaves 0x80 in every byte above the
//                        threshold, v_bcnt counts them, a DPP reduction sums the wave -> sums[t].
//   k_excess_rows_emit   one wave per tile again.  Per wave row one vote: no lane has a byte above the threshold -> next
//                        row.  Otherwise the lane counts, their DPP scan, and every lane stores its entries at the
//                        tile's base + the rows before + the scan's position.
//   k_excess_cols_count  one wave per (strip of 256 channels, time tile of 512 steps) of a time-major block: a lane
//                        reads the dword of its four channels at every step and keeps four 16-bit counters ->
//                        sums[channel * time_tiles + time_tile], the cells in channel-major order.
//   k_excess_cols_emit   the same walk; a lane stores the entries of its four cells at their bases.  No cross-lane
//                        operation: a lane whose dword has no byte above the threshold does nothing for the step.
//   k_excess_apply1      r == 1: a thread per entry of a row adds val to the byte (or int32) it alone owns.
//   k_excess_apply       r > 1: a thread per run of 32 output elements of a row searches the row's sorted entries for
//                        the run's first position and walks them to its end: every element has one owner, so no atomic
//                        and the same result from run to run.
// Memory safety: every emit store is compared with `capacity` first, and the bases are all the emit kernels take from
// the scratch -- if the input changed between the passes the output is unspecified but stays inside [0, capacity).  The
// apply kernels clamp first / last to n_entries, compare pos with [start, stop) before an address is formed from it,
// and a thread of k_excess_apply stores to the elements of its own run only.
#pragma once
#include "mh_device.hpp"
#include "mh_excess_layout.hpp"
#include "mh_unbin.hpp"

namespace mh {

typedef uint32_t u32_u __attribute__((aligned(1)));

// 0x80 in every byte of w that is above the threshold.  k = (255 - threshold) in every byte: x > threshold <=> x + k
// carries out of the byte, and the carry out of bit 7 is the majority of x7, k7 and the carry into bit 7 -- which is
// bit 7 of the sum of the low seven bits, a sum that cannot leave its byte.
__device__ __forceinline__ uint32_t excess_mask(uint32_t w, uint32_t k)
{
    const uint32_t low = (w & 0x7F7F7F7Fu) + (k & 0x7F7F7F7Fu);
    return ((w & k) | ((w | k) & low)) & 0x80808080u;
}

struct ExcessSpan {
    const uint8_t *p;  // first byte examined
    uint32_t len;      // 0 .. kUnbinTile
    uint32_t col0;     // the column of p[0]
};

// tile t < pieces of the ROWS form: the columns of tile k of its row that lie in [lo[row], min(hi[row], cols));
// uniform over the wave
__device__ __forceinline__ ExcessSpan excess_span(const uint8_t *__restrict__ in, const uint64_t *__restrict__ row_off,
                                                  const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                  uint64_t cols, uint32_t tpr, uint32_t t)
{
    const uint32_t row = t / tpr, k = t - row * tpr;
    uint64_t a = (uint64_t)k * kUnbinTile, b = a + kUnbinTile;
    uint64_t h = hi ? hi[row] : cols;
    const uint64_t l = lo ? lo[row] : 0ull;
    if (h > cols) h = cols;
    if (b > h) b = h;
    if (a < l) a = l;
    ExcessSpan s;
    s.len = b > a ? (uint32_t)(b - a) : 0u;
    s.col0 = (uint32_t)a;  // only used with len > 0, where a < cols < 2^32
    s.p = in + row_off[row] + a;
    return s;
}

__device__ __forceinline__ uint32_t excess_count16(const u32x4 v, uint32_t k)
{
    uint32_t s = (uint32_t)__builtin_popcount(excess_mask(v.x, k));
    s += (uint32_t)__builtin_popcount(excess_mask(v.y, k));
    s += (uint32_t)__builtin_popcount(excess_mask(v.z, k));
    return s + (uint32_t)__builtin_popcount(excess_mask(v.w, k));
}

__global__ __launch_bounds__(64 * kExcessWaves) void k_excess_rows_count(const uint8_t *__restrict__ in,
                                                                         const uint64_t *__restrict__ row_off,
                                                                         const uint64_t *__restrict__ lo,
                                                                         const uint64_t *__restrict__ hi, uint64_t cols,
                                                                         uint32_t tpr, uint32_t tiles, uint32_t k,
                                                                         uint32_t *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t64 = (uint64_t)blockIdx.x * kExcessWaves + wave;
    if (t64 >= tiles) return;  // whole waves leave; nothing below synchronises across waves
    const uint32_t t = (uint32_t)t64;
    const ExcessSpan sp = excess_span(in, row_off, lo, hi, cols, tpr, t);
    uint32_t s = 0;
    if (sp.len == kUnbinTile) {  // a whole tile: every load is issued before the first compare
        u32x4 v[kUnbinTileRows];
#pragma unroll
        for (uint32_t r = 0; r < kUnbinTileRows; ++r)
            v[r] = *reinterpret_cast<const u32x4_u *>(sp.p + r * kUnbinRowBytes + lane * 16u);
#pragma unroll
        for (uint32_t r = 0; r < kUnbinTileRows; ++r) s += excess_count16(v[r], k);
    } else {
        for (uint32_t r = 0; r * kUnbinRowBytes < sp.len; ++r)
            s += excess_count16(unbin_load(sp.p, sp.len, r * kUnbinRowBytes + lane * 16u), k);  // behind len: zeros
    }
    s = wave_sum_u32(s);
    if (lane == 0) sums[t] = s;
}

__global__ __launch_bounds__(64 * kExcessWaves) void k_excess_rows_emit(const uint8_t *__restrict__ in,
                                                                        const uint64_t *__restrict__ row_off,
                                                                        const uint64_t *__restrict__ lo,
                                                                        const uint64_t *__restrict__ hi, uint64_t cols,
                                                                        uint32_t tpr, uint32_t tiles, uint32_t k,
                                                                        uint32_t threshold, const uint64_t *__restrict__ base,
                                                                        uint32_t *__restrict__ out_pos,
                                                                        uint8_t *__restrict__ out_val, uint64_t capacity,
                                                                        unsigned long long *over)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t64 = (uint64_t)blockIdx.x * kExcessWaves + wave;
    if (t64 >= tiles) return;
    const uint32_t t = (uint32_t)t64;
    const ExcessSpan sp = excess_span(in, row_off, lo, hi, cols, tpr, t);
    if (sp.len == 0) return;
    uint64_t at = base[t];  // the output position of the wave row's first entry; uniform
    uint32_t lost = 0;
    // three wave rows are in flight while one is examined (unbin_load gives zeros behind the span's end, loads nothing)
    u32x4 a = unbin_load(sp.p, sp.len, lane * 16u);
    u32x4 b = unbin_load(sp.p, sp.len, kUnbinRowBytes + lane * 16u);
    u32x4 c = unbin_load(sp.p, sp.len, 2u * kUnbinRowBytes + lane * 16u);
    for (uint32_t r = 0; r * kUnbinRowBytes < sp.len; ++r) {
        const uint32_t place = r * kUnbinRowBytes + lane * 16u;
        const u32x4 v = a;
        a = b;
        b = c;
        c = unbin_load(sp.p, sp.len, place + 3u * kUnbinRowBytes);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t m[4];
#pragma unroll
        for (uint32_t d = 0; d < 4u; ++d) m[d] = excess_mask(w[d], k);
        if (!__any((m[0] | m[1] | m[2] | m[3]) != 0u)) continue;  // the one vote of a row without an entry
        uint32_t s = 0;
#pragma unroll
        for (uint32_t d = 0; d < 4u; ++d) s += (uint32_t)__builtin_popcount(m[d]);
        const uint32_t incl = wave_scan_incl_dpp(s);
        if (s) {
            uint64_t o = at + (incl - s);
#pragma unroll
            for (uint32_t d = 0; d < 4u; ++d) {
                if (m[d] == 0u) continue;
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    if (!((m[d] >> (8u * e + 7u)) & 1u)) continue;
                    if (o < capacity) {
                        out_pos[o] = sp.col0 + place + 4u * d + e;
                        out_val[o] = (uint8_t)(((w[d] >> (8u * e)) & 0xFFu) - threshold);
                    } else {
                        ++lost;
                    }
                    ++o;
                }
            }
        }
        at += wave_last(incl);
    }
    lost = wave_sum_u32(lost);
    if (lane == 0 && lost) atomicAdd(over, (unsigned long long)lost);
}

// the dword of a lane's channels [c0, c0 + n) at time step t; n < 4 only in the block's last strip, read bytewise
__device__ __forceinline__ uint32_t excess_cols_load(const uint8_t *__restrict__ in, uint64_t C, uint64_t t, uint32_t c0,
                                                     uint32_t n)
{
    const uint8_t *const p = in + t * C + c0;
    if (n == kExcessLaneCh) return *reinterpret_cast<const u32_u *>(p);
    uint32_t w = 0;
    for (uint32_t j = 0; j < n; ++j) w |= (uint32_t)p[j] << (8u * j);
    return w;
}

constexpr uint32_t kExcessBatch = 8;  // time steps whose loads are issued together

struct ExcessCell {
    uint32_t c0, n;      // the lane's channels [c0, c0 + n), n = 0 .. 4
    uint32_t tt;         // the time tile
    uint64_t t0, t1;     // its steps
};

// wave w < strips * ntt -> its strip and time tile (time tiles of a strip are adjacent waves); uniform but c0 / n
__device__ __forceinline__ ExcessCell excess_cell(uint64_t w, uint32_t ntt, uint64_t T, uint64_t C, uint32_t lane)
{
    ExcessCell q;
    const uint32_t strip = (uint32_t)(w / ntt);
    q.tt = (uint32_t)(w - (uint64_t)strip * ntt);
    const uint64_t c0 = (uint64_t)strip * kExcessStrip + lane * kExcessLaneCh;
    q.c0 = (uint32_t)c0;  // only used with n > 0, where c0 < C < 2^32
    q.n = c0 >= C ? 0u : (C - c0 < kExcessLaneCh ? (uint32_t)(C - c0) : kExcessLaneCh);
    q.t0 = (uint64_t)q.tt * kExcessTileT;
    q.t1 = q.t0 + kExcessTileT < T ? q.t0 + kExcessTileT : T;
    return q;
}

__global__ __launch_bounds__(64 * kExcessWaves) void k_excess_cols_count(const uint8_t *__restrict__ in, uint64_t T, uint64_t C,
                                                                         uint32_t ntt, uint64_t waves, uint32_t k,
                                                                         uint32_t *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * kExcessWaves + wave;
    if (w >= waves) return;
    const ExcessCell q = excess_cell(w, ntt, T, C, lane);
    if (q.n == 0) return;
    uint32_t a02 = 0, a13 = 0;  // 16-bit counters of channels (0, 2) and (1, 3): at most kExcessTileT each
    for (uint64_t t = q.t0; t < q.t1; t += kExcessBatch) {
        uint32_t v[kExcessBatch];
#pragma unroll
        for (uint32_t j = 0; j < kExcessBatch; ++j) v[j] = t + j < q.t1 ? excess_cols_load(in, C, t + j, q.c0, q.n) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < kExcessBatch; ++j) {
            const uint32_t m = excess_mask(v[j], k);
            a02 += (m >> 7) & 0x00FF00FFu;
            a13 += (m >> 15) & 0x00FF00FFu;
        }
    }
    const uint32_t cnt[4] = {a02 & 0xFFFFu, a13 & 0xFFFFu, a02 >> 16, a13 >> 16};
#pragma unroll
    for (uint32_t j = 0; j < kExcessLaneCh; ++j)
        if (j < q.n) sums[(uint64_t)(q.c0 + j) * ntt + q.tt] = cnt[j];
}

__global__ __launch_bounds__(64 * kExcessWaves) void k_excess_cols_emit(const uint8_t *__restrict__ in, uint64_t T, uint64_t C,
                                                                        uint32_t ntt, uint64_t waves, uint32_t k,
                                                                        uint32_t threshold, const uint64_t *__restrict__ base,
                                                                        uint32_t *__restrict__ out_pos,
                                                                        uint8_t *__restrict__ out_val, uint64_t capacity,
                                                                        unsigned long long *over)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * kExcessWaves + wave;
    if (w >= waves) return;
    const ExcessCell q = excess_cell(w, ntt, T, C, lane);
    uint32_t lost = 0;
    if (q.n) {
        uint64_t o[kExcessLaneCh];  // the next output position of each of the lane's cells
#pragma unroll
        for (uint32_t j = 0; j < kExcessLaneCh; ++j) o[j] = j < q.n ? base[(uint64_t)(q.c0 + j) * ntt + q.tt] : 0ull;
        for (uint64_t t = q.t0; t < q.t1; t += kExcessBatch) {
            uint32_t v[kExcessBatch];
#pragma unroll
            for (uint32_t j = 0; j < kExcessBatch; ++j) v[j] = t + j < q.t1 ? excess_cols_load(in, C, t + j, q.c0, q.n) : 0u;
#pragma unroll
            for (uint32_t j = 0; j < kExcessBatch; ++j) {
                const uint32_t m = excess_mask(v[j], k);
                if (m == 0u) continue;  // the whole wave skips a step without an entry
#pragma unroll
                for (uint32_t e = 0; e < kExcessLaneCh; ++e) {
                    if (!((m >> (8u * e + 7u)) & 1u)) continue;  // bytes of channels >= C were loaded as 0
                    if (o[e] < capacity) {
                        out_pos[o[e]] = (uint32_t)(t + j);
                        out_val[o[e]] = (uint8_t)(((v[j] >> (8u * e)) & 0xFFu) - threshold);
                    } else {
                        ++lost;
                    }
                    ++o[e];
                }
            }
        }
    }
    // lanes behind C stay for the reduction: all 64 lanes must be active in it
    lost = wave_sum_u32(lost);
    if (lane == 0 && lost) atomicAdd(over, (unsigned long long)lost);
}

// ---- the read side ----------------------------------------------------------------------------------------------------

template <typename OUT>
__device__ __forceinline__ void excess_add(uint8_t *out, uint64_t row, uint64_t b, uint64_t row_stride, uint64_t col_stride,
                                           uint64_t add)
{
    OUT *const p = reinterpret_cast<OUT *>(out + row * row_stride + b * col_stride);
    if (sizeof(OUT) == 1) {
        const uint64_t s = (uint64_t)*p + add;
        *p = (OUT)(s > 255ull ? 255ull : s);
    } else {
        *p = (OUT)((uint32_t)*p + (uint32_t)add);
    }
}

// r == 1: blockIdx.y strides the rows, the threads of a grid row stride the row's entries
template <typename OUT>
__global__ __launch_bounds__(kApplyThreads) void k_excess_apply1(const uint32_t *__restrict__ pos, const uint8_t *__restrict__ val,
                                                                 uint64_t n_entries, const uint64_t *__restrict__ first,
                                                                 const uint64_t *__restrict__ last, uint64_t n_rows,
                                                                 uint64_t start, uint64_t stop, uint64_t lead,
                                                                 uint8_t *__restrict__ out, uint64_t row_stride,
                                                                 uint64_t col_stride)
{
    for (uint64_t i = blockIdx.y; i < n_rows; i += gridDim.y) {
        uint64_t f = first[i], l = last[i];
        if (f > n_entries) f = n_entries;
        if (l > n_entries) l = n_entries;
        for (uint64_t e = f + (uint64_t)blockIdx.x * kApplyThreads + threadIdx.x; e < l; e += (uint64_t)gridDim.x * kApplyThreads) {
            const uint64_t p = pos[e];
            if (p < start || p >= stop) continue;
            excess_add<OUT>(out, i, p - start + lead, row_stride, col_stride, val[e]);
        }
    }
}

// r > 1: a thread per run of kApplyRun elements; runs_per_row = ceil(elements / kApplyRun)
template <typename OUT>
__global__ __launch_bounds__(kApplyThreads) void k_excess_apply(const uint32_t *__restrict__ pos, const uint8_t *__restrict__ val,
                                                                uint64_t n_entries, const uint64_t *__restrict__ first,
                                                                const uint64_t *__restrict__ last, uint64_t n_rows,
                                                                uint64_t start, uint64_t stop, uint64_t r, uint64_t lead,
                                                                uint64_t elements, uint64_t runs_per_row,
                                                                uint8_t *__restrict__ out, uint64_t row_stride,
                                                                uint64_t col_stride)
{
    const uint64_t jobs = n_rows * runs_per_row;
    for (uint64_t job = (uint64_t)blockIdx.x * kApplyThreads + threadIdx.x; job < jobs; job += (uint64_t)gridDim.x * kApplyThreads) {
        const uint64_t i = job / runs_per_row, run = job - i * runs_per_row;
        uint64_t f = first[i], l = last[i];
        if (f > n_entries) f = n_entries;
        if (l > n_entries) l = n_entries;
        if (f >= l) continue;
        const uint64_t b0 = run * kApplyRun, b1 = b0 + kApplyRun < elements ? b0 + kApplyRun : elements;
        // the positions of the run: element b holds start + b*r - lead .. + r, cut to [start, stop)
        // (a lead of r or more leaves the first elements in front of `start`: no entry falls into them)
        const uint64_t plo = b0 * r > lead ? start + b0 * r - lead : start;
        uint64_t phi = start + b1 * r;
        phi = phi > lead ? phi - lead : 0ull;
        if (phi > stop) phi = stop;
        // the first entry of [f, l) at or behind plo
        uint64_t a = f, z = l;
        while (a < z) {
            const uint64_t mid = a + ((z - a) >> 1);
            if (pos[mid] < plo) a = mid + 1; else z = mid;
        }
        uint64_t cur = ~0ull, acc = 0;
        for (uint64_t e = a; e < l; ++e) {
            const uint64_t p = pos[e];
            if (p >= phi) break;
            if (p < plo) continue;  // only in a list that is not sorted
            const uint64_t b = (p - start + lead) / r;  // in [b0, b1): plo <= p < phi
            if (b != cur) {
                if (cur != ~0ull) excess_add<OUT>(out, i, cur, row_stride, col_stride, acc);
                cur = b, acc = 0;
            }
            acc += val[e];
        }
        if (cur != ~0ull) excess_add<OUT>(out, i, cur, row_stride, col_stride, acc);
    }
}

}  // namespace mh
