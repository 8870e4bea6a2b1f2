// mh_smooth.hpp -- the kernels of mhs_box and mhs_box_f32 (include/muahuff_smooth.h).  What a workgroup owns, the tiles,
// the halo and the grids are mh_smooth_layout.hpp's; DESIGN.md section 4 has the reasoning.
//
// k_box<TWO>: one (channel, tile) item per workgroup visit; one byte in and one (TWO: two) bytes out per sample.  Thread t
// loads the aligned 16-byte group at span position 16 t -- whole where its four dwords hold bytes of the row, dword by
// dword at the row's ragged ends --, clips the 16 bytes as packed 16-bit lanes (even and odd bytes of a dword apart, one
// v_pk_min_u16 each) and takes their running sum.  The threads' totals are scanned over the wave by shuffles and over the
// four waves through LDS; every thread then stores its 16 exclusive prefix sums P, modulo 2^16, to LDS.  A box sum is a
// difference of two of them, at most 65280, so the modulus does not matter, and neither does what the bytes outside
// the row held: no difference spans them.  In the second half lane t takes 4 consecutive outputs per trip, so that the
// wave's LDS reads are consecutive and its stores whole dwords: low bytes to lo, high bytes to hi.  A ragged last dword
// of the row is stored byte by byte: nothing behind the row's cols bytes is written.
//
// k_box_f32: one thread per output, at most 256 float64 additions in ascending column order, the bias, one rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mh_smooth_layout.hpp"

namespace mh {

struct BoxParams {
    const uint8_t *x;
    uint64_t x_row_stride, cols;
    uint32_t window, clip;
    uint8_t *lo, *hi;
    uint64_t out_row_stride, tiles, items;
};

typedef unsigned short box_u16x2 __attribute__((ext_vector_type(2)));
typedef uint16_t box_u16x8 __attribute__((ext_vector_type(8)));

// min of the two 16-bit lanes of v with those of q
__device__ inline uint32_t box_min2(uint32_t v, uint32_t q)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(box_u16x2, v), __builtin_bit_cast(box_u16x2, q)));
}

template <bool TWO>
__global__ __launch_bounds__(kBoxThreads) void k_box(BoxParams p)
{
    __shared__ alignas(16) uint16_t P[kBoxSpan + 8];  // the prefix sums P[0 .. kBoxSpan], written eight at a time
    __shared__ uint32_t wave_sum[kBoxThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q2 = p.clip | (p.clip << 16), w = p.window;
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        uint64_t c, tile, i0;
        box_item(item, p.tiles, &c, &tile);
        const uint32_t n = box_tile_outputs(tile, p.cols, &i0);
        const uint64_t row = (uint64_t)(uintptr_t)p.x + c * p.x_row_stride;
        const uint64_t first = row + i0, need_end = first + n + w - 1;  // the bytes [first, need_end) of the row
        const uint32_t shift = (uint32_t)(first & (kBoxGroup - 1));
        const uint64_t ga = first - shift + (uint64_t)kBoxGroup * tid;  // this thread's group
        const uint8_t *const gp = p.x + (int64_t)(ga - (uint64_t)(uintptr_t)p.x);  // from the kernel's pointer: global loads, not flat
        uint32_t d[4] = {0u, 0u, 0u, 0u};
        if (box_dword_ok(ga, row, need_end) && box_dword_ok(ga + 12, row, need_end)) {
            const uint4 v = *reinterpret_cast<const uint4 *>(gp);
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (box_dword_ok(ga + 4 * k, row, need_end)) d[k] = *reinterpret_cast<const uint32_t *>(gp + 4 * k);
        }
        // exclusive running sums of the 16 clipped bytes
        uint32_t s[16], run = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = box_min2(d[k] & 0x00ff00ffu, q2), o = box_min2((d[k] >> 8) & 0x00ff00ffu, q2);
            s[4 * k] = run, run += e & 0xffffu;
            s[4 * k + 1] = run, run += o & 0xffffu;
            s[4 * k + 2] = run, run += e >> 16;
            s[4 * k + 3] = run, run += o >> 16;
        }
        // the threads' totals: inclusive over the wave, then the waves in front through LDS
        uint32_t inc = run;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const uint32_t up = __shfl_up(inc, sft);
            if (lane >= (uint32_t)sft) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t off = inc - run;
        for (uint32_t v = 0; v < wave; ++v) off += wave_sum[v];
        box_u16x8 h0, h1;  // vectors of the element type P is declared with: one 16-byte LDS store each
#pragma unroll
        for (int k = 0; k < 8; ++k) h0[k] = (uint16_t)(s[k] + off), h1[k] = (uint16_t)(s[8 + k] + off);
        *reinterpret_cast<box_u16x8 *>(&P[kBoxGroup * tid]) = h0;
        *reinterpret_cast<box_u16x8 *>(&P[kBoxGroup * tid + 8]) = h1;
        if (tid == kBoxThreads - 1) P[kBoxSpan] = (uint16_t)(off + run);
        __syncthreads();
        // outputs: 4 per lane and trip
        uint8_t *const lo = p.lo + c * p.out_row_stride + i0;
        uint8_t *const hi = TWO ? p.hi + c * p.out_row_stride + i0 : nullptr;
        for (uint32_t o = 4 * tid; o < n; o += 4 * kBoxThreads) {
            uint32_t b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = shift + (o + k < n ? o + k : o);  // behind the tile's last output: output o again, not stored
                b[k] = (uint32_t)(uint16_t)(P[i + w] - P[i]);
            }
            if (o + 4 <= n) {
                *reinterpret_cast<uint32_t *>(lo + o) = (b[0] & 255u) | ((b[1] & 255u) << 8) | ((b[2] & 255u) << 16) | (b[3] << 24);
                if (TWO) *reinterpret_cast<uint32_t *>(hi + o) = (b[0] >> 8) | ((b[1] >> 8) << 8) | ((b[2] >> 8) << 16) | ((b[3] >> 8) << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (o + k < n) {
                        lo[o + k] = (uint8_t)b[k];
                        if (TWO) hi[o + k] = (uint8_t)(b[k] >> 8);
                    }
            }
        }
        __syncthreads();  // the next item overwrites the prefix sums
    }
}

struct BoxfParams {
    const uint8_t *in;  // float rows, in_row_stride bytes apart
    uint64_t in_row_stride;
    uint32_t k;
    uint64_t cols;
    uint32_t window;
    const float *bias;
    uint8_t *out;
    uint64_t out_row_stride, items;
};

__global__ __launch_bounds__(kBoxfThreads) void k_box_f32(BoxfParams p)
{
    for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint64_t tile = item / p.k;
        const uint32_t j = (uint32_t)(item - tile * p.k);
        const uint64_t i = tile * kBoxfTile + threadIdx.x;
        if (i >= p.cols) continue;
        const float *const in = reinterpret_cast<const float *>(p.in + (uint64_t)j * p.in_row_stride);
        const uint64_t m = i < p.window - 1 ? i : p.window - 1;
        double s = (double)in[i - m];
        for (uint64_t u = i - m + 1; u <= i; ++u) s += (double)in[u];
        reinterpret_cast<float *>(p.out + (uint64_t)j * p.out_row_stride)[i] = (float)(s + (double)p.bias[j]);
    }
}

}  // namespace mh
