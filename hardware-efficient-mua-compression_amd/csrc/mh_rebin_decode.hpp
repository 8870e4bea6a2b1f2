// mh_rebin_decode.hpp -- decode straight to a coarser bin period (mh_decode_rebin): out[b] = sum of r decoded samples.
//
// The work list (built by mh_worklist.hpp, which holds the records RebinTask / RebinFix and kNoSlot) is
// mh_decode_range's (one RebinTask per segment that overlaps the range, up to four consecutive tasks
// of one output row per workgroup, tables shared), but the decoded bytes never reach memory: decode_segment is
// instantiated with a SINK (RebinSink) that receives every decoded row -- 1024 consecutive samples, 16 per lane --
// in registers and turns it into bin sums:
//   * samples outside the task's [lo, hi) (cut by t0 / t1 / the window) are zeroed, in cut rows only;
//   * the lane's 16 inclusive byte prefix sums (packed adds: a sample is < 16, so a lane's sum fits a byte) and a DPP
//     scan of the lane totals go to a 1280-byte LDS row buffer of the wave: E(x) = sum of the row's samples before x is
//     then two LDS reads for any x;
//   * every bin boundary inside the row is taken by one lane (64 boundaries per pass): a bin that starts and ends in the
//     row is E(end) - E(start); the bin open at the row's end is carried, wave-uniform, into the next row / chunk.
// So each bin wholly inside a task is written once, by one lane.  A bin that more than one task touches (cut by a
// segment boundary; a head segment or a last chunk can be shorter than r, so possibly by several) is known to the host:
// its partial sums go by atomicAdd into a zeroed u32 side slot and k_rebin_fix writes it out afterwards; bins no task
// touches are zeroed by k_rebin_fill.  Integer adds: the result does not depend on the order.
// Every address written is fixed by the work list, never by stream contents.
#pragma once

#include "mh_range.hpp"

namespace mh {

struct RebinArgs {
    Dec2Args a;  // as RangeArgs
    const RebinTask *task;
    const RangeWg *wg;
    void *out;       // uint8_t (SAT) or uint32_t elements
    uint32_t *side;  // zeroed before the launch
    uint32_t r, rmagic;  // bin factor; floor(2^32 / r) + 1 (r >= 2): n / r == mulhi(n, rmagic) for n < 2^20
};

template <bool SAT>
struct RebinSink {
    typedef typename std::conditional<SAT, uint8_t, uint32_t>::type elem;
    elem *out;       // the task's bin 0
    uint32_t *side;
    uint32_t *rowbuf;  // LDS, kRebinRowDwords
    uint32_t r, rmagic, lo, hi, jfirst, jlast, head, tail;
    // wave-uniform running state
    uint32_t nbx;    // sample index of the next bin boundary not yet passed
    uint32_t nbin;   // the bin that starts there
    uint32_t carry;  // sum of the samples since the last boundary passed
    int lane;

    __device__ __forceinline__ uint32_t div_r(uint32_t n) const { return r == 1 ? n : __umulhi(n, rmagic); }

    __device__ __forceinline__ void begin(const RebinTask &t)
    {
        lo = t.lo, hi = t.hi, jfirst = t.jfirst, jlast = t.jlast, head = t.head, tail = t.tail;
        nbx = t.ph ? r - t.ph : 0u;
        nbin = t.ph ? 1u : 0u;
        carry = 0;
    }

    __device__ __forceinline__ void emit(uint32_t j, uint32_t v) const
    {
        if ((int32_t)j < (int32_t)jfirst || (int32_t)j > (int32_t)jlast) return;  // (j = -1: the bin before sample 0)
        if (j == jfirst && head != kNoSlot) atomicAdd(side + head, v);
        else if (j == jlast && tail != kNoSlot) atomicAdd(side + tail, v);
        else out[j] = (elem)(SAT && v > 255u ? 255u : v);
    }

    // sum of the row's samples before its sample x (x < 1024)
    __device__ __forceinline__ uint32_t before(uint32_t x) const
    {
        const uint32_t e = rowbuf[256 + (x >> 4)];
        const uint32_t b = reinterpret_cast<const uint8_t *>(rowbuf)[(x & 15u) ? x - 1u : 0u];
        return e + ((x & 15u) ? b : 0u);
    }

    // One decoded row: o = the lane's 16 samples (one per byte), x = the index of its first one.  All 64 lanes.
    __device__ __forceinline__ void row(u32x4 o, uint32_t x)
    {
        const uint32_t xr = (uint32_t)__builtin_amdgcn_readfirstlane((int)(x - (uint32_t)lane * MH_PIECE));
        if (xr < lo || xr + 1024u > hi) {  // a cut row: samples outside [lo, hi) count as 0
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int a = (int)lo - (int)(x + 4 * d), b = (int)hi - (int)(x + 4 * d);  // bytes [a, b) of the dword stay
                const uint32_t ma = a <= 0 ? 0xFFFFFFFFu : a >= 4 ? 0u : 0xFFFFFFFFu << (8 * a);
                const uint32_t mb = b >= 4 ? 0xFFFFFFFFu : b <= 0 ? 0u : ~(0xFFFFFFFFu << (8 * b));
                o[d] &= ma & mb;
            }
        }
        // inclusive prefix sums of the 16 bytes, in place (every sample < 16: no byte overflows)
        uint32_t up = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t p = o[d];
            p += p << 8;
            p += p << 16;
            p += up * 0x01010101u;
            up = p >> 24;
            o[d] = p;
        }
        const uint32_t incl = wave_scan_incl_dpp(up);
        const uint32_t total = wave_last(incl);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the previous row's reads are done
        __builtin_amdgcn_wave_barrier();
        *reinterpret_cast<u32x4 *>(rowbuf + lane * 4) = o;
        rowbuf[256 + lane] = incl - up;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t rel0 = nbx - xr;  // first boundary of the row, if < 1024 (nbx >= xr: rows come in order)
        if (rel0 >= 1024u) {
            carry += total;
            return;
        }
        const uint32_t cnt = div_r(1023u - rel0) + 1u;  // boundaries inside the row
        const uint32_t e0 = before(rel0);
        if (lane == 0) emit(nbin - 1u, carry + e0);  // the bin that ends at the first one
        for (uint32_t j0 = 0; j0 + 1u < cnt; j0 += kLanes) {  // bins that start and end in the row
            const uint32_t j = j0 + (uint32_t)lane;
            if (j + 1u < cnt) {
                const uint32_t s = rel0 + j * r;
                emit(nbin + j, before(s + r) - before(s));
            }
        }
        carry = total - before(rel0 + (cnt - 1u) * r);  // the bin open at the row's end
        nbx += cnt * r;
        nbin += cnt;
    }

    __device__ __forceinline__ void end()
    {
        if (lane == 0) emit(nbin - 1u, carry);
    }
};

// The rungs of k_decode_range (dec_pick, mh_select.hpp); SAT: uint8_t output, min(sum, 255), else uint32_t.
template <int K, int M, int NR, int RL, bool HY, bool SAT>
__global__ __launch_bounds__(256, kDecMinBlocks) void k_decode_rebin(RebinArgs r)
{
    static_assert(K != 1, "the one-symbol decoder has no workgroup form");
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const RangeWg g = r.wg[blockIdx.x];
    const Dec2Args &a = r.a;
    const DecArgs &d = a.d;
    const uint32_t W = a.W;
    constexpr uint32_t kEntDw = K == 4 ? 2 : 1;
    uint32_t *tab = smem;
    uint8_t *tab1 = reinterpret_cast<uint8_t *>(smem + (kEntDw << W));
    const uint32_t mask1 = build_decode_tables<K, 256, 0>(a, g.ch, tab, tab1, (int)threadIdx.x, lane);
    if ((uint32_t)wave >= g.ntask) return;
    uint32_t *stage = smem + dec2_shared_dwords(W, K) + (size_t)wave * (dec2_stage_dwords(NR) + kRebinRowDwords);
    const RebinTask t = r.task[g.task0 + (uint32_t)wave];
    RebinSink<SAT> sink;
    sink.out = reinterpret_cast<typename RebinSink<SAT>::elem *>(r.out) + t.dst;
    sink.side = r.side;
    sink.rowbuf = stage + dec2_stage_dwords(NR);
    sink.r = r.r;
    sink.rmagic = r.rmagic;
    sink.lane = lane;
    sink.begin(t);
    const uint64_t lim = d.payload_words;
    auto room = [&](uint64_t at, uint64_t need) { return at <= lim && lim - at >= need; };
    uint64_t pos = d.seg_off[t.seg];
    for (uint32_t k = 0; k < t.skip; ++k) {  // full chunks in front of the range: header only (k_decode_range's pass())
        bool ok = room(pos, 32);
        if (ok) {
            const ChunkHdr h = scan_header<HY>(d.payload[pos + (uint32_t)(lane & 31)], lane);
            ok = h.nw >= (uint32_t)kChunk / 32 && room(pos, (uint64_t)h.hw + h.nw);
            pos += h.hw + h.nw;
        }
        if (!ok) {
            if (lane == 0) atomicMax(d.err, d.epoch);
            return;
        }
    }
    // `out` of a decoder with a sink is not an address: it is the index of the chunk's first sample (0 here)
    decode_segment<K, M, NR, RL, HY, false, 0, kRangeTag + 1>(d, pos, sink_base(), t.n, tab, 0u, (1u << W) - 1u, tab1, mask1, stage, lane,
                                                               0, &sink);
    sink.end();
}

// Zero fill of elements [off, off + n) (bins no task touches): blockIdx.y = record (RangeFill), x strides over it.
template <class T>
__global__ __launch_bounds__(256) void k_rebin_fill(T *out, const RangeFill *fill)
{
    const RangeFill f = fill[blockIdx.y];
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < f.n; i += (uint64_t)gridDim.x * 256) out[f.off + i] = 0;
}

// The bins several tasks added up in a side slot, written out (after k_decode_rebin).
template <class T>
__global__ __launch_bounds__(256) void k_rebin_fix(T *out, const RebinFix *fix, uint32_t nfix, const uint32_t *side)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nfix) return;
    const uint32_t v = side[fix[i].slot];
    out[fix[i].off] = (T)(sizeof(T) == 1 && v > 255u ? 255u : v);
}

}  // namespace mh
