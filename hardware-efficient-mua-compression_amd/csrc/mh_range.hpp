// mh_range.hpp -- random access in time: decode samples [t0, t1) of selected channels (mh_decode_range).
//
// The work list is built on the host from the plan's directory (mh_worklist.hpp, which also holds the records RangeTask /
// RangeWg / RangeFill; muahuff.hip caches and uploads it): one RangeTask per
// segment that overlaps the range, up to four consecutive tasks of one output row per workgroup (RangeWg), so that
// the channel's decode tables are built once per workgroup as in k_decode2.  A task names the chunks of its segment
// that hold in-range samples: leading chunks before t0 are passed over by scanning their headers only, the decode
// stops after the chunk that holds t1 - 1.  Chunks wholly inside the range go through decode_segment straight into the
// output row; the (at most two per row) chunks cut by t0 or t1 are decoded into a 16-KiB scratch slot of the task and
// only their in-range bytes are copied out.  Positions outside the channel's window are zeroed by k_range_fill.
// The decoder templates are instantiated with a TAG of their own (decode_segment): the k_decode2 / k_decode2w instances
// compile exactly as before.
#pragma once

#include "mh_codec2.hpp"
#include "mh_worklist.hpp"

namespace mh {

struct RangeArgs {
    Dec2Args a;  // a.d: payload, payload_words, seg_off, err, epoch; a.W / peak / enc / codes / S / mode / nK: the tables
    const RangeTask *task;
    const RangeWg *wg;
    uint8_t *out;
    uint8_t *scratch;  // 16384 bytes per slot
};

// In-range bytes [lo, hi) of a chunk decoded into scratch `scr` -> dst.  Whole 16-byte pieces in range leave in one
// (unaligned) vector store, as mh_decode stores its pieces; the two pieces cut by lo / hi byte by byte.
__device__ __forceinline__ void range_copy_cut(const uint8_t *scr, uint8_t *dst, uint32_t lo, uint32_t hi, int lane)
{
    // the wave's own scratch stores (by other lanes) become visible to its loads
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    u32x4 v[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) v[r] = *reinterpret_cast<const u32x4 *>(scr + ((uint32_t)r * kLanes + lane) * MH_PIECE);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const uint32_t b = ((uint32_t)r * kLanes + lane) * MH_PIECE;
        if (b + MH_PIECE <= lo || b >= hi) continue;
        if (b >= lo && b + MH_PIECE <= hi) {
            *reinterpret_cast<u32x4_u *>(dst + b) = v[r];
            continue;
        }
#pragma unroll
        for (int i = 0; i < MH_PIECE; ++i)
            if (b + i >= lo && b + i < hi) dst[b + i] = (uint8_t)(v[r][i >> 2] >> (8 * (i & 3)));
    }
    // every scratch load has returned before the slot is decoded into again
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
}

constexpr int kRangeTag = 1;  // decode_segment's TAG: instances of its own (the codec kernels' code stays as it is)

// Workgroup form (shared tables, as k_decode2): the decoder rung dec_pick (mh_select.hpp) picks for a workgroup-task plan.
template <int K, int M, int NR, int RL, bool HY>
__global__ __launch_bounds__(256, kDecMinBlocks) void k_decode_range(RangeArgs r)
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
    uint32_t *stage = smem + dec2_shared_dwords(W, K) + (size_t)wave * dec2_stage_dwords(NR);
    const RangeTask t = r.task[g.task0 + (uint32_t)wave];
    const uint32_t maskW = (1u << W) - 1u;
    const uint64_t lim = d.payload_words;
    auto room = [&](uint64_t at, uint64_t need) { return at <= lim && lim - at >= need; };
    // pos = first header word of a FULL chunk -> first header word of the next one (false: the header points outside)
    auto pass = [&](uint64_t &p) {
        if (!room(p, 32)) return false;
        const ChunkHdr h = scan_header<HY>(d.payload[p + (uint32_t)(lane & 31)], lane);
        if (h.nw < (uint32_t)kChunk / 32 || !room(p, (uint64_t)h.hw + h.nw)) return false;
        p += h.hw + h.nw;
        return true;
    };
#define MH_RANGE_BAIL()                            \
    do {                                           \
        if (lane == 0) atomicMax(d.err, d.epoch);  \
        return;                                    \
    } while (0)
    uint64_t pos = d.seg_off[t.seg];
    for (uint32_t k = 0; k < t.skip; ++k)
        if (!pass(pos)) MH_RANGE_BAIL();
    uint8_t *out = r.out + t.dst;
    uint8_t *scr = r.scratch + (size_t)t.scr * kChunk;
    const uint32_t last0 = (t.ncnk - 1) * (uint32_t)kChunk;  // first sample of the last chunk
    uint32_t c = 0;                                          // next chunk to decode
    if (t.lo > 0 || (t.ncnk == 1 && t.hi < t.n)) {           // chunk c0 is cut: through scratch
        const uint32_t m = t.n < (uint32_t)kChunk ? t.n : (uint32_t)kChunk;
        decode_segment<K, M, NR, RL, HY, false, 0, kRangeTag>(d, pos, scr, m, tab, 0u, maskW, tab1, mask1, stage, lane);
        range_copy_cut(scr, out, t.lo, t.hi < m ? t.hi : m, lane);
        if (t.ncnk == 1) return;
        if (!pass(pos)) MH_RANGE_BAIL();
        c = 1;
    }
    const bool cut_last = t.hi < t.n;
    const uint32_t nmid = t.ncnk - c - (cut_last ? 1u : 0u);  // chunks wholly inside the range
    if (nmid) {
        const uint32_t first = c * (uint32_t)kChunk;
        const uint32_t n = cut_last ? nmid * (uint32_t)kChunk : t.n - first;
        decode_segment<K, M, NR, RL, HY, false, 0, kRangeTag>(d, pos, out + first, n, tab, 0u, maskW, tab1, mask1, stage, lane);
        if (!cut_last) return;
        for (uint32_t k = 0; k < nmid; ++k)
            if (!pass(pos)) MH_RANGE_BAIL();
    }
    // the last chunk, cut by t1
    decode_segment<K, M, NR, RL, HY, false, 0, kRangeTag>(d, pos, scr, t.n - last0, tab, 0u, maskW, tab1, mask1, stage, lane);
    range_copy_cut(scr, out + last0, 0u, t.hi - last0, lane);
#undef MH_RANGE_BAIL
}

// Zero fill: blockIdx.y = fill record; the blocks of x stride over its 16-byte-aligned pieces, the (at most two) pieces
// cut by the record's ends are written byte by byte.
__global__ __launch_bounds__(256) void k_range_fill(uint8_t *out, const RangeFill *fill)
{
    const RangeFill f = fill[blockIdx.y];
    if (f.n == 0) return;
    uint8_t *p = out + f.off;
    const uintptr_t a0 = (uintptr_t)p & ~(uintptr_t)15, a1 = (uintptr_t)p + f.n;
    const uint64_t npieces = (a1 - a0 + 15) >> 4;
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < npieces; i += (uint64_t)gridDim.x * 256) {
        const uintptr_t q = a0 + i * 16;
        if (q >= (uintptr_t)p && q + 16 <= a1) {
            *reinterpret_cast<u32x4 *>(q) = z;
        } else {
            for (int j = 0; j < 16; ++j)
                if (q + j >= (uintptr_t)p && q + j < a1) *reinterpret_cast<uint8_t *>(q + j) = 0;
        }
    }
}

}  // namespace mh
