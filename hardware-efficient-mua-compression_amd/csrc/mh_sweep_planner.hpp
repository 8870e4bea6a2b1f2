// mh_sweep_planner.hpp -- the host side of mh_sweep_create: per channel the sorted breakpoints of all nh windows, one
// slot per interval between them, and the histogram tiles of every slot.  Pure C++ (no HIP, no device), like
// mh_planner.hpp: muahuff.hip uploads what it computes (mh_plan_arena.hpp: sweep_arena); tests/planner_check.cpp
// --sweep runs it under -fsanitize=address,undefined and tests/test_host_sweep_planner.py compares it with a NumPy
// restatement of include/muahuff.h's text.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "mh_msg.hpp"
#include "mh_planner.hpp"

namespace mh {

constexpr uint32_t kSweepMaxHist = 16;  // hist_bits values of one sweep

struct SweepHost {
    uint32_t C = 0, nh = 0, ni = 0;  // ni = 2 * nh + 1 intervals per channel
    std::vector<uint64_t> ch_off;
    std::vector<uint64_t> bounds;    // C * (ni + 1), sorted per channel
    std::vector<uint64_t> slot_len;  // C * ni: slot c * ni + j is [bounds[j], bounds[j + 1]) of channel c
    std::vector<uint32_t> tile_ch, tile_n, tile_slot;  // the tiles of every non-empty slot, in slot order
    std::vector<uint64_t> tile_start;
};

inline int sweep_check_args(Msg &m, const uint64_t *ch_len, uint32_t C, const uint32_t *hist_bits, uint32_t nh)
{
    if (C == 0 || nh == 0 || nh > kSweepMaxHist) return m.set(MH_ERR_ARG, "mh_sweep_create: C=%u nh=%u", C, nh);
    for (uint32_t i = 0; i < nh; ++i)
        if (hist_bits[i] > 30) return m.set(MH_ERR_ARG, "hist_bits[%u]=%u outside 0..30", i, hist_bits[i]);
    for (uint32_t c = 0; c < C; ++c)
        if (ch_len[c] == 0)
            return m.set(MH_ERR_EMPTY_CHANNEL, "channel %u has no bins (the reference raises IndexError)", c);
    return MH_OK;
}

// arguments are already checked
inline void sweep_host_build(SweepHost &w, const uint64_t *ch_off, const uint64_t *ch_len, uint32_t C,
                             const uint32_t *hist_bits, uint32_t nh)
{
    w.C = C;
    w.nh = nh;
    w.ni = 2 * nh + 1;
    const uint32_t np = w.ni + 1;
    w.ch_off.assign(ch_off, ch_off + C);
    w.bounds.resize((size_t)C * np);
    w.slot_len.resize((size_t)C * w.ni);
    // (the tile vectors grow as locals: through `w` every push_back reloads the vector's three pointers)
    std::vector<uint32_t> tile_ch, tile_n, tile_slot;
    std::vector<uint64_t> tile_start;
    for (uint32_t c = 0; c < C; ++c) {
        const uint64_t T = ch_len[c];
        uint64_t *b = &w.bounds[(size_t)c * np];
        uint32_t k = 0;
        b[k++] = 0;
        for (uint32_t i = 0; i < nh; ++i) {
            const uint64_t lim = (uint64_t)1 << hist_bits[i];
            const uint64_t cut = T < lim ? T : lim;  // functions_1.py:59-64
            const uint64_t e = cut + T / 2;          // get_BR_with_approx_sort.py:180
            b[k++] = cut;
            b[k++] = e > T ? T : e;
        }
        b[k++] = T;
        for (uint32_t i = 1; i < np; ++i)  // insertion sort: np <= 34, nearly sorted as built
            for (uint32_t j = i; j > 0 && b[j] < b[j - 1]; --j) std::swap(b[j], b[j - 1]);
        for (uint32_t j = 0; j < w.ni; ++j) {
            const uint64_t lo = b[j], hi = b[j + 1], slot = (uint64_t)c * w.ni + j;
            w.slot_len[slot] = hi - lo;
            for (uint64_t first = lo; first < hi; first += kHistTileBytes) {
                tile_ch.push_back(c);
                tile_slot.push_back((uint32_t)slot);
                tile_start.push_back(first);
                tile_n.push_back(tile_samples(hi - first));
            }
        }
    }
    w.tile_ch = std::move(tile_ch), w.tile_n = std::move(tile_n), w.tile_slot = std::move(tile_slot);
    w.tile_start = std::move(tile_start);
}

}  // namespace mh
