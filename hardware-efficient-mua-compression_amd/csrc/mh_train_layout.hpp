// mh_train_layout.hpp -- the argument rules, the tiles, the scratch and the launch grids of mht_loss_grad
// (include/muahuff_train.h): the loss of one minibatch of an LSTM decoder's windows and its gradient with respect to the
// five weight tensors.  Pure C++ (no HIP, no device, no global state), as mh_lstm_layout.hpp: mh_train.hip checks with
// loss_grad_check(), launches what loss_grad_layout() returns, the kernels of mh_train.hpp find their work with the same
// functions, and tests/train_check.cpp walks all of it under -fsanitize=address,undefined.
//
// ROW r = b * lags + s is step s of window b; there are R = batch * lags of them.  Window b ends in bin
// t_b = train_bin(idx[b]) = idx[b] clamped into [lags-1, cols-1-lead]; its step s reads bin t_b - (lags-1) + s.
//
// The scratch, in floats (train_scratch() has the offsets, scratch_bytes() the size):
//     act  [R][4U]   the input half of the pre-activations after k_train_inproj; the activated gates i, f, g, o after
//                    k_train_forward (each value is replaced by the lane that read it)
//     dz   [R][4U]   the derivative of the loss with respect to the pre-activations
//     c    [R][U]    the cell state after step s
//     h    [R][U]    the output after step s
//     dout [batch][8] the derivative with respect to out[j][b], j < k
//
// Four launches.  k_train_inproj: items of (128 rows, 32 pre-activations), a wave 32 rows as the MFMA's M.
// k_train_forward: tiles of kWinTile = 32 windows with the blocks, the permutation and the k-steps of mhl_windows
// (windows_layout).  k_train_backward: the same tiles; the product dh = Wh^T dz has the units as M in UB = ceil(U / 32)
// blocks of 32 and the 4U pre-activations as the reduction, cut in two halves of 2U: wave w of 8 owns block w & 3 and half
// w >> 2, kBwdKSteps * UB k-steps of two pre-activations each (the pad multiplies zeros), and the second half is added to
// the first through LDS.  k_train_wgrad: one wave per item; an item is a 32 x 32 tile of dwx (g-tile, channel tile), a
// 32 x 32 tile of dwh (g-tile, unit tile), or 64 of the 4U + k U + k outputs of dbias, dwd and dbd, in that order.
// Every grid is capped; workgroup b starts at item b and strides by the grid.
#pragma once
#include <stdint.h>

#include "mh_lstm_layout.hpp"
#include "mh_rows.hpp"

namespace mh {

constexpr uint32_t kTrainMaxBatch = 65536;
constexpr uint32_t kTrainInThreads = 256;         // 4 waves, 32 rows each
constexpr uint32_t kTrainInRows = 32 * (kTrainInThreads / 64);
constexpr uint32_t kTrainInMaxBlocks = 4096;
constexpr uint32_t kTrainMaxTiles = 1024;         // the cap of the two recurrence grids
constexpr uint32_t kBwdThreads = 512;             // 8 waves: 4 unit blocks x 2 halves of the reduction
constexpr uint32_t kBwdKSteps = 32;               // k-steps of a wave per unit block: 2U pre-activations / 2, padded
constexpr uint32_t kBwdPitch = 33;                // floats of a row of 32 windows in LDS
constexpr uint32_t kGradThreads = 64;             // one wave per item
constexpr uint32_t kGradTile = 32;
constexpr uint32_t kGradMaxBlocks = 1024;
constexpr uint32_t kTrainDoutPitch = 8;           // floats of a window's row of dout (kLstmMaxK)

// the arguments, pointers as plain addresses: nothing here reads through them
struct LossGradArgs {
    uint64_t x, x_row_stride, rows, cols;
    uint32_t clip;
    uint64_t mean, inv, idx;
    uint32_t batch, lags, units, k;
    uint64_t lead;
    uint64_t wx, bias, wh, wd, bd;
    uint64_t y, y_row_stride;
    float scale;
    uint64_t scratch;
    uint64_t out, loss, dwx, dbias, dwh, dwd, dbd;
};

struct TrainScratch {  // offsets in floats
    uint64_t act, dz, c, h, dout, floats;
};

struct TrainLayout {
    uint64_t R;            // batch * lags
    uint32_t gtiles;       // ceil(4 units / 32)
    uint64_t in_items;     // ceil(R / kTrainInRows) * gtiles
    uint32_t in_grid;
    uint32_t tiles;        // ceil(batch / kWinTile)
    uint32_t rec_grid;     // of k_train_forward and k_train_backward
    uint32_t ksteps;       // of k_train_forward: windows_layout's
    uint32_t ublocks;      // UB = ceil(units / 32): k_train_backward is instantiated per UB
    uint32_t ctiles;       // ceil(rows / 32)
    uint64_t wx_items;     // gtiles * ctiles
    uint32_t wh_items;     // gtiles * ublocks
    uint32_t sum_items;    // ceil((4U + kU + k) / 64)
    uint64_t grad_items;
    uint32_t grad_grid;
};

MH_HD inline TrainScratch train_scratch(uint32_t batch, uint32_t lags, uint32_t units)
{
    const uint64_t R = (uint64_t)batch * lags, G = 4ull * units;
    TrainScratch s;
    s.act = 0;
    s.dz = R * G;
    s.c = 2 * R * G;
    s.h = s.c + R * units;
    s.dout = s.h + R * units;
    s.floats = s.dout + (uint64_t)batch * kTrainDoutPitch;
    return s;
}

// 4 * (batch * lags * 10 * units + 8 * batch): below 2^35
MH_HD inline uint64_t scratch_bytes(uint32_t batch, uint32_t lags, uint32_t units) { return 4 * train_scratch(batch, lags, units).floats; }

// the last bin of a window: idx clamped so that neither the window nor its target leaves the recording (cols >= lags + lead)
MH_HD inline uint64_t train_bin(int64_t idx, uint32_t lags, uint64_t cols, uint64_t lead)
{
    const int64_t lo = (int64_t)lags - 1, hi = (int64_t)(cols - 1 - lead);
    return (uint64_t)(idx < lo ? lo : idx > hi ? hi : idx);
}

inline void loss_grad_layout(uint64_t rows, uint32_t batch, uint32_t lags, uint32_t units, uint32_t k, TrainLayout *L)
{
    L->R = (uint64_t)batch * lags;
    L->gtiles = (4 * units + kGradTile - 1) / kGradTile;
    L->in_items = (L->R + kTrainInRows - 1) / kTrainInRows * L->gtiles;
    L->in_grid = (uint32_t)(L->in_items < kTrainInMaxBlocks ? L->in_items : kTrainInMaxBlocks);
    L->tiles = (batch + kWinTile - 1) / kWinTile;
    L->rec_grid = L->tiles < kTrainMaxTiles ? L->tiles : kTrainMaxTiles;
    WinLayout W;
    windows_layout(lags, lags, units, &W);
    L->ksteps = W.ksteps;
    L->ublocks = (units + 31) / 32;
    L->ctiles = (uint32_t)((rows + kGradTile - 1) / kGradTile);
    L->wx_items = (uint64_t)L->gtiles * L->ctiles;
    L->wh_items = L->gtiles * L->ublocks;
    L->sum_items = (4 * units + k * units + k + kGradThreads - 1) / kGradThreads;
    L->grad_items = L->wx_items + L->wh_items + L->sum_items;
    L->grad_grid = (uint32_t)(L->grad_items < kGradMaxBlocks ? L->grad_items : kGradMaxBlocks);
}

// MH_OK, or MH_ERR_ARG with the text in m: every rule of the header's comment, before any device work
inline int loss_grad_check(Msg &m, const LossGradArgs &a)
{
    const char *const fn = "mht_loss_grad";
    if (!a.x || !a.mean || !a.inv || !a.idx || !a.wx || !a.bias || !a.wh || !a.wd || !a.bd || !a.y || !a.scratch || !a.out || !a.loss ||
        !a.dwx || !a.dbias || !a.dwh || !a.dwd || !a.dbd)
        return m.set(MH_ERR_ARG, "%s: NULL pointer", fn);
    if (a.units < 1 || a.units > kLstmMaxUnits) return m.set(MH_ERR_ARG, "%s: units=%u outside 1..%u", fn, a.units, kLstmMaxUnits);
    if (a.lags < 1 || a.lags > kLstmMaxLags) return m.set(MH_ERR_ARG, "%s: lags=%u outside 1..%u", fn, a.lags, kLstmMaxLags);
    if (int rc = k_rule(m, fn, a.k, kLstmMaxK)) return rc;
    if (int rc = rows_rule(m, fn, a.rows, kLstmMaxRows)) return rc;
    if (a.batch < 1 || a.batch > kTrainMaxBatch) return m.set(MH_ERR_ARG, "%s: batch=%u outside 1..%u", fn, a.batch, kTrainMaxBatch);
    if (int rc = clip_rule(m, fn, a.clip)) return rc;
    if (int rc = cols_rule(m, fn, a.cols)) return rc;
    if (a.lead >= a.cols || a.cols - a.lead < a.lags)
        return m.set(MH_ERR_ARG, "%s: cols=%llu leave no window at lags=%u, lead=%llu", fn, (unsigned long long)a.cols, a.lags,
                     (unsigned long long)a.lead);
    if (!(a.scale == a.scale) || a.scale - a.scale != 0.0f) return m.set(MH_ERR_ARG, "%s: scale is not finite", fn);
    if (a.mean % 4 || a.inv % 4 || a.wx % 4 || a.bias % 4 || a.wh % 4 || a.wd % 4 || a.bd % 4 || a.y % 4 || a.y_row_stride % 4 || a.scratch % 4 ||
        a.out % 4 || a.loss % 4 || a.dwx % 4 || a.dbias % 4 || a.dwh % 4 || a.dwd % 4 || a.dbd % 4)
        return m.set(MH_ERR_ARG, "%s: the float pointers and y_row_stride must be multiples of 4", fn);
    if (a.idx % 8) return m.set(MH_ERR_ARG, "%s: idx must be a multiple of 8", fn);
    if (a.rows > 1 && (a.x_row_stride < a.cols || a.x_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "%s: x_row_stride=%llu is below the %llu bytes of a row, or not below 2^48", fn,
                     (unsigned long long)a.x_row_stride, (unsigned long long)a.cols);
    if (a.k > 1 && (a.y_row_stride < 4 * a.cols || a.y_row_stride >= kMaxStride))
        return m.set(MH_ERR_ARG, "%s: y_row_stride=%llu is below the %llu bytes of a row, or not below 2^48", fn,
                     (unsigned long long)a.y_row_stride, (unsigned long long)(4 * a.cols));
    // what is written (the scratch first, then the seven results) lies apart from what is read and from each other
    const uint64_t U = a.units, G = 4 * U;
    const uint64_t wr[8][2] = {{a.scratch, scratch_bytes(a.batch, a.lags, a.units)},
                               {a.out, 4ull * a.k * a.batch},
                               {a.loss, 4ull * a.batch},
                               {a.dwx, 4 * G * a.rows},
                               {a.dbias, 4 * G},
                               {a.dwh, 4 * G * U},
                               {a.dwd, 4 * U * a.k},
                               {a.dbd, 4ull * a.k}};
    const uint64_t rd[10][2] = {{a.x, strided_end(a.x, a.rows, a.x_row_stride, a.cols) - a.x},
                                {a.mean, 4 * a.rows},
                                {a.inv, 4 * a.rows},
                                {a.idx, 8ull * a.batch},
                                {a.wx, 4 * G * a.rows},
                                {a.bias, 4 * G},
                                {a.wh, 4 * G * U},
                                {a.wd, 4 * U * a.k},
                                {a.bd, 4ull * a.k},
                                {a.y, strided_end(a.y, a.k, a.y_row_stride, 4 * a.cols) - a.y}};
    for (int i = 0; i < 8; ++i) {
        for (int j = 0; j < 10; ++j)
            if (ranges_overlap(wr[i][0], wr[i][0] + wr[i][1], rd[j][0], rd[j][0] + rd[j][1]))
                return m.set(MH_ERR_ARG, "%s: the scratch or a result overlaps an input", fn);
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(wr[i][0], wr[i][0] + wr[i][1], wr[j][0], wr[j][0] + wr[j][1]))
                return m.set(MH_ERR_ARG, "%s: the scratch and the results overlap each other", fn);
    }
    return MH_OK;
}

}  // namespace mh
