// mh_train.hip -- the C ABI of include/muahuff_train.h over the kernels of mh_train.hpp.  The entry point builds its
// argument struct, asks mh_train_layout.hpp for a verdict and the layout, and launches what came back: no argument rule
// and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_train.hpp"
#include "mh_train_layout.hpp"
// built with -fvisibility=hidden: the mht_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_train.h"
#pragma GCC visibility pop

namespace {

template <int NB, int KS>
void launch_forward(const mh::TrainParams &q, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL((mh::k_train_forward<NB, KS>), dim3(grid), dim3(mh::kWinThreads), 0, st, q);
}

template <int UB>
void launch_backward(const mh::TrainParams &q, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL((mh::k_train_backward<UB>), dim3(grid), dim3(mh::kBwdThreads), 0, st, q);
}

}  // namespace

extern "C" {

int mht_version(void) { return MH_VERSION; }

const char *mht_last_error(void) { return g_err; }

int mht_loss_grad(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t clip, const float *mean, const float *inv,
                  const int64_t *idx, uint32_t batch, uint32_t lags, uint32_t units, uint32_t k, uint64_t lead, const float *wx,
                  const float *bias, const float *wh, const float *wd, const float *bd, const float *y, uint64_t y_row_stride, float scale,
                  void *scratch, float *out, float *loss, float *dwx, float *dbias, float *dwh, float *dwd, float *dbd, void *stream)
{
    const mh::LossGradArgs a = {(uintptr_t)x, x_row_stride, rows, cols, clip, (uintptr_t)mean, (uintptr_t)inv, (uintptr_t)idx, batch, lags, units, k,
                                lead, (uintptr_t)wx, (uintptr_t)bias, (uintptr_t)wh, (uintptr_t)wd, (uintptr_t)bd, (uintptr_t)y, y_row_stride, scale,
                                (uintptr_t)scratch, (uintptr_t)out, (uintptr_t)loss, (uintptr_t)dwx, (uintptr_t)dbias, (uintptr_t)dwh, (uintptr_t)dwd,
                                (uintptr_t)dbd};
    mh::Msg msg;
    if (int rc = mh::loss_grad_check(msg, a)) return fail(rc, msg);
    mh::TrainLayout L;  // the rows, the tiles, the items and the capped grids (mh_train_layout.hpp)
    mh::loss_grad_layout(rows, batch, lags, units, k, &L);
    const mh::TrainScratch s = mh::train_scratch(batch, lags, units);
    float *const f = static_cast<float *>(scratch);
    const mh::TrainParams q = {x, rows > 1 ? x_row_stride : 0, (uint32_t)rows, cols, (float)clip, mean, inv, idx, batch, lags, units, k, lead,
                               wx, bias, wh, wd, bd, reinterpret_cast<const uint8_t *>(y), k > 1 ? y_row_stride : 0, scale,
                               f + s.act, f + s.dz, f + s.c, f + s.h, f + s.dout, out, loss, dwx, dbias, dwh, dwd, dbd,
                               (uint32_t)L.R, L.gtiles, L.in_items, L.tiles, L.ctiles, L.ublocks, L.wx_items, L.grad_items, L.wh_items};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mh::k_train_inproj, dim3(L.in_grid), dim3(mh::kTrainInThreads), 0, st, q);
    switch (L.ksteps) {  // as mhl_windows: one block per wave up to 32 k-steps (64 units), two above
        case 8: launch_forward<1, 8>(q, L.rec_grid, st); break;
        case 16: launch_forward<1, 16>(q, L.rec_grid, st); break;
        case 24: launch_forward<1, 24>(q, L.rec_grid, st); break;
        case 32: launch_forward<1, 32>(q, L.rec_grid, st); break;
        case 40: launch_forward<2, 40>(q, L.rec_grid, st); break;
        case 48: launch_forward<2, 48>(q, L.rec_grid, st); break;
        case 56: launch_forward<2, 56>(q, L.rec_grid, st); break;
        default: launch_forward<2, 64>(q, L.rec_grid, st); break;
    }
    switch (L.ublocks) {
        case 1: launch_backward<1>(q, L.rec_grid, st); break;
        case 2: launch_backward<2>(q, L.rec_grid, st); break;
        case 3: launch_backward<3>(q, L.rec_grid, st); break;
        default: launch_backward<4>(q, L.rec_grid, st); break;
    }
    hipLaunchKernelGGL(mh::k_train_wgrad, dim3(L.grad_grid), dim3(mh::kGradThreads), 0, st, q);
    return launched("mht_loss_grad");
}

}  // extern "C"
