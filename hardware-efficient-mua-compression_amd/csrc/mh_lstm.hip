// mh_lstm.hip -- the C ABI of include/muahuff_lstm.h over the kernels of mh_lstm.hpp.  Every entry point builds its
// argument struct, asks mh_lstm_layout.hpp for a verdict and the layout, and launches what came back: no argument rule
// and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_lstm.hpp"
#include "mh_lstm_layout.hpp"
// built with -fvisibility=hidden: the mhl_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_lstm.h"
#pragma GCC visibility pop

namespace {

template <int NB, int KS>
void launch_windows(const mh::WinParams &q, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL((mh::k_windows<NB, KS>), dim3(grid), dim3(mh::kWinThreads), 0, st, q);
}

}  // namespace

extern "C" {

int mhl_version(void) { return MH_VERSION; }

const char *mhl_last_error(void) { return g_err; }

int mhl_inproj(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t clip, const float *wx, const float *bias,
               uint32_t units, float *p, void *stream)
{
    const mh::InprojArgs a = {(uintptr_t)x, x_row_stride, rows, cols, clip, (uintptr_t)wx, (uintptr_t)bias, units, (uintptr_t)p};
    mh::Msg msg;
    if (int rc = mh::inproj_check(msg, a)) return fail(rc, msg);
    mh::InprojLayout L;  // the tiles, the g-tiles and the capped grid (mh_lstm_layout.hpp)
    mh::inproj_layout(cols, units, &L);
    const mh::InprojParams q = {x, rows > 1 ? x_row_stride : 0, (uint32_t)rows, cols, (float)clip, wx, bias, units, p, L.gtiles, L.items};
    hipLaunchKernelGGL(mh::k_inproj, dim3(L.grid), dim3(mh::kInThreads), 0, (hipStream_t)stream, q);
    return launched("mhl_inproj");
}

int mhl_windows(const float *p, uint64_t cols, uint32_t lags, uint32_t units, const float *wh, const float *wd, const float *bd, uint32_t k,
                float *out, uint64_t out_row_stride, void *stream)
{
    const mh::WindowsArgs a = {(uintptr_t)p, cols, lags, units, (uintptr_t)wh, (uintptr_t)wd, (uintptr_t)bd, k, (uintptr_t)out, out_row_stride};
    mh::Msg msg;
    if (int rc = mh::windows_check(msg, a)) return fail(rc, msg);
    mh::WinLayout L;  // the tiles, the blocks a wave owns, the k-steps and the capped grid (mh_lstm_layout.hpp)
    mh::windows_layout(cols, lags, units, &L);
    const mh::WinParams q = {p, lags, units, wh, wd, bd, k, reinterpret_cast<uint8_t *>(out), k > 1 ? out_row_stride : 0, L.windows, L.tiles};
    hipStream_t st = (hipStream_t)stream;
    switch (L.ksteps) {  // per_wave is 1 up to 32 k-steps (64 units), 2 above
        case 8: launch_windows<1, 8>(q, L.grid, st); break;
        case 16: launch_windows<1, 16>(q, L.grid, st); break;
        case 24: launch_windows<1, 24>(q, L.grid, st); break;
        case 32: launch_windows<1, 32>(q, L.grid, st); break;
        case 40: launch_windows<2, 40>(q, L.grid, st); break;
        case 48: launch_windows<2, 48>(q, L.grid, st); break;
        case 56: launch_windows<2, 56>(q, L.grid, st); break;
        default: launch_windows<2, 64>(q, L.grid, st); break;
    }
    return launched("mhl_windows");
}

}  // extern "C"
