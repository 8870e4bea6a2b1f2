// mh_wiener.hip -- the C ABI of include/muahuff_wiener.h over the kernels of mh_wiener.hpp.  Every entry point builds its
// argument struct, asks mh_wiener_layout.hpp for a verdict and the layout, and launches what came back: no argument rule
// and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_wiener.hpp"
#include "mh_wiener_layout.hpp"
// built with -fvisibility=hidden: the mhw_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_wiener.h"
#pragma GCC visibility pop

namespace {

template <int K>
void xty_launch(const mh::XtyParams &p, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(mh::k_xty<K>, dim3(grid), dim3(mh::kXtyThreads), 0, st, p);
}

}  // namespace

extern "C" {

int mhw_version(void) { return MH_VERSION; }

const char *mhw_last_error(void) { return g_err; }

int mhw_xty_scratch_bytes(uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint64_t *bytes)
{
    mh::Msg m;
    if (int rc = mh::xty_scratch_check(m, rows, cols, lags, k, (uintptr_t)bytes)) return fail(rc, m);
    mh::XtyLayout L;
    mh::xty_layout(rows, cols, lags, k, &L);
    *bytes = L.scratch_bytes;
    return MH_OK;
}

int mhw_xty(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t clip, const float *y,
            uint64_t y_row_stride, uint32_t k, double *out, uint32_t accumulate, void *scratch, uint64_t scratch_bytes,
            void *stream)
{
    const mh::XtyArgs a = {(uintptr_t)x, x_row_stride, rows, cols, lags, clip, (uintptr_t)y, y_row_stride, k, (uintptr_t)out,
                           accumulate, (uintptr_t)scratch, scratch_bytes};
    mh::Msg m;
    if (int rc = mh::xty_check(m, a)) return fail(rc, m);
    mh::XtyLayout L;  // the runs, the items and the two capped grids (mh_wiener_layout.hpp)
    mh::xty_layout(rows, cols, lags, k, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::XtyParams p = {x, x_row_stride, (uint32_t)rows, cols, lags, clip, reinterpret_cast<const uint8_t *>(y), y_row_stride,
                             static_cast<double *>(scratch), L.items};
    dispatch_k(k, [&](auto K) { xty_launch<K>(p, L.grid, st); });
    hipLaunchKernelGGL(mh::k_xty_sum, dim3(L.sum_grid), dim3(mh::kXtySumThreads), 0, st, static_cast<const double *>(scratch),
                       L.runs, (uint32_t)rows, lags, k, L.elements, out, accumulate);
    return launched("mhw_xty");
}

int mhw_fir(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t clip, const float *w,
            const float *bias, uint32_t k, float *out, uint64_t out_row_stride, void *stream)
{
    const mh::FirArgs a = {(uintptr_t)x, x_row_stride, rows, cols, lags, clip, (uintptr_t)w, (uintptr_t)bias, k, (uintptr_t)out,
                           out_row_stride};
    mh::Msg m;
    if (int rc = mh::fir_check(m, a)) return fail(rc, m);
    mh::FirLayout L;  // the workgroup tiles, the M-tiles and the capped grid (mh_wiener_layout.hpp)
    mh::fir_layout(cols, lags, k, &L);
    const mh::FirParams p = {x, x_row_stride, (uint32_t)rows, cols, lags, (float)clip, w, bias, k, reinterpret_cast<uint8_t *>(out),
                             out_row_stride, L.tile_outputs, L.per_mtile, L.mtiles, L.items};
    hipLaunchKernelGGL(mh::k_fir, dim3(L.grid), dim3(mh::kFirThreads), 0, (hipStream_t)stream, p);
    return launched("mhw_fir");
}

}  // extern "C"
