// mh_smooth.hip -- the C ABI of include/muahuff_smooth.h over the kernels of mh_smooth.hpp.  Every entry point builds its
// argument struct, asks mh_smooth_layout.hpp for a verdict and the layout, and launches what came back: no argument rule
// and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_smooth.hpp"
#include "mh_smooth_layout.hpp"
// built with -fvisibility=hidden: the mhs_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_smooth.h"
#pragma GCC visibility pop

extern "C" {

int mhs_version(void) { return MH_VERSION; }

const char *mhs_last_error(void) { return g_err; }

int mhs_box(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t window, uint32_t clip, uint8_t *lo,
            uint8_t *hi, uint64_t out_row_stride, void *stream)
{
    const mh::BoxArgs a = {(uintptr_t)x, x_row_stride, rows, cols, window, clip, (uintptr_t)lo, (uintptr_t)hi, out_row_stride};
    mh::Msg m;
    if (int rc = mh::box_check(m, a)) return fail(rc, m);
    mh::BoxLayout L;  // the tiles, the items and the capped grid (mh_smooth_layout.hpp)
    mh::box_layout(rows, cols, hi != nullptr, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::BoxParams q = {x, rows > 1 ? x_row_stride : 0, cols, window, clip, lo, hi, rows > 1 ? out_row_stride : 0, L.tiles, L.items};
    if (hi)
        hipLaunchKernelGGL(mh::k_box<true>, dim3(L.grid), dim3(mh::kBoxThreads), 0, st, q);
    else
        hipLaunchKernelGGL(mh::k_box<false>, dim3(L.grid), dim3(mh::kBoxThreads), 0, st, q);
    return launched("mhs_box");
}

int mhs_box_f32(const float *in, uint64_t in_row_stride, uint32_t k, uint64_t cols, uint32_t window, const float *bias, float *out,
                uint64_t out_row_stride, void *stream)
{
    const mh::BoxfArgs a = {(uintptr_t)in, in_row_stride, k, cols, window, (uintptr_t)bias, (uintptr_t)out, out_row_stride};
    mh::Msg m;
    if (int rc = mh::boxf_check(m, a)) return fail(rc, m);
    mh::BoxfLayout L;  // the tiles, the items and the capped grid (mh_smooth_layout.hpp)
    mh::boxf_layout(cols, k, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::BoxfParams q = {reinterpret_cast<const uint8_t *>(in), k > 1 ? in_row_stride : 0, k, cols, window, bias,
                              reinterpret_cast<uint8_t *>(out), k > 1 ? out_row_stride : 0, L.items};
    hipLaunchKernelGGL(mh::k_box_f32, dim3(L.grid), dim3(mh::kBoxfThreads), 0, st, q);
    return launched("mhs_box_f32");
}

}  // extern "C"
