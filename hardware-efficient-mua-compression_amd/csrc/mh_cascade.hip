// mh_cascade.hip -- the C ABI of include/muahuff_cascade.h over the kernels of mh_cascade.hpp.  Every entry point builds
// its argument struct, asks mh_cascade_layout.hpp for a verdict and the layout, and launches what came back: no argument
// rule and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_cascade.hpp"
#include "mh_cascade_layout.hpp"
// built with -fvisibility=hidden: the mhc_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_cascade.h"
#pragma GCC visibility pop

namespace {

template <int D>
void moments_launch(const mh::MomParams &p, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(mh::k_moments<D>, dim3(grid), dim3(mh::kMomThreads), 0, st, p);
}

template <int D>
void polyval_launch(const mh::PolyParams &p, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(mh::k_polyval<D>, dim3(grid), dim3(mh::kPolyThreads), 0, st, p);
}

}  // namespace

extern "C" {

int mhc_version(void) { return MH_VERSION; }

const char *mhc_last_error(void) { return g_err; }

int mhc_moments_scratch_bytes(uint64_t cols, uint32_t k, uint32_t degree, uint32_t n_ranges, uint64_t *bytes)
{
    mh::Msg m;
    if (int rc = mh::mom_scratch_check(m, cols, k, degree, n_ranges, (uintptr_t)bytes)) return fail(rc, m);
    *bytes = mh::mom_scratch_bytes(cols, k, degree, n_ranges);
    return MH_OK;
}

int mhc_moments(const float *p, uint64_t p_row_stride, const float *y, uint64_t y_row_stride, uint32_t k, uint64_t cols,
                const uint64_t *ranges, uint32_t n_ranges, uint32_t degree, const double *center, const double *inv_scale, double *out,
                uint32_t accumulate, void *scratch, uint64_t scratch_bytes, void *stream)
{
    const mh::MomArgs a = {(uintptr_t)p, p_row_stride, (uintptr_t)y, y_row_stride, k, cols, ranges, n_ranges, degree, (uintptr_t)center,
                           (uintptr_t)inv_scale, (uintptr_t)out, accumulate, (uintptr_t)scratch, scratch_bytes};
    mh::Msg m;
    if (int rc = mh::mom_check(m, a)) return fail(rc, m);
    mh::MomLayout L;  // the ranges by value, their runs, the items and the two capped grids (mh_cascade_layout.hpp)
    mh::mom_layout(ranges, n_ranges, k, degree, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::MomParams q = {reinterpret_cast<const uint8_t *>(p), reinterpret_cast<const uint8_t *>(y), p_row_stride, y_row_stride, k,
                             center, inv_scale, static_cast<double *>(scratch), L.items, L.ranges};
    if (L.grid) {  // every range empty: nothing to read, the second kernel stores the zeros
        switch (degree) {
        case 1: moments_launch<1>(q, L.grid, st); break;
        case 2: moments_launch<2>(q, L.grid, st); break;
        case 3: moments_launch<3>(q, L.grid, st); break;
        case 4: moments_launch<4>(q, L.grid, st); break;
        case 5: moments_launch<5>(q, L.grid, st); break;
        default: moments_launch<6>(q, L.grid, st); break;
        }
    }
    hipLaunchKernelGGL(mh::k_moments_sum, dim3(L.sum_grid), dim3(mh::kMomSumThreads), 0, st, static_cast<const double *>(scratch),
                       L.ranges, k, L.per, L.elements, out, accumulate);
    return launched("mhc_moments");
}

int mhc_polyval(const float *p, uint64_t p_row_stride, uint32_t k, uint64_t cols, const float *coef, uint32_t degree,
                const float *center, const float *inv_scale, float *out, uint64_t out_row_stride, void *stream)
{
    const mh::PolyArgs a = {(uintptr_t)p, p_row_stride, k, cols, (uintptr_t)coef, degree, (uintptr_t)center, (uintptr_t)inv_scale,
                            (uintptr_t)out, out_row_stride};
    mh::Msg m;
    if (int rc = mh::poly_check(m, a)) return fail(rc, m);
    mh::PolyLayout L;  // the tiles, the items and the capped grid (mh_cascade_layout.hpp)
    mh::poly_layout(cols, k, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::PolyParams q = {reinterpret_cast<const uint8_t *>(p), p_row_stride, k, cols, coef, center, inv_scale,
                              reinterpret_cast<uint8_t *>(out), out_row_stride, L.items};
    switch (degree) {
    case 1: polyval_launch<1>(q, L.grid, st); break;
    case 2: polyval_launch<2>(q, L.grid, st); break;
    case 3: polyval_launch<3>(q, L.grid, st); break;
    case 4: polyval_launch<4>(q, L.grid, st); break;
    case 5: polyval_launch<5>(q, L.grid, st); break;
    default: polyval_launch<6>(q, L.grid, st); break;
    }
    return launched("mhc_polyval");
}

}  // extern "C"
