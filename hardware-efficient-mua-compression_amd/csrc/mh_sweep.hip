// mh_sweep.hip -- the C ABI of include/muahuff_sweep.h over the kernels of mh_sweep.hpp.  Every entry point builds its
// argument struct, asks mh_sweep_layout.hpp for a verdict and the layout, and launches what came back: no argument rule
// and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_sweep.hpp"
#include "mh_sweep_layout.hpp"
// built with -fvisibility=hidden: the mhq_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_sweep.h"
#pragma GCC visibility pop

namespace {

template <int K>
void xty_clips_launch(const mh::XtyClipsParams &p, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(mh::k_xty_clips<K>, dim3(grid), dim3(mh::kXtyThreads), 0, st, p);
}

}  // namespace

extern "C" {

int mhq_version(void) { return MH_VERSION; }

const char *mhq_last_error(void) { return g_err; }

int mhq_gram_clips(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, const uint64_t *ranges, uint32_t n_ranges,
                   const uint32_t *clips, uint32_t n_clips, uint32_t lags, int64_t *gram, int64_t *sums, void *stream)
{
    const mh::GramClipsArgs a = {(uintptr_t)x, x_row_stride, rows, cols, ranges, n_ranges, clips, n_clips, lags, (uintptr_t)gram,
                                 (uintptr_t)sums};
    mh::Msg m;
    if (int rc = mh::gram_clips_check(m, a)) return fail(rc, m);
    mh::GramClipsLayout L;  // the ranges and clips by value, the items and the capped grid (mh_sweep_layout.hpp)
    mh::gram_clips_layout(a, &L);
    if (L.grid == 0) return MH_OK;  // every range is empty: nothing is added
    const mh::GramClipsParams p = {x, rows > 1 ? x_row_stride : 0, (uint32_t)rows, lags, n_clips, L.nt, L.tiles0, L.tiles1, L.dt, L.items,
                                   reinterpret_cast<unsigned long long *>(gram), reinterpret_cast<unsigned long long *>(sums), L.ranges,
                                   L.clips};
    hipLaunchKernelGGL(mh::k_gram_clips, dim3(L.grid), dim3(mh::kGramThreads), 0, (hipStream_t)stream, p);
    return launched("mhq_gram_clips");
}

int mhq_xty_clips_scratch_bytes(uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint32_t n_ranges, uint32_t n_clips,
                                uint64_t *bytes)
{
    mh::Msg m;
    if (int rc = mh::xty_clips_scratch_check(m, rows, cols, lags, k, n_ranges, n_clips, (uintptr_t)bytes)) return fail(rc, m);
    *bytes = mh::xty_clips_scratch_bytes(rows, cols, lags, k, n_ranges, n_clips);
    return MH_OK;
}

int mhq_xty_clips(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, const uint64_t *ranges, uint32_t n_ranges,
                  const uint32_t *clips, uint32_t n_clips, uint32_t lags, uint32_t lead, const float *y, uint64_t y_row_stride,
                  uint32_t k, double *out, void *scratch, uint64_t scratch_bytes, void *stream)
{
    const mh::XtyClipsArgs a = {(uintptr_t)x, x_row_stride, rows, cols, ranges, n_ranges, clips, n_clips, lags, lead, (uintptr_t)y,
                                y_row_stride, k, (uintptr_t)out, (uintptr_t)scratch, scratch_bytes};
    mh::Msg m;
    if (int rc = mh::xty_clips_check(m, a)) return fail(rc, m);
    mh::XtyClipsLayout L;  // the ranges and clips by value, the runs, the items and the two capped grids
    mh::xty_clips_layout(a, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::XtyClipsParams p = {x, rows > 1 ? x_row_stride : 0, (uint32_t)rows, lags, lead, n_clips, reinterpret_cast<const uint8_t *>(y),
                                  k > 1 ? y_row_stride : 0, static_cast<double *>(scratch), L.items, L.ranges, L.clips};
    if (L.grid) {
        switch (k) {
        case 1: xty_clips_launch<1>(p, L.grid, st); break;
        case 2: xty_clips_launch<2>(p, L.grid, st); break;
        case 3: xty_clips_launch<3>(p, L.grid, st); break;
        case 4: xty_clips_launch<4>(p, L.grid, st); break;
        case 5: xty_clips_launch<5>(p, L.grid, st); break;
        case 6: xty_clips_launch<6>(p, L.grid, st); break;
        case 7: xty_clips_launch<7>(p, L.grid, st); break;
        default: xty_clips_launch<8>(p, L.grid, st); break;
        }
    }
    hipLaunchKernelGGL(mh::k_xty_clips_sum, dim3(L.sum_grid), dim3(mh::kXtySumThreads), 0, st, static_cast<const double *>(scratch),
                       L.ranges, n_clips, (uint32_t)rows, lags, k, L.elements, out);
    return launched("mhq_xty_clips");
}

}  // extern "C"
