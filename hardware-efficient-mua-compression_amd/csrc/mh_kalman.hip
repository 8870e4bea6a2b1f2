// mh_kalman.hip -- the C ABI of include/muahuff_kalman.h over the kernels of mh_kalman.hpp.  Every entry point builds its
// argument struct, asks mh_kalman_layout.hpp for a verdict and the layout, and launches what came back: no argument rule
// and no grid is worked out here.  A companion of libmuahuff.so, not part of it; there is no CPU fallback here either.
#include <hip/hip_runtime.h>

#include "mh_abi.hpp"
#include "mh_kalman.hpp"
#include "mh_kalman_layout.hpp"
// built with -fvisibility=hidden: the mhk_* functions of the header are ALL the library exports
#pragma GCC visibility push(default)
#include "muahuff_kalman.h"
#pragma GCC visibility pop

namespace {

template <int K>
void launch_project(const mh::ProjectParams &q, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(mh::k_project<K>, dim3(grid), dim3(mh::kProjThreads), 0, st, q);
}

template <int K>
void launch_scan(const mh::ScanParams &q, hipStream_t st)
{
    if (q.L.grid) hipLaunchKernelGGL(mh::k_scan_local<K>, dim3(q.L.grid), dim3(mh::kScanThreads), 0, st, q);
    hipLaunchKernelGGL(mh::k_scan_carry<K>, dim3(q.L.n_ranges), dim3(mh::kScanThreads), 0, st, q);
    if (q.L.grid) hipLaunchKernelGGL(mh::k_scan_apply<K>, dim3(q.L.grid), dim3(mh::kScanThreads), 0, st, q);
}

}  // namespace

extern "C" {

int mhk_version(void) { return MH_VERSION; }

const char *mhk_last_error(void) { return g_err; }

int mhk_project(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t clip, const double *m, const double *m0,
                uint32_t k, double *v, uint64_t v_row_stride, void *stream)
{
    const mh::ProjectArgs a = {(uintptr_t)x, x_row_stride, rows, cols, clip, (uintptr_t)m, (uintptr_t)m0, k, (uintptr_t)v, v_row_stride};
    mh::Msg msg;
    if (int rc = mh::project_check(msg, a)) return fail(rc, msg);
    mh::ProjectLayout L;  // the tiles and the capped grid (mh_kalman_layout.hpp)
    mh::project_layout(cols, &L);
    hipStream_t st = (hipStream_t)stream;
    const mh::ProjectParams q = {x, rows > 1 ? x_row_stride : 0, (uint32_t)rows, cols, clip, m, m0, reinterpret_cast<uint8_t *>(v),
                                 k > 1 ? v_row_stride : 0, L.tiles};
    dispatch_k(k, [&](auto K) { launch_project<K>(q, L.grid, st); });
    return launched("mhk_project");
}

int mhk_scan_scratch_bytes(uint64_t cols, uint32_t k, uint32_t n_ranges, uint64_t *bytes)
{
    mh::Msg msg;
    if (int rc = mh::scan_scratch_check(msg, cols, k, n_ranges, (uintptr_t)bytes)) return fail(rc, msg);
    *bytes = mh::scan_scratch_bytes(cols, k, n_ranges);
    return MH_OK;
}

int mhk_scan(const double *v, uint64_t v_row_stride, uint32_t k, uint64_t cols, const uint64_t *ranges, uint32_t n_ranges, const double *F,
             const double *B, uint32_t n_gain, const double *init, double *out, uint64_t out_row_stride, void *scratch, uint64_t scratch_bytes,
             void *stream)
{
    const mh::ScanArgs a = {(uintptr_t)v, v_row_stride, k, cols, ranges, n_ranges, (uintptr_t)F, (uintptr_t)B, n_gain, (uintptr_t)init,
                            (uintptr_t)out, out_row_stride, (uintptr_t)scratch, scratch_bytes};
    mh::Msg msg;
    if (int rc = mh::scan_check(msg, a)) return fail(rc, msg);
    mh::ScanParams q = {reinterpret_cast<const uint8_t *>(v), k > 1 ? v_row_stride : 0, F, B, n_gain, init, reinterpret_cast<uint8_t *>(out),
                        k > 1 ? out_row_stride : 0, static_cast<double *>(scratch), {}};
    mh::scan_layout(ranges, n_ranges, k, &q.L);  // the ranges by value, their tiles and the capped grid (mh_kalman_layout.hpp)
    hipStream_t st = (hipStream_t)stream;
    dispatch_k(k, [&](auto K) { launch_scan<K>(q, st); });
    return launched("mhk_scan");
}

}  // extern "C"
