/* muahuff_kalman.h -- the C ABI of libmuahuff_kalman.so, the sixth companion of libmuahuff.so: the prediction of a Kalman
 * filter decoder on uint8 spike counts.  In information form the filter's data path is a constant projection of the
 * clipped counts onto the k state directions, v_t = m0 + M min(x_t, clip) (mhk_project), and an affine recurrence
 * s_t = F_t s_{t-1} + B_t v_t whose k x k maps do not depend on the data and reach a fixed point after some steps
 * (mhk_scan).  The conventions of muahuff.h hold: every call returns MH_OK or an MH_ERR_* code, mhk_last_error() has the
 * text (per thread), there is no CPU fallback. */
#ifndef MUAHUFF_KALMAN_H
#define MUAHUFF_KALMAN_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mhk_version(void);

/* the text of the calling thread's last error */
const char *mhk_last_error(void);

/* ---- the constant projection ------------------------------------------------------------------------------------------------
 * v[j][t] = m0[j] + sum over c < rows of m[j][c] * min(x[c][t], clip),  j < k, t < cols.
 * x: uint8, row c at x + c*x_row_stride, cols bytes, at ANY byte address; nothing outside a row's cols bytes is read.
 * m: float64 [k][rows], device.  m0: float64 [k], device, NULL = 0.
 * v: float64, row j at (char *)v + j*v_row_stride, cols values; the pointer and the stride are multiples of 8.
 * k 1..8, rows 1..65536, cols 1..2^40-1, clip 1..255 (255 = none).
 * Arithmetic: float64 throughout.  An output is ONE chain owned by one thread: it starts at m0[j] (0.0 without m0) and
 * takes the channels in ASCENDING order c = 0, 1, .., rows-1, each as one fma(m[j][c], (double)min(x[c][t], clip), acc).
 * No atomics, no partial sums: two calls give identical bits, and a column's bits depend on that column alone, not on
 * cols or on what lies next to it.
 * MH_ERR_ARG, before any device work: x, m or v NULL; k, rows, cols, clip outside the ranges above; m, m0, v or
 * v_row_stride not a multiple of 8; with rows > 1 x_row_stride below cols, with k > 1 v_row_stride below 8*cols, either
 * of them 2^48 or more; v overlapping x, m or m0.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhk_project(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t clip, const double *m,
                const double *m0, uint32_t k, double *v, uint64_t v_row_stride, void *stream);

/* ---- the affine recurrence over ranges of columns ---------------------------------------------------------------------------
 * For every range r < n_ranges of columns [a, b) = [ranges[2r], ranges[2r+1]):
 *   out[:, a] = init[r];   out[:, t] = F[i] out[:, t-1] + B[i] v[:, t],  i = min(t - a - 1, n_gain - 1),  t = a+1 .. b-1.
 * An empty range writes nothing, a range of one column writes only init[r]; columns outside every range are not touched.
 * v, out: float64, row j at (char *) + j*row_stride, cols values; pointers and strides are multiples of 8.  out may be v
 * with the same row stride (in place); otherwise the two do not overlap.
 * F, B: float64 [n_gain][k][k], row major, device; n_gain 1..4096: the last pair serves every later step.
 * init: float64 [n_ranges][k], device.  k 1..8, cols 1..2^40-1, n_ranges 1..16.
 * `ranges` is a HOST array of 2*n_ranges uint64, read during the call and copied by value into the kernel parameters:
 * ascending, disjoint, inside [0, cols].
 * Three launches, ordered by the stream; no workgroup waits for another inside a launch.  The steps t = a+1 .. b-1 of a
 * range are cut into tiles of 512 counted from the range's own start.  (1) A thread per tile runs the recurrence from a
 * zero state and multiplies the tile's maps together; both go to `scratch`.  (2) One wave per range: lane l folds the
 * tiles [l*per, (l+1)*per) of the range, per = ceil(tiles / 64), into one affine map, the 64 maps are applied in lane
 * order to init[r], and lane l walks its tiles again to store the state in front of each.  (3) A thread per tile runs
 * the recurrence from that state and writes its columns.  A step is, row by row, B's k terms in ascending order (one
 * product, then fma) followed by F's k terms (fma).  The order is fixed and depends on the range alone: two calls give
 * identical bits, and a range's bits are the same whether it is computed alone or next to other ranges.
 * scratch: device memory, 8-byte aligned, at least what these ranges need -- mhk_scan_scratch_bytes gives what is enough
 * for ANY n_ranges ranges inside cols columns; its contents before and after mean nothing.
 * MH_ERR_ARG, before any device work: a NULL pointer among v, ranges, F, B, init, out, scratch; k, cols, n_ranges, n_gain
 * outside the ranges above; a pointer or a row stride not a multiple of 8; with k > 1 a row stride below 8*cols or 2^48
 * or more; a range that is reversed, starts before the one in front ends, or ends past cols; out overlapping v without
 * being v with the same stride; scratch_bytes too small; scratch overlapping v or out; out overlapping F, B or init.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhk_scan_scratch_bytes(uint64_t cols, uint32_t k, uint32_t n_ranges, uint64_t *bytes);
int mhk_scan(const double *v, uint64_t v_row_stride, uint32_t k, uint64_t cols, const uint64_t *ranges, uint32_t n_ranges,
             const double *F, const double *B, uint32_t n_gain, const double *init, double *out, uint64_t out_row_stride,
             void *scratch, uint64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_KALMAN_H */
