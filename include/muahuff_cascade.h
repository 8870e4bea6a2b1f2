/* muahuff_cascade.h -- the C ABI of libmuahuff_cascade.so, the third companion of libmuahuff.so: what the Wiener cascade
 * (a lagged linear filter followed by a polynomial per output) and fold-wise scoring need on top of muahuff_wiener.h
 * from a prediction that is resident on the device -- its power sums against the target over ranges of columns, and
 * the polynomial itself.  The conventions of muahuff.h hold: every call returns MH_OK or an MH_ERR_* code,
 * mhc_last_error() has the text (per thread), there is no CPU fallback.
 *
 * p, y, out: float32 rows, row j at (char *)p + j*p_row_stride (a multiple of 4), at ANY float address, unit stride
 * along the columns.  Both calls read and write the cols floats of every row and nothing else: what lies around a
 * pitched row is never loaded.  k 1..8, cols 1..2^40-1, degree 1..6. */
#ifndef MUAHUFF_CASCADE_H
#define MUAHUFF_CASCADE_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mhc_version(void);

/* the text of the calling thread's last error */
const char *mhc_last_error(void);

/* ---- power sums of a prediction against a target ------------------------------------------------------------------------
 * For every range r < n_ranges of columns [ranges[2r], ranges[2r+1]) and every output j < k, with
 *   u = ((double)p[j][t] - center[j]) * inv_scale[j]          (center, inv_scale: float64, device, NULL = 0 and 1)
 * out[(r*k + j)*(3*degree + 4) + ...], float64, contiguous, (+)= in this order:
 *   T_i = sum of u^i, i = 0..2*degree (T_0 is the number of columns);  Q_i = sum of u^i * y, i = 0..degree;
 *   YY = sum of y^2;  E = sum of (u - y)^2.
 * That is what a polynomial fit of y on u up to `degree` (Hankel normal equations), the root mean squared error and
 * Pearson's r of u against y need.  The caller offsets p and y so that column t of both belongs together.
 * `ranges` is a HOST array of 2*n_ranges uint64, read during the call and copied by value into the kernel parameters:
 * ascending, disjoint, inside [0, cols); an empty range (a == b) is allowed and gives zeros.  accumulate = 0
 * overwrites, 1 adds to what is there -- once per element.
 * Arithmetic: every per-column term is built from float64 operations that are rounded one by one, never contracted:
 * u (one subtraction, one multiplication), u^i = u^(i-1) * u, u^i * (double)y, (double)y * (double)y,
 * (u - y) * (u - y).  The same chain in any IEEE float64 arithmetic gives the same terms bit for bit; only the order
 * in which they are added is the kernel's own.
 * That order is fixed: every range is cut into runs of 16384 columns counted from the range's own start, every (run,
 * output) writes its 3*degree + 4 partial sums to `scratch` -- device memory, 8-byte aligned, at least what
 * mhc_moments_scratch_bytes gives for the same cols, k, degree and n_ranges; its contents before and after mean nothing
 * -- from a fixed tree, and a second kernel adds a range's runs in run order.  No float atomics: two calls give identical
 * bits, and a range's sums are the same bits whether it is computed alone or next to other ranges.
 * MH_ERR_ARG, before any device work: a NULL pointer among p, y, out, scratch, ranges; k, cols, degree outside the
 * ranges above, n_ranges outside 1..16; accumulate above 1; a range that is reversed, starts before the one in front
 * ends, or ends past cols; p, y or a row stride not a multiple of 4, out, scratch, center or inv_scale not a multiple
 * of 8; a row stride below 4*cols with k > 1; scratch_bytes too small.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhc_moments_scratch_bytes(uint64_t cols, uint32_t k, uint32_t degree, uint32_t n_ranges, uint64_t *bytes);
int mhc_moments(const float *p, uint64_t p_row_stride, const float *y, uint64_t y_row_stride, uint32_t k, uint64_t cols,
                const uint64_t *ranges, uint32_t n_ranges, uint32_t degree, const double *center, const double *inv_scale, double *out,
                uint32_t accumulate, void *scratch, uint64_t scratch_bytes, void *stream);

/* ---- the polynomial stage -------------------------------------------------------------------------------------------------
 * out[j][i] = coef[j][0]*u^degree + ... + coef[j][degree],  u = (p[j][i] - center[j]) * inv_scale[j],  i < cols, in float32.
 * coef: k*(degree + 1) float32, device, the highest power first (as numpy.polyval takes it); center, inv_scale: k
 * float32, device, NULL = 0 and 1.  u is one float32 subtraction and one multiplication, the polynomial Horner's rule as
 * `degree` fmaf: one fixed chain per output, owned by one thread, so two calls give identical bits.
 * out == p with the same row stride (in place) is allowed; any other overlap of out with p or coef is refused.
 * MH_ERR_ARG, before any device work: a NULL pointer among p, coef, out; k, cols, degree outside the ranges above; a
 * pointer or a row stride not a multiple of 4; a row stride below 4*cols with k > 1; such an overlap.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhc_polyval(const float *p, uint64_t p_row_stride, uint32_t k, uint64_t cols, const float *coef, uint32_t degree,
                const float *center, const float *inv_scale, float *out, uint64_t out_row_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_CASCADE_H */
