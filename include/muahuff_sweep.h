/* muahuff_sweep.h -- the C ABI of libmuahuff_sweep.so, the fifth companion of libmuahuff.so: the dynamic-range sweep of
 * the behavioural decoders.  The study clips the counts at S = 2..39 and fits its decoders at every S; these two calls
 * give the Wiener statistics that muahuff_ingest.h (mhi_gram on a clamped copy) and muahuff_wiener.h (mhw_xty) give for
 * ONE clip and ONE range of columns, for every clip of a list, every lag difference and every range in one pass over
 * the counts.  The clamp happens in registers: no clamped copy is written.  The conventions of muahuff.h hold: every
 * call returns MH_OK or an MH_ERR_* code, mhq_last_error() has the text (per thread), there is no CPU fallback.
 *
 * x: uint8 counts, row c at x + c*x_row_stride, cols bytes, at ANY byte address; rows 1..65536, cols 1..2^40-1, lags
 * 1..32.  No byte before column ranges[0] - (lags-1) and none at or after column cols is read.
 * ranges: a HOST array of 2*n_ranges uint64, n_ranges 1..16: range r is the columns [ranges[2r], ranges[2r+1]) of x,
 * ascending and disjoint, the first starting at or after lags-1; an empty range (a == b) is allowed.
 * clips: a HOST array of n_clips uint32, n_clips 1..64, each 1..255 (255 = no clip), strictly ascending.
 * Both arrays are read during the call and copied by value into the kernel parameters. */
#ifndef MUAHUFF_SWEEP_H
#define MUAHUFF_SWEEP_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mhq_version(void);

/* the text of the calling thread's last error */
const char *mhq_last_error(void);

/* ---- count products at every lag difference, for every clip and range ------------------------------------------------------
 * gram[r][n][d][i][j] += sum over u in range r of min(x[i][u], clips[n]) * min(x[j][u-d], clips[n]),   d < lags
 * sums[r][n][i]       += sum over u in range r of min(x[i][u], clips[n])
 * gram: int64 [n_ranges][n_clips][lags][rows][rows], sums: int64 [n_ranges][n_clips][rows], device, contiguous.  Exact,
 * on the int8 matrix cores, ADDED with 64-bit integer atomics: the caller zeroes both first, and two calls give
 * identical bits.  d = 0 computes only the tiles on or above the diagonal and mirrors them.
 * MH_ERR_ARG, before any device work: a NULL pointer among x, ranges, clips, gram, sums; rows, cols, lags, n_ranges or
 * n_clips outside the ranges above; a clip that is 0, above 255 or not above the one in front; a range that is
 * reversed, starts before the one in front ends (the first: before lags-1) or ends past cols; gram or sums not a
 * multiple of 8; x_row_stride below cols with more than one row.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhq_gram_clips(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, const uint64_t *ranges, uint32_t n_ranges,
                   const uint32_t *clips, uint32_t n_clips, uint32_t lags, int64_t *gram, int64_t *sums, void *stream);

/* ---- counts times covariates at every lag, for every clip and range ---------------------------------------------------------
 * out[r][n][l][c][j] = sum over t in range r of min(x[c][t-l], clips[n]) * (double)y[j][t+lead],   l < lags, j < k
 * y: float32 device rows, row j at (char *)y + j*y_row_stride (a multiple of 4), cols floats each; k 1..8; lead below
 * cols, and every range ends at or before cols - lead.  out: float64 [n_ranges][n_clips][lags][rows][k], device,
 * contiguous, overwritten; an empty range gives zeros.
 * The (r, n) slice of out is, bit for bit, what mhw_xty (muahuff_wiener.h) gives on that range with that clip -- x + a -
 * (lags-1), y + a + lead, b - a columns: the same runs counted from the range's own start, the same tree inside a
 * workgroup, the run sums added in run order by a second kernel, no float atomics.
 * scratch: device memory, 8-byte aligned, at least what mhq_xty_clips_scratch_bytes gives for the same rows, cols, lags,
 * k, n_ranges and n_clips -- room for any ranges inside cols; its contents before and after mean nothing.
 * MH_ERR_ARG, before any device work: a NULL pointer among x, ranges, clips, y, out, scratch; a count outside the ranges
 * above; clips and ranges as for mhq_gram_clips, with cols - lead in the place of cols; out or scratch not a multiple
 * of 8, y or y_row_stride not a multiple of 4; x_row_stride below cols with more than one row, y_row_stride below 4*cols
 * with k > 1; scratch_bytes too small.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhq_xty_clips_scratch_bytes(uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint32_t n_ranges, uint32_t n_clips,
                                uint64_t *bytes);
int mhq_xty_clips(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, const uint64_t *ranges, uint32_t n_ranges,
                  const uint32_t *clips, uint32_t n_clips, uint32_t lags, uint32_t lead, const float *y, uint64_t y_row_stride,
                  uint32_t k, double *out, void *scratch, uint64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_SWEEP_H */
