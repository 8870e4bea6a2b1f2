/* muahuff_wiener.h -- the C ABI of libmuahuff_wiener.so, the second companion of libmuahuff.so: what a lagged linear
 * (Wiener) decoder needs from a matrix of spike counts that is resident on the device -- the products of the counts with
 * float covariates at every lag, and the prediction of a fitted filter.  The exact count-by-count products of the
 * normal equations are mhi_gram's (muahuff_ingest.h).  The conventions of muahuff.h hold: every call returns MH_OK or an
 * MH_ERR_* code, mhw_last_error() has the text (per thread), there is no CPU fallback.
 *
 * x: uint8 counts, row c (a channel) at x + c*x_row_stride, at ANY byte address, unit stride along time.  Both calls
 * read cols + lags - 1 bytes of every row; mhw_fir reads them as aligned dwords, so up to 3 bytes on either side of a
 * row that share a dword with it are loaded (never another dword) and do not reach the result.
 * lags 1..32, k 1..8, rows 1..65536, cols 1..2^40-1, clip 1..255 (counts enter as min(x, clip); 255 = as they are). */
#ifndef MUAHUFF_WIENER_H
#define MUAHUFF_WIENER_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mhw_version(void);

/* the text of the calling thread's last error */
const char *mhw_last_error(void);

/* ---- counts times covariates at every lag ---------------------------------------------------------------------------
 * out[(l*rows + c)*k + j] (+)= sum over t < cols of min(x[c][t + lags-1-l], clip) * (double)y[j][t]     (float64)
 * y: float32 device rows, row j at (char *)y + j*y_row_stride (a multiple of 4), cols floats each.  out: rows*lags*k
 * float64, contiguous.  accumulate = 0 overwrites, 1 adds to what is there -- once per element.
 * Every product is exact in float64 (8 bits times 24 bits) and the sums stay in float64.  The columns are cut into
 * fixed runs; every (run, channel) writes its lags*k partial sums to `scratch` -- device memory, 8-byte aligned, at
 * least what mhw_xty_scratch_bytes gives for the same rows, cols, lags and k; its contents before and after mean
 * nothing -- and a second kernel adds the runs in run order.  No float atomics: two calls give identical bits.
 * MH_ERR_ARG, before any device work: a NULL pointer; lags, k, rows, cols or clip outside the ranges above; accumulate
 * above 1; out or scratch not a multiple of 8, y or y_row_stride not a multiple of 4; x_row_stride below cols + lags - 1
 * with more than one row, y_row_stride below 4*cols with k > 1; scratch_bytes too small.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph. */
int mhw_xty_scratch_bytes(uint64_t rows, uint64_t cols, uint32_t lags, uint32_t k, uint64_t *bytes);
int mhw_xty(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t clip, const float *y,
            uint64_t y_row_stride, uint32_t k, double *out, uint32_t accumulate, void *scratch, uint64_t scratch_bytes,
            void *stream);

/* ---- the prediction of a lagged linear filter -----------------------------------------------------------------------
 * out[j][i] = bias[j] + sum over l < lags, c < rows of w[(j*lags + l)*rows + c] * min(x[c][i + lags-1-l], clip)   i < cols
 * w (k*lags*rows) and bias (k): float32, device.  out[j][i] is the float at (char *)out + j*out_row_stride + 4*i.
 * The products over the channels run on the f32 matrix cores (v_mfma_f32_32x32x2_f32: an f32 FMA chain, one rounding
 * per product), the sum over the lags follows through LDS.  Every output is one fixed chain -- channels ascending within
 * a lag, then the lags ascending, then the bias -- owned by one thread: no atomics, two calls give identical bits.
 * out must not overlap x, w or bias.
 * MH_ERR_ARG, before any device work: a NULL pointer; lags, k, rows, cols or clip outside the ranges above; w, bias,
 * out or out_row_stride not a multiple of 4; x_row_stride below cols + lags - 1 with more than one row, out_row_stride
 * below 4*cols with k > 1.
 * Only enqueues on `stream`: no synchronisation, allocation or free, so it can be captured into a hipGraph. */
int mhw_fir(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t lags, uint32_t clip, const float *w,
            const float *bias, uint32_t k, float *out, uint64_t out_row_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_WIENER_H */
