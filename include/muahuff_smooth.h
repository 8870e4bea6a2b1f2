/* muahuff_smooth.h -- the C ABI of libmuahuff_smooth.so, the fourth companion of libmuahuff.so: the box sums behind the
 * moving-average window of the behavioural decoders (muahuff_wiener.h, muahuff_cascade.h).  mhs_box turns clipped
 * counts into the sums of `window` consecutive bins, written as two byte planes that the uint8 kernels of the other
 * libraries (mhi_gram, mhw_xty) read as they are; mhs_box_f32 is the same trailing sum on a float32 prediction, which
 * is the prediction from smoothed counts since the box and the filter commute.  The conventions of muahuff.h hold:
 * every call returns MH_OK or an MH_ERR_* code, mhs_last_error() has the text (per thread), there is no CPU fallback. */
#ifndef MUAHUFF_SMOOTH_H
#define MUAHUFF_SMOOTH_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mhs_version(void);

/* the text of the calling thread's last error */
const char *mhs_last_error(void);

/* ---- box sums of clipped counts, as byte planes ---------------------------------------------------------------------------
 * lo[c][i] + 256*hi[c][i] = sum over j < window of min(x[c][i + j], clip),  c < rows, i < cols.
 * x: uint8, row c at x + c*x_row_stride, cols + window - 1 bytes, at ANY byte address.  Rows are read as aligned dwords:
 * at most the 3 bytes on either side that share a dword with the row are loaded, never another dword.
 * window 1..256, clip 1..255, rows 1..65536, cols 1..2^40-1.  The sums are at most 65280 and exact.
 * lo, hi: uint8, row c at + c*out_row_stride, cols bytes; the pointers and the stride are multiples of 16.  Only the cols
 * bytes of every row are written.  hi may be NULL if and only if window*clip <= 255 (every sum fits lo).
 * MH_ERR_ARG, before any device work: x or lo NULL; window, clip, rows, cols outside the ranges above; hi NULL with
 * window*clip > 255; lo, hi or out_row_stride not a multiple of 16; with rows > 1 x_row_stride below cols + window - 1,
 * out_row_stride below cols, or either of them 2^48 or more; lo or hi overlapping x (as byte ranges) or each other
 * (row by row: the rows of hi may lie in the gaps of lo's pitch).
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph.
 * Integers only: two calls give identical bytes. */
int mhs_box(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t window, uint32_t clip,
            uint8_t *lo, uint8_t *hi, uint64_t out_row_stride, void *stream);

/* ---- the trailing box sum of a float prediction -----------------------------------------------------------------------------
 * out[j][i] = (float)(bias[j] + sum over m = 0..min(window-1, i) of (double)in[j][i-m]),  j < k, i < cols:
 * float64 additions in ascending column order, then the bias, then one rounding to float32; one fixed chain per output,
 * owned by one thread, no atomics: identical bits on every call.  Zeros stand in front of column 0.
 * in, out: float32 rows, row j at (char *)in + j*in_row_stride, cols floats each; bias: k float32, device.
 * k 1..8, cols 1..2^40-1, window 1..256.
 * MH_ERR_ARG, before any device work: a NULL pointer among in, bias, out; k, cols, window outside the ranges above; a
 * pointer or a row stride not a multiple of 4; with k > 1 a row stride below 4*cols or 2^48 or more; out overlapping in
 * or bias.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhs_box_f32(const float *in, uint64_t in_row_stride, uint32_t k, uint64_t cols, uint32_t window, const float *bias,
                float *out, uint64_t out_row_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_SMOOTH_H */
