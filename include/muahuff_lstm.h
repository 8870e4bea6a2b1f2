/* muahuff_lstm.h -- the C ABI of libmuahuff_lstm.so, the seventh companion of libmuahuff.so: the prediction of an LSTM
 * decoder on uint8 spike counts -- one LSTM layer of `units` cells over the last `lags` bins of every channel, then a
 * dense layer, Keras / TF2 defaults, stateless.  The input half of the gate pre-activations depends on the bin and not on
 * the window, so it is computed once per bin (mhl_inproj); only the recurrent half is repeated per window (mhl_windows).
 * With g = gate * units + unit and the gates in Keras order i, f, g (the cell candidate), o:
 *     z = p[i + s] + Wh h;  i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_g);  c = f c + i g;  h = o tanh(c)
 * for the steps s = 0 .. lags-1 of window i, from h = c = 0, and out = Wd h + bd.
 * The conventions of muahuff.h hold: every call returns MH_OK or an MH_ERR_* code, mhl_last_error() has the text (per
 * thread), there is no CPU fallback. */
#ifndef MUAHUFF_LSTM_H
#define MUAHUFF_LSTM_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mhl_version(void);

/* the text of the calling thread's last error */
const char *mhl_last_error(void);

/* ---- the input half of the pre-activations, once per bin --------------------------------------------------------------------
 * p[t*4U + g] = bias[g] + sum over c < rows of wx[g*rows + c] * min(x[c][t], clip),  t < cols, g < 4U, U = units.
 * x: uint8, row c at x + c*x_row_stride, cols bytes, at ANY byte address; nothing outside a row's cols bytes is read.
 * wx: float32 [4U][rows], device; bias: float32 [4U], device: the caller has folded the z-scoring of the counts into both.
 * p: float32 [cols][4U], device, contiguous, time-major: cols * 16 U bytes.
 * units 1..128, rows 1..65536, cols 1..2^40-1, clip 1..255 (255 = none).
 * Arithmetic: float32 on the matrix cores (v_mfma_f32_32x32x2_f32), which is a chain of fmaf.  An output is ONE chain: it
 * starts at 0, takes the channels in ASCENDING order c = 0, 1, .., rows-1, each as one fmaf(min(x[c][t], clip), wx[g][c],
 * acc), and adds bias[g] last.  No atomics, no partial sums: two calls give identical bits, and the bits of p[t] depend on
 * column t and the weights alone, not on cols, on where the column falls in a tile, or on what lies next to it.
 * MH_ERR_ARG, before any device work: x, wx, bias or p NULL; units, rows, cols, clip outside the ranges above; wx, bias or
 * p not a multiple of 4; with rows > 1 x_row_stride below cols or 2^48 or more; p overlapping x, wx or bias.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhl_inproj(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t clip, const float *wx,
               const float *bias, uint32_t units, float *p, void *stream);

/* ---- the recurrence over every window and the dense layer -------------------------------------------------------------------
 * For every window i < cols - lags + 1: the recurrence above over the rows i .. i+lags-1 of p, then
 *     out[j][i] = bd[j] + sum over v < U of wd[j*U + v] * h[v],  j < k,  at (char *)out + j*out_row_stride + 4*i.
 * p: float32 [cols][4U], what mhl_inproj wrote.  wh: float32 [4U][U], device: wh[g*U + v] is the weight from the previous
 * h[v] to pre-activation g.  wd: float32 [k][U], bd: float32 [k], device.  out: float32 rows of cols - lags + 1 values.
 * units 1..128, lags 1..32, k 1..8, cols lags..2^40-1.
 * Arithmetic: float32.  A pre-activation is ONE chain: it starts at p's value and takes the previous units in ASCENDING
 * order, each as one fmaf(wh[g][v], h[v], acc) on the matrix cores (step 0 has h = 0 and adds nothing); an output starts
 * at 0, takes the units ascending as fmaf(wd[j][v], h[v], acc) and adds bd[j] last.  A workgroup owns 32 consecutive
 * windows and a window's arithmetic does not depend on its place among them; no atomics: two calls give identical bits.
 * sigmoid(z) = 1 / (1 + exp(-z)) and tanh(z) = sign(z) * -m / (2 + m), m = expm1(-2 |z|): finite and monotone for every
 * float z, 0 / 1 and -1 / 1 where they saturate.
 * MH_ERR_ARG, before any device work: a NULL pointer among p, wh, wd, bd, out; units, lags, k outside the ranges above;
 * cols below lags or 2^40 or more; a pointer or out_row_stride not a multiple of 4; with k > 1 out_row_stride below
 * 4*(cols - lags + 1) or 2^48 or more; out overlapping p, wh, wd or bd.
 * Only enqueues on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a hipGraph. */
int mhl_windows(const float *p, uint64_t cols, uint32_t lags, uint32_t units, const float *wh, const float *wd,
                const float *bd, uint32_t k, float *out, uint64_t out_row_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_LSTM_H */
