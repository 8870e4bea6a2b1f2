/* muahuff_train.h -- the C ABI of libmuahuff_train.so, the eighth companion of libmuahuff.so: the loss of one minibatch of
 * an LSTM decoder's windows and its gradient with respect to the weights, from the uint8 spike counts where they lie.  The
 * model is muahuff_lstm.h's -- one LSTM layer of `units` cells over `lags` bins of every channel, then a dense layer, the
 * gates in Keras order i, f, g (the cell candidate), o, g = gate * units + unit -- on z-scored counts:
 *     u[c][t] = (float(min(x[c][t], clip)) - mean[c]) * inv[c]
 *     z = Wx u[:, t] + bias + Wh h;  i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_g);  c = f c + i g;  h = o tanh(c)
 * from h = c = 0, and out = Wd h + bd.  The weights are NOT folded: the gradients are with respect to wx, bias, wh, wd and
 * bd as given.  The optimizer is the caller's.
 * The conventions of muahuff.h hold: every call returns MH_OK or an MH_ERR_* code, mht_last_error() has the text (per
 * thread), there is no CPU fallback. */
#ifndef MUAHUFF_TRAIN_H
#define MUAHUFF_TRAIN_H

#include <stdint.h>

#include "muahuff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MH_VERSION of the muahuff.h this library was built against */
int mht_version(void);

/* the text of the calling thread's last error */
const char *mht_last_error(void);

/* ---- the loss of a minibatch and its gradient ---------------------------------------------------------------------------------
 * Window b < batch ends in bin t_b = idx[b] clamped into [lags-1, cols-1-lead] (so no value of idx reads outside x or y;
 * passing valid indices is the caller's duty), covers the bins t_b - (lags-1) .. t_b, oldest first, and its target is
 * y[j][t_b + lead], j < k.  With err[j] = out[j][b] - y[j][t_b + lead]:
 *     out[j*batch + b] = bd[j] + sum over v < U of wd[j*U + v] * h[v]            (h after the last step)
 *     loss[b] = sqrt(mean over j of err[j]^2)
 * and dwx, dbias, dwh, dwd, dbd are the gradient of  scale * sum over b of loss[b]  with respect to wx, bias, wh, wd, bd.
 * A window whose loss is exactly 0 contributes a ZERO gradient (the derivative of the root does not exist there; autograd
 * frameworks return NaN).  A window that idx names twice contributes twice.
 * x: uint8, device, row c at x + c*x_row_stride, cols bytes, at any byte address.  mean, inv: float32 [rows], device;
 * inv[c] = 0 drops channel c (its column of dwx is exactly 0).  idx: int64 [batch], device.
 * wx: float32 [4U][rows]; bias: [4U]; wh: [4U][U]; wd: [k][U]; bd: [k] -- device, contiguous, U = units, the layouts of
 * mhl_inproj / mhl_windows and torch.nn.LSTM.  y: float32, device, row j at (char *)y + j*y_row_stride, cols values.
 * out: float32 [k][batch]; loss: [batch]; dwx, dbias, dwh, dwd, dbd: the shapes of wx, bias, wh, wd, bd -- device, contiguous.
 * scratch: device, 4 * (batch * lags * 10 * units + 8 * batch) bytes.  In floats, with R = batch * lags and row
 * r = b * lags + s for step s of window b: the activated gates [R][4U] at 0, dz (the derivative with respect to the
 * pre-activations) [R][4U] at 4UR, c [R][U] at 8UR, h [R][U] at 9UR, dout [batch][8] at 10UR.
 * units 1..128, lags 1..32, k 1..8, rows 1..65536, batch 1..65536, clip 1..255 (255 = none), cols lags+lead..2^40-1.
 * Arithmetic: float32, the products on the matrix cores (v_mfma_f32_32x32x2_f32), which is a chain of fmaf.  Forward, a
 * pre-activation is one chain: 0, the channels ascending, bias, then the previous units ascending; sigmoid and tanh are
 * mhl_windows'.  Backward, dh of a step is the first 2U pre-activations ascending plus the last 2U ascending.  A weight
 * gradient is ONE chain: it starts at 0 and takes the rows r ascending; no atomics and no partial sums across workgroups.
 * Two calls give identical bits, wherever the scratch lies, and at equal scale a window's out, loss and dz rows do not
 * depend on what else is in the minibatch or where the window stands in idx.
 * MH_ERR_ARG, before any device work: a NULL pointer; units, lags, k, rows, batch, clip, cols outside the ranges above;
 * scale not finite; a float pointer or y_row_stride not a multiple of 4, idx not a multiple of 8; with rows > 1
 * x_row_stride below cols or 2^48 or more; with k > 1 y_row_stride below 4*cols or 2^48 or more; the scratch or a result
 * overlapping an input or each other.
 * Four launches, only enqueued on `stream`: no synchronisation, allocation, copy or free, so it can be captured into a
 * hipGraph (a serial chain). */
int mht_loss_grad(const uint8_t *x, uint64_t x_row_stride, uint64_t rows, uint64_t cols, uint32_t clip, const float *mean,
                  const float *inv, const int64_t *idx, uint32_t batch, uint32_t lags, uint32_t units, uint32_t k,
                  uint64_t lead, const float *wx, const float *bias, const float *wh, const float *wd, const float *bd,
                  const float *y, uint64_t y_row_stride, float scale, void *scratch, float *out, float *loss, float *dwx,
                  float *dbias, float *dwh, float *dwd, float *dbd, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUAHUFF_TRAIN_H */
