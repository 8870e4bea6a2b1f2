"""The loss of a minibatch of the LSTM decoder's windows and its gradient, restated in NumPy float64 and independent of
muahuff.lstm and of any autograd: the forward pass of tests/lstm_oracle.py on explicit z-scored windows with every step
kept, and a hand-written backward pass through time.  Weights come in Keras layout as lstm_oracle.weights makes them
(kernel [C, 4U], recurrent_kernel [U, 4U], bias [4U], dense_kernel [U, K], dense_bias [K]); the gradients go out in
torch.nn.LSTM's layout, which is mht_loss_grad's: wx [4U, C], bias [4U], wh [4U, U], wd [K, U], bd [K]."""
import numpy as np

from tests.lstm_oracle import sigmoid


def zscored(x, clip, mean, inv):
    """x uint8 [C, T] -> float64 [T, C]: (min(x, clip) - mean) * inv, what every channel enters as"""
    q = np.minimum(x.astype(np.float64), 255.0 if clip is None else float(clip))
    return ((q - mean[:, None]) * inv[:, None]).T


def gather(z, idx, lags):
    """z [T, C] -> the explicit windows [B, lags, C]: window b is the rows idx[b] - (lags-1) .. idx[b], oldest first"""
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.min() >= lags - 1 and idx.max() < z.shape[0]
    return np.stack([z[i - (lags - 1):i + 1] for i in idx])


def loss_grad(u, target, kernel, recurrent_kernel, bias, dense_kernel, dense_bias, scale):
    """u float64 [B, L, C]: the windows; target float64 [B, K].
    -> dict(out [K, B], loss [B]: sqrt(mean over K of err^2), dz [B, L, 4U], and wx, bias, wh, wd, bd: the gradient of
    scale * loss.sum()).  A window whose loss is 0 adds nothing to the gradient."""
    B, L, _C = u.shape
    U = recurrent_kernel.shape[0]
    K = dense_kernel.shape[1]
    h, c = np.zeros((B, U)), np.zeros((B, U))
    tape = []
    for s in range(L):
        z = u[:, s] @ kernel + h @ recurrent_kernel + bias
        i, f, o = sigmoid(z[:, :U]), sigmoid(z[:, U:2 * U]), sigmoid(z[:, 3 * U:])
        g = np.tanh(z[:, 2 * U:3 * U])
        c_prev, h_prev = c, h
        c = f * c + i * g
        h = o * np.tanh(c)
        tape.append((i, f, g, o, c, c_prev, h_prev))
    out = h @ dense_kernel + dense_bias                              # [B, K]
    err = out - target
    loss = np.sqrt((err ** 2).mean(1))
    dout = np.zeros_like(err)
    pos = loss > 0
    dout[pos] = scale * err[pos] / (K * loss[pos, None])
    dwd, dbd = dout.T @ h, dout.sum(0)
    dh = dout @ dense_kernel.T
    dc = np.zeros((B, U))
    dzs = np.zeros((B, L, 4 * U))
    dwx, dwh, dbias = np.zeros((4 * U, u.shape[2])), np.zeros((4 * U, U)), np.zeros(4 * U)
    for s in range(L - 1, -1, -1):
        i, f, g, o, c_s, c_prev, h_prev = tape[s]
        tc = np.tanh(c_s)
        dc = dc + dh * o * (1.0 - tc * tc)
        dz = np.concatenate([dc * g * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], axis=1)
        dzs[:, s] = dz
        dwx += dz.T @ u[:, s]
        dwh += dz.T @ h_prev
        dbias += dz.sum(0)
        dh = dz @ recurrent_kernel.T
        dc = dc * f
    return dict(out=out.T.copy(), loss=loss, dz=dzs, wx=dwx, bias=dbias, wh=dwh, wd=dwd, bd=dbd)
