"""The LSTM decoder restated in NumPy float64, independent of muahuff.lstm: the reference's input_shaping arithmetic builds the
windows explicitly, the clipped counts are z-scored explicitly, and one Keras LSTM(units) layer (TF2 defaults: gates in
the order i, f, c, o, sigmoid recurrent activation, tanh activation, stateless) followed by Dense(outputs) runs over
them.  Weights are in Keras layout throughout: kernel [C, 4U], recurrent_kernel [U, 4U], bias [4U], dense_kernel [U, K],
dense_bias [K]."""
import numpy as np


def input_shaping(Xin, timestep, stride=1):
    """the reference's preprocess.input_shaping: Xin [samples, features] -> [iterations, timestep, features], row i the
    samples i*stride .. i*stride + timestep - 1, oldest first"""
    num_sample, num_feature = Xin.shape
    num_iter = (num_sample - timestep) // stride + 1
    Xout = np.empty([num_iter, timestep, num_feature])
    Xout[:] = np.nan
    for i in range(num_iter):
        start_idx = i * stride
        Xout[i] = Xin[start_idx:start_idx + timestep]
    return Xout


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def zscore(x, clip, mean, std):
    """x uint8 [C, T] -> float64 [T, C]: (min(x, clip) - mean) / std, a channel of std 0 as zeros (it is dropped)"""
    q = np.minimum(x.astype(np.float64), 255.0 if clip is None else float(clip))
    keep = std > 0
    z = np.zeros_like(q)
    z[keep] = (q[keep] - mean[keep, None]) / std[keep, None]
    return z.T


def steps(Z, lags, recurrent_kernel):
    """Z float64 [rows, 4U]: the input half of the pre-activations of every bin (bias included).  -> the last h of every
    window of `lags` rows, float64 [rows - lags + 1, U]"""
    U = recurrent_kernel.shape[0]
    n = Z.shape[0] - lags + 1
    W = input_shaping(Z, lags, 1)                                   # [n, lags, 4U], explicit windows
    h, c = np.zeros((n, U)), np.zeros((n, U))
    for s in range(lags):
        z = W[:, s] + h @ recurrent_kernel
        i, f, o = sigmoid(z[:, :U]), sigmoid(z[:, U:2 * U]), sigmoid(z[:, 3 * U:])
        g = np.tanh(z[:, 2 * U:3 * U])
        c = f * c + i * g
        h = o * np.tanh(c)
    return h


def recurrence(p, lags, recurrent_kernel, dense_kernel, dense_bias):
    """what mhl_windows computes from a given p [cols, 4U] -> float64 [K, cols - lags + 1]"""
    h = steps(np.asarray(p, dtype=np.float64), lags, recurrent_kernel)
    return (h @ dense_kernel + dense_bias).T


def predict(x, lags, clip, kernel, recurrent_kernel, bias, dense_kernel, dense_bias, mean, std):
    """x uint8 [C, T] -> float64 [K, T - lags + 1]: the model on explicit z-scored windows.  The input half is computed
    per window element, as a framework does, not once per bin."""
    u = input_shaping(zscore(x, clip, mean, std), lags, 1)          # [n, lags, C]
    U = recurrent_kernel.shape[0]
    n = u.shape[0]
    h, c = np.zeros((n, U)), np.zeros((n, U))
    for s in range(lags):
        z = u[:, s] @ kernel + h @ recurrent_kernel + bias
        i, f, o = sigmoid(z[:, :U]), sigmoid(z[:, U:2 * U]), sigmoid(z[:, 3 * U:])
        g = np.tanh(z[:, 2 * U:3 * U])
        c = f * c + i * g
        h = o * np.tanh(c)
    return (h @ dense_kernel + dense_bias).T


def counts(C, T, seed, silent=None):
    """uint8 [C, T]: Poisson counts whose rates drift slowly, a few above any clip; channel `silent` is constant"""
    rng = np.random.RandomState(seed)
    rate = 1.5 + np.sin(np.arange(T)[None, :] / 37.0 + rng.rand(C, 1) * 6.0) + rng.rand(C, 1)
    x = rng.poisson(np.maximum(rate, 0.05)).astype(np.uint8)
    if silent is not None:
        x[silent] = 2
    return x


def moments(x, clip):
    q = np.minimum(x.astype(np.float64), 255.0 if clip is None else float(clip))
    return q.mean(1), q.std(1)


def weights(C, U, K, seed, scale=1.0):
    """Keras-sized random weights: (kernel, recurrent_kernel, bias, dense_kernel, dense_bias), float64, exactly
    representable in float32; `scale` multiplies the input side (kernel and bias) alone"""
    rng = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    kernel = f(scale * rng.uniform(-1, 1, (C, 4 * U)) * np.sqrt(6.0 / (C + 4 * U)))
    rec = f(rng.randn(U, 4 * U) / np.sqrt(U))
    bias = f(scale * 0.1 * rng.randn(4 * U))
    bias[U:2 * U] += 1.0
    return kernel, rec, f(bias), f(rng.uniform(-1, 1, (U, K)) * np.sqrt(6.0 / (U + K))), f(0.1 * rng.randn(K))


def target(x, lags, lead, K, seed):
    """float32 [K, T]: a non-linear function of the lagged counts -- tanh of a projection of the last `lags` bins, times
    the mean rate of a few channels -- placed `lead` bins after the window's last bin"""
    rng = np.random.RandomState(seed)
    C, T = x.shape
    q = np.minimum(x.astype(np.float64), 3.0)
    w = rng.randn(K, lags, C) / np.sqrt(lags * C)
    y = np.zeros((K, T))
    for i in range(T - lags + 1 - lead):
        win = q[:, i:i + lags].T - 1.5
        y[:, i + lags - 1 + lead] = np.tanh(2.0 * np.einsum("klc,lc->k", w, win)) * (1.0 + q[:2, i + lags - 1].mean())
    return y.astype(np.float32)
