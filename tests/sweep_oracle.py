"""NumPy restatements of the two entry points of include/muahuff_sweep.h (mhq_gram_clips, mhq_xty_clips): a loop over the
clips and the ranges of tests/wiener_oracle.design, the explicit design matrix.  Written for this project; the loop is
the study's `for S in S_vector: X_in[X_in > S] = S` (Behavioral decoding/HPC code/*_BDP_S_train.py) around the lagged
design of preprocess.input_shaping."""
import numpy as np

from tests import wiener_oracle as wo


def gram_clips(x, ranges, clips, lags):
    """-> (gram int64 [R, n, lags, C, C], sums int64 [R, n, C]): gram[r][n][d][i][j] = sum over u in range r of
    min(x[i][u], q_n) min(x[j][u-d], q_n) -- the design's lag 0 block against its lag d block"""
    C = x.shape[0]
    gram = np.zeros((len(ranges), len(clips), lags, C, C), np.int64)
    sums = np.zeros((len(ranges), len(clips), C), np.int64)
    for r, (a, b) in enumerate(ranges):
        for n, q in enumerate(clips):
            X, _ = wo.design(x, np.zeros((1, x.shape[1]), np.float32), lags, 0, q, a, b)
            sums[r, n] = X[:, :C].sum(0)
            for d in range(lags):
                gram[r, n, d] = X[:, :C].T @ X[:, d * C:(d + 1) * C]
    return gram, sums


def xty_clips(x, y, ranges, clips, lags, lead):
    """-> (out float64 [R, n, lags, C, K], the sums of |products|, the design rows per range [R])"""
    C, K = x.shape[0], y.shape[0]
    out = np.zeros((len(ranges), len(clips), lags, C, K))
    mag = np.zeros_like(out)
    for r, (a, b) in enumerate(ranges):
        for n, q in enumerate(clips):
            X, Y = wo.design(x, y, lags, lead, q, a, b)
            Xd = X.T.astype(np.float64)
            out[r, n], mag[r, n] = (Xd @ Y).reshape(lags, C, K), (Xd @ np.abs(Y)).reshape(lags, C, K)
    return out, mag, np.array([b - a for a, b in ranges])


def gram_clips_fast(x, ranges, clips, lags):
    """gram_clips without the design matrix, for shapes where that is too large or too slow: the clamped rows against
    themselves d columns earlier as float64 products, which are exact while every sum stays below 2^53 (asserted)"""
    C = x.shape[0]
    gram = np.zeros((len(ranges), len(clips), lags, C, C), np.int64)
    sums = np.zeros((len(ranges), len(clips), C), np.int64)
    for n, q in enumerate(clips):
        xq = wo.clipped(x, q).astype(np.float64)
        for r, (a, b) in enumerate(ranges):
            assert 255.0 * 255.0 * (b - a) < 2.0 ** 53
            sums[r, n] = xq[:, a:b].sum(1).astype(np.int64)
            for d in range(lags):
                gram[r, n, d] = (xq[:, a:b] @ xq[:, a - d:b - d].T).astype(np.int64)
    return gram, sums
