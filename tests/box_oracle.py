"""NumPy restatements for the moving-average window (muahuff.smooth, wiener.stats(window=), include/muahuff_smooth.h).
Written for this project on top of tests/wiener_oracle.py: the study's train scripts stack the lags, clip at S and then
smooth every column of the design matrix with functions.preprocess.moving_average, a trailing mean over `window` rows
with window - 1 rows of zeros stacked in front.  Here the division by the window is left out (z-scoring removes it), so
everything stays integer."""
import numpy as np

from tests import wiener_oracle as wo


def box(x, window, clip=None):
    """mhs_box on x [rows, cols + window - 1] -> int64 [rows, cols]: the sums of `window` consecutive clipped bytes"""
    xq = wo.clipped(x, clip).astype(np.int64)
    cs = np.concatenate([np.zeros((x.shape[0], 1), np.int64), np.cumsum(xq, axis=1)], axis=1)   # exact: integers
    return cs[:, window:] - cs[:, :x.shape[1] - window + 1]


def planes(x, window, clip=None):
    """-> (lo, hi) uint8: box() as the two byte planes"""
    b = box(x, window, clip)
    return (b & 255).astype(np.uint8), (b >> 8).astype(np.uint8)


def trailing(M, window):
    """the zero-padded trailing sum down the rows of M [n, F]: row r is the sum of the rows max(0, r-window+1) .. r"""
    pad = np.concatenate([np.zeros((window,) + M.shape[1:], M.dtype), M])
    cs = np.cumsum(pad, axis=0)
    return cs[window:] - cs[:-window]


def design(x, y, lags, lead=0, clip=None, window=1, t0=None, t1=None):
    """-> (X int64 [n, lags*C], Y float64 [n, K]) for the design rows [t0, t1): wo.design over ALL rows, smoothed down the
    rows with zeros in front of the first, then the rows asked for"""
    T = x.shape[1]
    X, Y = wo.design(x, y, lags, lead, clip)
    X = trailing(X, window)
    a = 0 if t0 is None else t0 - (lags - 1)
    b = T - lead - (lags - 1) if t1 is None else t1 - (lags - 1)
    return X[a:b], Y[a:b]


def stats(x, y, lags, lead=0, clip=None, window=1, t0=None, t1=None):
    X, Y = design(x, y, lags, lead, clip, window, t0, t1)
    Xd = X.astype(np.float64)
    return dict(n=X.shape[0], sum_x=X.sum(0), gram=X.T @ X, xty=Xd.T @ Y, sum_y=Y.sum(0), sum_yy=Y.T @ Y, abs_xty=Xd.T @ np.abs(Y))


def box_f32(p, window, bias):
    """mhs_box_f32 on p [k, cols] -> (out, mag) in extended precision: bias + the sum of the last `window` columns (fewer in
    front), and |bias| + the sum of their magnitudes.  Integer input gives integers."""
    wide = np.int64 if np.issubdtype(np.asarray(p).dtype, np.integer) else np.longdouble
    p = np.asarray(p).astype(wide)
    k, cols = p.shape
    out = np.repeat(np.asarray(bias).astype(wide)[:, None], cols, 1)
    mag = np.abs(out)
    for m in range(min(window, cols)):
        out[:, m:] += p[:, :cols - m]
        mag[:, m:] += np.abs(p[:, :cols - m])
    return out, mag
