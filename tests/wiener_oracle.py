"""NumPy restatements for the Wiener-filter tests (muahuff.wiener, include/muahuff_wiener.h): the explicit design matrix
and everything the device code derives without ever building it.  Written for this project; each function names the
lines of the reference study it restates (Behavioral decoding/HPC code/functions/{preprocess,metrics}.py and the
*_BDP_S_train.py scripts)."""
import numpy as np


def clipped(x, clip):
    return np.minimum(x, 255 if clip is None else clip)


def design(x, y, lags, lead=0, clip=None, t0=None, t1=None):
    """-> (X int64 [n, lags*C], Y float64 [n, K]) for the design rows [t0, t1) (default: all, [lags-1, T-lead)).
    Feature l*C + c of row t is min(x[c][t-l], clip), target k is y[k][t+lead].  preprocess.input_shaping stacks the
    same `timesteps` bins (oldest first; the order of the lag axis does not change the fit) and the train scripts clip at
    S and shift the kinematics by the lag before it."""
    C, T = x.shape
    t0 = lags - 1 if t0 is None else t0
    t1 = T - lead if t1 is None else t1
    xq = clipped(x, clip).astype(np.int64)
    X = np.concatenate([xq[:, t0 - l:t1 - l].T for l in range(lags)], axis=1)
    Y = np.asarray(y, np.float64).reshape(-1, T)[:, t0 + lead:t1 + lead].T
    return X, Y


def stats(x, y, lags, lead=0, clip=None, t0=None, t1=None):
    X, Y = design(x, y, lags, lead, clip, t0, t1)
    return dict(n=X.shape[0], sum_x=X.sum(0), gram=X.T @ X, xty=X.T.astype(np.float64) @ Y, sum_y=Y.sum(0), sum_yy=Y.T @ Y,
                abs_xty=X.T.astype(np.float64) @ np.abs(Y))


def fit_from_stats(n, sum_x, gram, xty, sum_y, alpha, lags, channels):
    """The train scripts' pipeline from the statistics alone: z-score the features with np.nanmean / np.nanstd (ddof 0),
    drop the columns that turn nan (zero variance), ridge-regress with an unpenalised intercept.  -> (weights
    [K, lags, C], bias [K]) for raw clipped counts; dropped features get 0.  Solved by LU (np.linalg.solve)."""
    n = float(n)
    sum_x, gram = np.asarray(sum_x, np.float64), np.asarray(gram, np.float64)
    mean = sum_x / n
    var = np.diag(gram) / n - mean * mean
    keep = np.flatnonzero(np.asarray(n * np.diag(gram) - sum_x * sum_x) > 0)
    m, s = mean[keep], np.sqrt(var[keep])
    ztz = (gram[np.ix_(keep, keep)] - n * np.outer(m, m)) / np.outer(s, s)
    zty = (np.asarray(xty)[keep] - np.outer(m, sum_y)) / s[:, None]
    wz = np.linalg.solve(ztz + alpha * np.eye(len(keep)), zty)
    w = np.zeros((gram.shape[0], zty.shape[1]))
    w[keep] = wz / s[:, None]
    bias = np.asarray(sum_y) / n - w.T @ mean
    return w.T.reshape(-1, lags, channels), bias


def zscored(X):
    """-> (Z, kept columns, mean, std): the design z-scored as the train scripts do, nan columns removed"""
    X = X.astype(np.float64)
    mean, std = X.mean(0), X.std(0)
    keep = np.flatnonzero(std > 0)
    return (X[:, keep] - mean[keep]) / std[keep], keep, mean, std


def unfold(wz, b0, keep, mean, std, F):
    """weights on the z-scored kept columns and their intercept -> (w [F, K], bias [K]) on the raw features"""
    w = np.zeros((F, wz.shape[1]))
    w[keep] = wz / std[keep][:, None]
    return w, b0 - w.T @ mean


def fit_lstsq(X, Y, alpha):
    """Ridge as least squares on the augmented design [[Z, 1], [sqrt(alpha) I, 0]] against [[Y], [0]] -> (w [F, K], bias)"""
    Z, keep, mean, std = zscored(X)
    n, p = Z.shape
    A = np.zeros((n + p, p + 1))
    A[:n, :p], A[:n, p] = Z, 1.0
    A[n:, :p] = np.sqrt(alpha) * np.eye(p)
    B = np.concatenate([Y, np.zeros((p, Y.shape[1]))])
    sol = np.linalg.lstsq(A, B, rcond=None)[0]
    return unfold(sol[:p], sol[p], keep, mean, std, X.shape[1])


def split_index(n, num_fold):
    """preprocess.split_index on n rows: floor(n / num_fold) rows per fold in order; the validation fold of split i is
    fold i, its test fold is np.roll(arange(num_fold), num_fold - 1)[i], the others train.  -> [(train, valid, test)] as
    index arrays"""
    per = int(np.floor(n / num_fold))
    folds = [np.arange(i * per, (i + 1) * per) for i in range(num_fold)]
    valid = np.arange(num_fold)
    test = np.roll(valid, num_fold - 1)
    out = []
    for i in range(num_fold):
        rest = [folds[k] for k in range(num_fold) if k not in (valid[i], test[i])]
        out.append((np.concatenate(rest) if rest else np.arange(0), folds[valid[i]], folds[test[i]]))
    return out


def rmse(ytrue, ypred):
    """metrics.compute_rmse: per output (columns), over the rows"""
    return np.sqrt(np.mean(np.square(ypred - ytrue), axis=0))


def pearson(ytrue, ypred):
    """metrics.compute_pearson: np.corrcoef per output"""
    return np.array([np.corrcoef(ytrue[:, i], ypred[:, i], rowvar=False)[0, 1] for i in range(ytrue.shape[1])])


def xty(x, y, lags, clip=255):
    """mhw_xty on x [rows, cols + lags - 1], y [k, cols] -> (sum [lags, rows, k], sum of |products|), float64"""
    rows, k, cols = x.shape[0], y.shape[0], y.shape[1]
    xq = clipped(x, clip).astype(np.float64)
    yd = y.astype(np.float64)
    out, mag = np.zeros((lags, rows, k)), np.zeros((lags, rows, k))
    for l in range(lags):
        seg = xq[:, lags - 1 - l:lags - 1 - l + cols]
        out[l], mag[l] = seg @ yd.T, seg @ np.abs(yd).T
    return out, mag


def fir(x, w, bias, lags, clip=255):
    """mhw_fir on x [rows, cols + lags - 1], w [k, lags, rows], bias [k] -> (out [k, cols], |bias| + sum |w| x), in the
    dtype of w (int64 for the exact tests, float64 otherwise)"""
    cols = x.shape[1] - lags + 1
    xq = clipped(x, clip).astype(w.dtype)
    out = np.repeat(np.asarray(bias, w.dtype)[:, None], cols, 1)
    mag = np.abs(out)
    for l in range(lags):
        seg = xq[:, lags - 1 - l:lags - 1 - l + cols]
        out = out + w[:, l, :] @ seg
        mag = mag + np.abs(w[:, l, :]) @ seg
    return out, mag
