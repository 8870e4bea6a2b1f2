"""NumPy restatements for the Wiener-cascade tests (muahuff.cascade, include/muahuff_cascade.h): the power sums with the
header's term chain, the polynomial, the cascade with an explicit design matrix and the cross-validation loop.  Written
for this project on top of tests/wiener_oracle.py; each function names the lines of the reference study it restates
(Behavioral decoding/HPC code/functions/decoders.py, WienerCascadeDecoder, and the *_BDP_S_train.py scripts)."""
import numpy as np

from tests import wiener_oracle as wo


def per(degree):
    return 3 * degree + 4


def moment_terms(p, y, degree, center=None, inv_scale=None):
    """The per-column terms of mhc_moments, float64 [K, 3*degree + 4, cols], in the order of the result: u^0..u^2D,
    u^0 y..u^D y, y^2, (u - y)^2.  Every line is one IEEE float64 operation per element, in the order the header states:
    u = (p - center) * inv_scale, u^i = u^(i-1) * u, u^i * y, (u - y) * (u - y)."""
    p64, y64 = np.asarray(p, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    K = p64.shape[0]
    c = np.zeros(K) if center is None else np.asarray(center, np.float64)
    s = np.ones(K) if inv_scale is None else np.asarray(inv_scale, np.float64)
    u = (p64 - c[:, None]) * s[:, None]
    pw = [np.ones_like(u), u]
    for _ in range(2, 2 * degree + 1):
        pw.append(pw[-1] * u)
    d = u - y64
    rows = pw + [y64] + [pw[i] * y64 for i in range(1, degree + 1)] + [y64 * y64, d * d]
    return np.stack(rows, 1)


def moments(p, y, ranges, degree, center=None, inv_scale=None):
    """mhc_moments -> (sums [R, K, 3*degree + 4], sums of the terms' magnitudes), float64; summed by np.sum (pairwise)"""
    t = moment_terms(p, y, degree, center, inv_scale)
    out = np.stack([t[:, :, a:b].sum(2) for a, b in ranges])
    mag = np.stack([np.abs(t[:, :, a:b]).sum(2) for a, b in ranges])
    return out, mag


def split(sums, degree):
    """a result [..., 3D+4] -> (t [..., 2D+1], q [..., D+1], yy, err)"""
    D = degree
    return sums[..., :2 * D + 1], sums[..., 2 * D + 1:3 * D + 2], sums[..., 3 * D + 2], sums[..., 3 * D + 3]


def polyfit_from_moments(t, q, degree):
    """Hankel normal equations by LU (np.linalg.solve) -> [..., degree + 1], highest power first"""
    idx = np.arange(degree + 1)
    h = t[..., idx[:, None] + idx[None, :]]
    return np.linalg.solve(h, q[..., :degree + 1, None])[..., 0][..., ::-1]


def polyval(p, coef, center=None, inv_scale=None):
    """mhc_polyval in float64 -> (values [K, cols], sum |c_i| |u|^i): coef [K, degree + 1], highest power first"""
    p64, coef = np.asarray(p).astype(np.float64), np.asarray(coef).astype(np.float64)
    K = p64.shape[0]
    c = np.zeros(K) if center is None else np.asarray(center).astype(np.float64)
    s = np.ones(K) if inv_scale is None else np.asarray(inv_scale).astype(np.float64)
    u = (p64 - c[:, None]) * s[:, None]
    out, mag = np.zeros_like(u), np.zeros_like(u)
    for i in range(coef.shape[1]):
        out = out * u + coef[:, i:i + 1]
        mag = mag * np.abs(u) + np.abs(coef[:, i:i + 1])
    return out, mag


def cascade_fit(X, Y, alpha, degree, f32=False):
    """WienerCascadeDecoder.fit (decoders.py: `regres.fit`, `y_pred_linear = regres.predict(X_train)`, `p = np.polyfit(
    y_pred_linear, y_train[:, i], self.degree)`) on the train scripts' z-scored design, the ridge as wo.fit_lstsq solves
    it -> (w [F, K], bias [K], [coefficients per output] or None for degree None).  f32: the linear prediction is rounded
    to float32 before the polynomial sees it, as the device's is."""
    w, b = wo.fit_lstsq(X, Y, alpha)
    if degree is None:
        return w, b, None
    lin = linear(X, w, b, f32)
    return w, b, [np.polyfit(lin[:, k], Y[:, k], degree) for k in range(Y.shape[1])]


def linear(X, w, b, f32=False):
    lin = X.astype(np.float64) @ w + b
    return lin.astype(np.float32).astype(np.float64) if f32 else lin


def cascade_predict(X, w, b, coefs, f32=False):
    """WienerCascadeDecoder.predict: `np.polyval(p, y_pred_linear)` per output -> [n, K]"""
    lin = linear(X, w, b, f32)
    if coefs is None:
        return lin
    return np.stack([np.polyval(coefs[k], lin[:, k]) for k in range(lin.shape[1])], 1)


def cross_validate(x, y, lags, lead, clip, alphas, degrees, num_fold, f32=False):
    """The loop of the *_BDP_S_train.py scripts (`for i in range(num_fold)`: split_index, z-score by the training rows,
    fit, predict the validation and test folds, compute_rmse / compute_pearson into rmse_valid[i, :] ...) over the design
    rows of wo.design -> {(alpha, degree): dict of four [num_fold, K] arrays}"""
    X, Y = wo.design(x, y, lags, lead, clip)
    K = Y.shape[1]
    res = {(a, d): {k: np.full((num_fold, K), np.nan) for k in ("rmse_valid", "rmse_test", "cc_valid", "cc_test")}
           for a in alphas for d in degrees}
    for i, (tr, va, te) in enumerate(wo.split_index(len(X), num_fold)):
        for a in alphas:
            for d in degrees:
                w, b, coefs = cascade_fit(X[tr], Y[tr], a, d, f32)
                r = res[(a, d)]
                for name, idx in (("valid", va), ("test", te)):
                    pred = cascade_predict(X[idx], w, b, coefs, f32)
                    r["rmse_" + name][i] = wo.rmse(Y[idx], pred)
                    r["cc_" + name][i] = wo.pearson(Y[idx], pred)
    return res
