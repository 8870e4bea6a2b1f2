"""NumPy float64 restatements for the Kalman-filter tests (muahuff.kalman, include/muahuff_kalman.h), written for this
project.  (a) reference_fit / reference_predict are the reference study's KalmanDecoder (Behavioral decoding/HPC
code/functions/decoders.py) as it stands: sklearn's Ridge in closed form, np.cov of the residuals, and a prediction loop
with an explicit C x C inverse in every step.  (b) gain_table / information_predict are the information form the device
runs: K_t = B_t M.  serial_scan / tiled_scan are mhk_scan's semantics, bin by bin and in three phases over tiles."""
import numpy as np

from tests import wiener_oracle as wo


def data(C=7, K=2, T=4000, seed=0):
    """-> (x uint8 [C, T], y float32 [K, T]): a stable AR(1) state (a slow rotation, spectral radius 0.97) drives Poisson
    counts through a log-linear tuning; channel min(3, C-1) is silent, a few counts are 255"""
    rng = np.random.RandomState(seed)
    th = 0.15
    rot = np.eye(K)
    if K > 1:
        rot[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    A = 0.97 * rot
    y = np.zeros((K, T))
    s = rng.randn(K)
    for t in range(T):
        s = A @ s + 0.3 * rng.randn(K)
        y[:, t] = s
    y = y + np.arange(1, K + 1)[:, None]                          # a mean to centre
    tune = 0.6 * rng.randn(C, K)
    rate = np.exp(0.2 + tune @ (y - y.mean(1, keepdims=True)))
    x = np.minimum(rng.poisson(np.minimum(rate, 200.0)), 255).astype(np.uint8)
    x[rng.rand(C, T) < 0.002] = 255
    x[min(3, C - 1)] = 0
    return x, y.astype(np.float32)


def prepare(x, y, lead=0, clip=None, t0=0, t1=None, like=None):
    """The study's preprocessing of the columns [t0, t1): -> dict(Z [n, C'] the z-scored clipped counts with constant
    channels removed, Y [n, K] the centred states y[:, t + lead], keep, mean, std, ybar).  like: a training set's dict,
    whose keep, mean, std and ybar are then used (a test fold)."""
    t1 = x.shape[1] - lead if t1 is None else t1
    X, Y = wo.design(x, y, 1, lead, clip, t0, t1)
    X = X.astype(np.float64)
    if like is None:
        mean, std = X.mean(0), X.std(0)
        keep, ybar = np.flatnonzero(std > 0), Y.mean(0)
    else:
        mean, std, keep, ybar = like["mean"], like["std"], like["keep"], like["ybar"]
    return dict(Z=(X[:, keep] - mean[keep]) / std[keep], Y=Y - ybar, keep=keep, mean=mean, std=std, ybar=ybar)


def ridge(X, Y, alpha):
    """sklearn.linear_model.Ridge(alpha).fit(X, Y).coef_ in closed form: both sides centred, the intercept unpenalised
    -> [outputs, features]"""
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    return np.linalg.solve(Xc.T @ Xc + alpha * np.eye(X.shape[1]), Xc.T @ Yc).T


def reference_fit(Z, Y, alpha=0.0, segments=None):
    """KalmanDecoder.fit(X_train=Z, Y_train=Y) -> (A, W, H, Q).  segments: the lengths of the folds that were concatenated
    into Z and Y; the pairs across their junctions are then left out of A and W (the reference itself counts them)"""
    X1, X2 = Y[:-1], Y[1:]
    if segments is not None:
        inside = np.ones(len(Y) - 1, bool)
        inside[np.cumsum(segments)[:-1] - 1] = False
        X1, X2 = X1[inside], X2[inside]
    A = ridge(X1, X2, alpha)
    W = np.atleast_2d(np.cov((X2 - X1 @ A.T).T))
    H = ridge(Y, Z, alpha)
    Q = np.atleast_2d(np.cov((Z - Y @ H.T).T))
    return A, W, H, Q


def reference_predict(model, Z, y0):
    """KalmanDecoder.predict(X_test=Z, y_test) with y_test[0] = y0 -> states [n, K]: the explicit recursion"""
    A, W, H, Q = model
    k = A.shape[0]
    states = np.empty((Z.shape[0], k))
    P = np.zeros((k, k))
    state = np.asarray(y0, np.float64).copy()
    states[0] = state
    for t in range(Z.shape[0] - 1):
        P_m = A @ P @ A.T + W
        state_m = A @ state
        Kg = P_m @ H.T @ np.linalg.inv(H @ P_m @ H.T + Q)
        P = (np.eye(k) - Kg @ H) @ P_m
        state = state_m + Kg @ (Z[t + 1] - H @ state_m)
        states[t + 1] = state
    return states


def gain_table(model, tol=2.0 ** -50, most=4096):
    """-> (F, B, M): B_t = (I + P_t^- G)^-1 P_t^-, F_t = (I - B_t G) A with M = H^T Q^-1 and G = M H, from P_0^- = W until B
    and F both change by at most tol of their largest entry; None after `most` steps"""
    A, W, H, Q = model
    k = A.shape[0]
    M = np.linalg.solve(Q, H).T
    G = M @ H
    P, Fs, Bs = W.copy(), [], []
    for _ in range(most):
        B = np.linalg.solve(np.eye(k) + P @ G, P)
        low = np.eye(k) - B @ G
        F = low @ A
        done = bool(Fs) and np.abs(B - Bs[-1]).max() <= tol * np.abs(B).max() and np.abs(F - Fs[-1]).max() <= tol * np.abs(F).max()
        Fs.append(F), Bs.append(B)
        if done:
            return np.stack(Fs), np.stack(Bs), M
        P = A @ (low @ P) @ A.T + W
    return None


def serial_scan(v, ranges, F, B, init, out=None):
    """mhk_scan's definition, bin by bin.  v [k, cols]; F, B [n_gain, k, k]; init [ranges, k]"""
    out = np.full(v.shape, np.nan) if out is None else out
    n_gain = len(F)
    for r, (a, b) in enumerate(ranges):
        if b <= a:
            continue
        s = np.asarray(init[r], np.float64).copy()
        out[:, a] = s
        for t in range(a + 1, b):
            i = min(t - a - 1, n_gain - 1)
            s = F[i] @ s + B[i] @ v[:, t]
            out[:, t] = s
    return out


def tiled_scan(v, ranges, F, B, init, tile, out=None):
    """the same in three phases over tiles of `tile` steps counted from each range's own start: per tile the recurrence
    from zero and the product of its maps, then the carries tile after tile, then the recurrence from each carry"""
    out = np.full(v.shape, np.nan) if out is None else out
    n_gain, k = len(F), v.shape[0]
    for r, (a, b) in enumerate(ranges):
        if b <= a:
            continue
        out[:, a] = init[r]
        steps = b - a - 1
        tiles = [(i0, min(i0 + tile, steps)) for i0 in range(0, steps, tile)]
        local = []
        for i0, i1 in tiles:
            s, P = np.zeros(k), np.eye(k)
            for i in range(i0, i1):
                g = min(i, n_gain - 1)
                s = F[g] @ s + B[g] @ v[:, a + 1 + i]
                P = F[g] @ P
            local.append((P, s))
        carry, c = [], np.asarray(init[r], np.float64).copy()
        for P, e in local:
            carry.append(c)
            c = P @ c + e
        for (i0, i1), s in zip(tiles, carry):
            for i in range(i0, i1):
                g = min(i, n_gain - 1)
                s = F[g] @ s + B[g] @ v[:, a + 1 + i]
                out[:, a + 1 + i] = s
    return out


def information_predict(model, Z, y0, tol=2.0 ** -50):
    """the prediction as the device runs it: v_t = M z_t, then s_t = F_i s_{t-1} + B_i v_t from the gain table -> [n, K]"""
    F, B, M = gain_table(model, tol)
    v = M @ Z.T
    return serial_scan(v, [(0, Z.shape[0])], F, B, [y0]).T


def stats(x, y, lead=0, clip=None, t0=0, t1=None):
    """what muahuff.kalman.stats computes for the columns [t0, t1), from the explicit data"""
    t1 = x.shape[1] - lead if t1 is None else t1
    r = wo.stats(x, y, 1, lead, clip, t0, t1)
    Y = np.asarray(y, np.float64)[:, t0 + lead:t1 + lead]
    a, b = Y[:, :-1], Y[:, 1:]
    d = b - a
    r.update(n_pairs=max(t1 - t0 - 1, 0), sum_a=a.sum(1), sum_b=b.sum(1), aa=a @ a.T, bb=b @ b.T, ab=a @ b.T, sum_d=d.sum(1), dd=d @ d.T, ad=a @ d.T)
    return r


def contractive(k, n_gain, radius, seed):
    """-> (F, B) [n_gain, k, k]: random maps, every F scaled to the given spectral radius"""
    rng = np.random.RandomState(seed)
    F = rng.randn(n_gain, k, k)
    for g in range(n_gain):
        F[g] *= radius / np.abs(np.linalg.eigvals(F[g])).max()
    return F, rng.randn(n_gain, k, k)
