"""Behavioural decoding from spike counts: the Kalman filter -- the state-space decoder of the BMI literature, with the
kinematics y (float32 [K, T]) as the state and the z-scored clipped counts x (uint8 [C, T]) as the observation --
fitted from sufficient statistics and applied on the device without a loop over time bins.

The model is  y[t+1] = A y[t] + w, w ~ N(0, W)  and  z[t] = H y[t] + q, q ~ N(0, Q),  with z the z-scored counts and y
centred.  With a lead of g >= 0 bins (neural data precede the kinematics) column t of the counts belongs to y[:, t + g].

stats() gives, per range of columns, wiener.stats at one lag (the exact int64 Gram matrix of the counts from mhi_gram,
the products with the kinematics from mhw_xty) and the state's own pair moments; KalmanStats of disjoint ranges add.
KalmanFilter.fit() restates the reference's fit from them: ridge regressions for A and H, residual covariances for W and
Q.  The prediction is in information form: with M = H^T Q^-1 (one Cholesky of Q at fit time) and G = M H, the gain of step
t is K_t = B_t M with B_t = (I + P_t^- G)^-1 P_t^-, k x k, so that
    s_t = F_t s_{t-1} + B_t v_t,   F_t = (I - B_t G) A,   v_t = M z_t.
The covariance recursion never sees the data: gains() tabulates B_t, F_t on the host until they stop changing.  predict()
is then ONE mhk_project (v_t for every bin, with the z-scoring folded into the matrix) and ONE mhk_scan (the recurrence as
a scan of affine maps over ranges of columns).  There is no CPU path: host matrices are refused."""
import numpy as np
import torch

from . import wiener
from .windows import _matrix


class KalmanStats:
    """The sufficient statistics of a range of columns: w, the wiener.Stats at one lag (n, sum_x, gram, xty, sum_y,
    sum_yy); and over the n_pairs pairs (t, t+1) with both members inside the range, float64: sum_a [K] (of y[t]), sum_b
    [K] (of y[t+1]), aa, bb, ab [K, K] (of y[t] y[t]^T, y[t+1] y[t+1]^T, y[t] y[t+1]^T); and the same pairs' steps
    d = y[t+1] - y[t]: sum_d [K], dd, ad [K, K] (of d d^T, y[t] d^T).  The steps carry nothing new, but the fit reads the
    process noise from them: W is the covariance of what is left of a STEP, far smaller than the states wherever the
    kinematics are smooth, and taken from aa, bb and ab it would be the difference of sums thousands of times its size."""

    def __init__(self, w, n_pairs, sum_a, sum_b, aa, bb, ab, sum_d, dd, ad):
        self.w, self.n_pairs, self.sum_a, self.sum_b, self.aa, self.bb, self.ab = w, int(n_pairs), sum_a, sum_b, aa, bb, ab
        self.sum_d, self.dd, self.ad = sum_d, dd, ad

    def _sums(self):
        return (self.sum_a, self.sum_b, self.aa, self.bb, self.ab, self.sum_d, self.dd, self.ad)

    def __add__(self, other):
        """Two results over disjoint ranges -> the result over both.  The pair that straddles the junction of two ranges
        that touch is NOT counted: the sum is over the pairs inside either range.  (The reference concatenates its
        training folds and so counts one spurious pair per junction, between bins that were not neighbours.)"""
        if not isinstance(other, KalmanStats):
            return NotImplemented
        return KalmanStats(self.w + other.w, self.n_pairs + other.n_pairs, *[u + v for u, v in zip(self._sums(), other._sums())])

    def __radd__(self, other):  # sum() starts from 0
        return self if other == 0 else NotImplemented

    def to(self, device):
        return KalmanStats(self.w.to(device), self.n_pairs, *[t.to(device) for t in self._sums()])


def _pair_moments(yr):
    """yr: float64 [K, n], the states of a range -> (n_pairs, sum_a, sum_b, aa, bb, ab, sum_d, dd, ad)"""
    K, n = int(yr.shape[0]), int(yr.shape[1])
    if n < 2:
        z1, z2 = torch.zeros((K,), dtype=torch.float64, device=yr.device), torch.zeros((K, K), dtype=torch.float64, device=yr.device)
        return 0, z1, z1.clone(), z2, z2.clone(), z2.clone(), z1.clone(), z2.clone(), z2.clone()
    a, b = yr[:, :-1], yr[:, 1:]
    d = b - a
    return n - 1, a.sum(1), b.sum(1), a @ a.t(), b @ b.t(), a @ b.t(), d.sum(1), d @ d.t(), a @ d.t()


def stats(x, y, lead=0, clip=None, ranges=None):
    """The sufficient statistics of a Kalman filter -> [KalmanStats], one per range [a, b) of columns of the counts
    (default: the single range [0, bins - lead)); column t belongs to the state y[:, t + lead].  x: counts, a 2-D uint8
    device tensor or a ChannelSet; y: float32 device tensor [K, bins]; clip: None or 1..255.  The count statistics are
    wiener.stats(x, y, 1, lead, clip, ranges); the pair moments are float64 torch sums over the range.

    Added ranges drop the pair across their junction (KalmanStats.__add__); the reference, which concatenates its
    training folds, counts one spurious pair per junction."""
    x, _rows, cols = _matrix(x, "kalman.stats")
    ws = wiener.stats(x, y, 1, lead, clip, ranges)
    y, _K = wiener._covariates(y, x, cols)
    g = int(lead)
    out = []
    for (a, b), w in zip(wiener._ranges(ranges, 1, g, cols), ws):
        out.append(KalmanStats(w, *_pair_moments(y[:, a + g:b + g].double())))
    return out


def _chol(a, what):
    """the Cholesky factor of a, refused by the pivot test of WienerFilter.fit"""
    chol, info = torch.linalg.cholesky_ex(a)
    floor = 64 * 2.0 ** -52 * a.shape[0] * float(torch.diagonal(a).max())
    if int(info) != 0 or float((torch.diagonal(chol) ** 2).min()) <= floor:
        raise ValueError("%s is not positive definite (collinear channels or too few bins): use alpha > 0" % what)
    return chol


class KalmanFilter:
    """The reference's KalmanDecoder from KalmanStats alone.  After fit(): A, W [K, K], H [C', K], Q [C', C'] over the C'
    channels that are not constant (`kept`, their indices), gain = M = H^T Q^-1 [K, C'], G = M H; m [K, C] and m0 [K],
    which apply to raw clipped counts: M z_t = m0 + m min(x_t, clip), a zero column for a dropped channel; mean_y [K], the
    training mean of the states; lead, clip, channels.  All float64, on the device of the statistics."""

    def __init__(self, alpha=0.0):
        if alpha < 0:
            raise ValueError("alpha is not negative")
        self.alpha = float(alpha)
        self.A = self.W = self.H = self.Q = self.gain = self.G = self.m = self.m0 = self.mean_y = self.kept = None
        self.lead = self.clip = self.channels = None
        self._table = None

    def fit(self, stats):  # noqa: A002
        ks = stats[0] if isinstance(stats, (list, tuple)) and len(stats) == 1 else stats
        if not isinstance(ks, KalmanStats) or ks.w.n < 3 or ks.n_pairs < 2:
            raise ValueError("fit takes the KalmanStats of at least three bins and two pairs")
        s = ks.w
        if s.lags != 1 or s.window != 1:
            raise ValueError("the observation is one bin of every channel: statistics at one lag, without a window")
        n = float(s.n)
        G, sx = s.gram.double(), s.sum_x.double()
        mean = sx / n
        # constant channels are dropped, as WienerFilter.fit decides it
        diag = torch.diagonal(s.gram)
        if s.n * s.clip * s.clip * s.n < 2 ** 63:
            keep = (s.n * diag - s.sum_x * s.sum_x) > 0
        else:
            num = n * diag.double() - sx * sx
            keep = num > 2.0 ** -40 * n * diag.double()
        idx = torch.nonzero(keep).flatten()
        if idx.numel() == 0:
            raise ValueError("every channel is constant: nothing to fit")
        K = int(s.xty.shape[1])
        eye = torch.eye(K, dtype=torch.float64, device=G.device)
        mu = mean[idx]
        std = torch.sqrt(torch.diagonal(G)[idx] / n - mu * mu)                     # ddof = 0
        ybar = s.sum_y / n
        # the observation model: ridge with intercept of the z-scored counts on the states, then the residuals' covariance
        czz = (G[idx][:, idx] - n * mu.unsqueeze(1) * mu.unsqueeze(0)) / (std.unsqueeze(1) * std.unsqueeze(0))
        cxx = s.sum_yy - n * ybar.unsqueeze(1) * ybar.unsqueeze(0)
        czx = (s.xty[idx] - mu.unsqueeze(1) * s.sum_y.unsqueeze(0)) / std.unsqueeze(1)
        H = torch.linalg.solve(cxx + self.alpha * eye, czx.t()).t()
        Q = (czz - H @ czx.t() - czx @ H.t() + H @ cxx @ H.t()) / (n - 1.0)       # ddof = 1
        # the state model, from the pairs and their steps d = b - a.  Ridge of b on a gives A^T = (caa + alpha I)^-1 cab
        # with cab = caa + cad, so A = I + E with E^T = (caa + alpha I)^-1 (cad - alpha I); what is left of b is what is
        # left of d after E a, and its covariance comes from the steps' own moments without cancellation.
        p = float(ks.n_pairs)
        ma, md = ks.sum_a / p, ks.sum_d / p
        caa = ks.aa - p * ma.unsqueeze(1) * ma.unsqueeze(0)
        cdd = ks.dd - p * md.unsqueeze(1) * md.unsqueeze(0)
        cad = ks.ad - p * ma.unsqueeze(1) * md.unsqueeze(0)
        E = torch.linalg.solve(caa + self.alpha * eye, cad - self.alpha * eye).t()
        A = eye + E
        W = (cdd - E @ cad - cad.t() @ E.t() + E @ caa @ E.t()) / (p - 1.0)
        chol = _chol(Q, "the observation noise covariance Q")
        M = torch.cholesky_solve(H, chol).t()                                      # H^T Q^-1
        self.A, self.W, self.H, self.Q, self.gain, self.G = A, W, H, Q, M, M @ H
        m = torch.zeros((K, s.channels), dtype=torch.float64, device=G.device)
        m[:, idx] = M / std.unsqueeze(0)
        self.m, self.m0, self.mean_y, self.kept = m.contiguous(), -(m * mean.unsqueeze(0)).sum(1), ybar, idx
        self.lead, self.clip, self.channels = s.lead, s.clip, s.channels
        self._table = None
        return self

    def gains(self, tol=2.0 ** -50):
        """-> (F, B), float64 numpy [n, K, K]: B_t = (I + P_t^- G)^-1 P_t^- and F_t = (I - B_t G) A for the steps t = 0, 1,
        .. after a restart (P = 0, so P_0^- = W), iterated on the host.  The table ends with the first step whose B and F
        both differ from the step before by at most tol times their largest entry: that step serves every later one."""
        from ._kalman import MAX_GAINS
        if self.A is None:
            raise ValueError("gains come after fit")
        A, W, G = self.A.cpu().numpy(), self.W.cpu().numpy(), self.G.cpu().numpy()
        eye = np.eye(A.shape[0])
        P = W.copy()
        Fs, Bs, change = [], [], np.inf
        for _step in range(MAX_GAINS):
            B = np.linalg.solve(eye + P @ G, P)
            low = eye - B @ G
            F = low @ A
            if Fs:
                db, df = np.abs(B - Bs[-1]).max(), np.abs(F - Fs[-1]).max()
                change = max(db / max(np.abs(B).max(), 1e-300), df / max(np.abs(F).max(), 1e-300))
            Fs.append(F), Bs.append(B)
            if change <= tol:
                return np.stack(Fs), np.stack(Bs)
            P = A @ (low @ P) @ A.T + W
        raise ValueError("the gains still change by %.3g of their largest entry after %d steps: use a tol above that"
                         % (change, MAX_GAINS))

    def _device_table(self, device):
        if self._table is None or self._table[0].device != device:
            F, B = self.gains()
            self._table = (torch.from_numpy(F).to(device).contiguous(), torch.from_numpy(B).to(device).contiguous())
        return self._table

    def predict(self, x, y0=None, ranges=None):
        """-> float64 [K, T]: column t estimates y[:, t + lead].  ranges: ascending, disjoint ranges [a, b) of columns
        (default the whole recording); every range restarts the filter (P = 0, the first entry of the gain table) from
        y0[r] ([ranges, K]; default the training mean), which is also its first column.  Columns outside every range are
        NaN.  One mhk_project and one mhk_scan per 16 ranges; the training mean is added back."""
        from . import _kalman
        if self.A is None:
            raise ValueError("predict comes after fit")
        x, rows, cols = _matrix(x, "KalmanFilter.predict")
        dev = x.device
        rs, init = self._scan_args(rows, cols, dev, y0, ranges)
        v = torch.empty((int(self.A.shape[0]), cols), dtype=torch.float64, device=dev)
        _kalman.project(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, self.clip, self.m.to(dev), self.m0.to(dev), v)
        return self._scan(v, cols, rs, init)

    def predict_from(self, src, y0=None, ranges=None):
        """predict on the bins of a gram.BinSource (archive.Reader.bins, container_io.bins), without holding them: one
        mhk_project per batch into its columns of v [K, n], then the scans over the whole of v as in predict.  With
        ranges only the batches that hold a bin of one are read."""
        from . import _kalman
        from .gram import walk_ranges
        if self.A is None:
            raise ValueError("predict comes after fit")
        rows, cols = wiener._source(src, "KalmanFilter.predict_from")
        dev = src.device
        rs, init = self._scan_args(rows, cols, dev, y0, ranges)
        K = int(self.A.shape[0])
        whole = len(rs) == 1 and rs[0] == (0, cols)
        v = (torch.empty if whole else torch.zeros)((K, cols), dtype=torch.float64, device=dev)
        m, m0 = self.m.to(dev), self.m0.to(dev)
        for b0, nb, h, view, _pieces in walk_ranges(src, 0, rs):
            _kalman.project(view.data_ptr() + h, view.stride(0) if rows > 1 else nb, rows, nb, self.clip, m, m0, v[:, b0:b0 + nb])
        return self._scan(v, cols, rs, init)

    def _scan_args(self, rows, cols, dev, y0, ranges):
        """the checks of predict behind the counts' shape -> (ranges, the centred first states [ranges, K])"""
        if rows != self.channels:
            raise ValueError("the filter was fitted on %d channels, not %d" % (self.channels, rows))
        K = int(self.A.shape[0])
        rs = [(0, cols)] if ranges is None else [(int(a), int(b)) for a, b in ranges]
        prev = 0
        for a, b in rs:
            if not prev <= a <= b <= cols:
                raise ValueError("the ranges are ascending, disjoint and inside the %d bins" % cols)
            prev = b
        mean = self.mean_y.to(dev)
        if y0 is None:
            init = torch.zeros((len(rs), K), dtype=torch.float64, device=dev)
        else:
            init = (torch.as_tensor(y0, device=dev).double().reshape(len(rs), K) - mean.unsqueeze(0)).contiguous()
        return rs, init

    def _scan(self, v, cols, rs, init):
        """predict behind mhk_project: v float64 [K, cols], projected wherever a range lies -> the prediction"""
        from . import _kalman
        dev, K = v.device, int(v.shape[0])
        mean = self.mean_y.to(dev)
        F, B = self._device_table(dev)
        whole = len(rs) == 1 and rs[0] == (0, cols)
        out = v if whole else torch.full((K, cols), float("nan"), dtype=torch.float64, device=dev)
        n = min(len(rs), _kalman.MAX_RANGES)
        scratch = torch.empty((max(_kalman.scan_scratch_bytes(cols, K, n), 8),), dtype=torch.uint8, device=dev)
        for i in range(0, len(rs), _kalman.MAX_RANGES):
            _kalman.scan(v, rs[i:i + n], F, B, init[i:i + n], out, scratch)
        out += mean.unsqueeze(1)
        return out

    def score(self, x, y, ranges=None):
        """-> (rmse, cc), float64 [ranges, K]: the root mean squared error and Pearson's r of the prediction over every
        range [a, b) of columns against y[:, a + lead : b + lead].  Every range starts from the TRUE first state, as the
        reference's predict(X_test, y_test) does, and that first column is counted, as the reference counts it."""
        x, _rows, cols = _matrix(x, "KalmanFilter.score")
        y, _K = wiener._covariates(y, x, cols)
        rs, y0 = self._scored(y, cols, ranges)
        return self._score(self.predict(x, y0, rs), y, rs)

    def score_from(self, src, y, ranges=None):
        """score with the counts in a gram.BinSource: the prediction is predict_from's"""
        _rows, cols = wiener._source(src, "KalmanFilter.score_from")
        y, _K = wiener._source_covariates(y, src)
        rs, y0 = self._scored(y, cols, ranges)
        return self._score(self.predict_from(src, y0, rs), y, rs)

    def _scored(self, y, cols, ranges):
        g = self.lead
        rs = [(0, cols - g)] if ranges is None else [(int(a), int(b)) for a, b in ranges]
        if any(b + g > cols or b <= a for a, b in rs):
            raise ValueError("a scored range holds a bin and its targets lie inside the recording")
        return rs, torch.stack([y[:, a + g] for a, _b in rs]).double()

    def _score(self, pred, y, rs):
        g = self.lead
        rmse, cc = [], []
        for a, b in rs:
            p, t = pred[:, a:b], y[:, a + g:b + g].double()
            rmse.append(torch.sqrt(((p - t) ** 2).mean(1)))
            pc, tc = p - p.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
            cc.append((pc * tc).sum(1) / torch.sqrt((pc * pc).sum(1) * (tc * tc).sum(1)))
        return torch.stack(rmse), torch.stack(cc)


def cross_validate(x, y, lead=0, clip=None, alphas=(0.0,), num_fold=5):
    """The study's cross-validation of the Kalman decoder -> dict(rmse_valid, rmse_test, cc_valid, cc_test), each float64
    [len(alphas), num_fold, K] on the device: split i validates on fold i, tests on fold i + 1 (cyclically) and trains on
    the others (wiener.folds).  One stats() pass over the folds; per split the sum of the training folds' KalmanStats
    (without the pairs across their junctions, see KalmanStats.__add__); per (split, alpha) one fit, one gain table and
    one score over the two held-out folds."""
    x, rows, cols = _matrix(x, "kalman.cross_validate")
    y, K = wiener._covariates(y, x, cols)
    _L, g = wiener._settings(1, lead, rows, cols)
    alphas, num_fold = [float(a) for a in alphas], int(num_fold)
    if not alphas or len(set(alphas)) != len(alphas) or num_fold < 3:
        raise ValueError("at least one alpha, each once, and at least 3 folds")
    fr = wiener.fold_ranges(cols - g, num_fold)
    st = stats(x, y, g, clip, fr)
    return _validate_folds(st, fr, alphas, K, x.device, lambda f, rs: f.score(x, y, rs))


def _validate_folds(st, fr, alphas, K, device, score):
    """cross_validate behind its statistics: st the KalmanStats of the folds fr, score(filter, ranges) the fitted
    filter's score over the held-out folds"""
    num_fold = len(fr)
    res = {k: torch.empty((len(alphas), num_fold, K), dtype=torch.float64, device=device)
           for k in ("rmse_valid", "rmse_test", "cc_valid", "cc_test")}
    for i in range(num_fold):
        v, t = i, (i + 1) % num_fold
        tot = sum(st[k] for k in range(num_fold) if k not in (v, t))
        held = sorted((v, t))
        iv, it = held.index(v), held.index(t)
        for j, a in enumerate(alphas):
            rmse, cc = score(KalmanFilter(a).fit(tot), [fr[k] for k in held])
            res["rmse_valid"][j, i], res["rmse_test"][j, i] = rmse[iv], rmse[it]
            res["cc_valid"][j, i], res["cc_test"][j, i] = cc[iv], cc[it]
    return res


def stats_from(src, y, lead=0, clip=None, ranges=None):
    """stats() with the counts in a gram.BinSource (archive.Reader.bins, container_io.bins) -> [KalmanStats]: the count
    statistics are wiener.stats_from at one lag, one pass over the bins the ranges hold; the pair moments are those of
    y, which is resident.  y: float32 [K, src.n] on the source's bin grid."""
    _rows, cols = wiener._source(src, "kalman.stats_from")
    ws = wiener.stats_from(src, y, 1, lead, clip, ranges)
    y, _K = wiener._source_covariates(y, src)
    g = int(lead)
    return [KalmanStats(w, *_pair_moments(y[:, a + g:b + g].double()))
            for (a, b), w in zip(wiener._ranges(ranges, 1, g, cols), ws)]


def cross_validate_from(src, y, lead=0, clip=None, alphas=(0.0,), num_fold=5):
    """cross_validate with the counts in a gram.BinSource -> the same dict.  One pass over the source for the fold
    statistics; per (split, alpha) KalmanFilter.score_from reads the two held-out folds again for its projection."""
    rows, cols = wiener._source(src, "kalman.cross_validate_from")
    y, K = wiener._source_covariates(y, src)
    _L, g = wiener._settings(1, lead, rows, cols)
    alphas, num_fold = [float(a) for a in alphas], int(num_fold)
    if not alphas or len(set(alphas)) != len(alphas) or num_fold < 3:
        raise ValueError("at least one alpha, each once, and at least 3 folds")
    fr = wiener.fold_ranges(cols - g, num_fold)
    st = stats_from(src, y, g, clip, fr)
    return _validate_folds(st, fr, alphas, K, y.device, lambda f, rs: f.score_from(src, y, rs))
