"""The Wiener cascade of the behavioural study on the device: the linear filter of wiener.py followed by a polynomial per
output, and the scores of both per range of design rows.

moments() gives, per range of columns, the power sums of a prediction p against its target y (mhc_moments): T_i = sum
u^i, Q_i = sum u^i y, sum y^2 and sum (u - y)^2 with u = (p - center) / scale.  They are all a polynomial fit of y on u
(polyfit(): Hankel normal equations, any degree up to the one asked for), the root mean squared error and Pearson's r
need, they are float64 and deterministic, and Moments of disjoint ranges add: a fold's training ranges cost one pass.
WienerCascade fits the polynomial from them and applies it in place behind mhw_fir (mhc_polyval); cross_validate() runs
the study's loop over folds, alphas and degrees and returns its four arrays.  There is no CPU path: host matrices are
refused.

Columns and design rows are wiener.py's: with L lags and a lead of g bins, prediction column i belongs to design row
i + L-1 and its target is y[:, i + L-1 + g]."""
import torch

from . import wiener
from .windows import _matrix


class Moments:
    """The power sums of n columns per (range, output).  t float64 [R, K, 2D+1] (t[..., 0] = n), q [R, K, D+1], yy and err
    [R, K]; degree D; ranges: per leading index the list of (a, b) column ranges summed there.  total() drops the leading
    axis.  err is the sum of (u - y)^2: an error of the prediction itself only where no center or scale was given."""

    def __init__(self, t, q, yy, err, degree, ranges):
        self.t, self.q, self.yy, self.err, self.degree, self.ranges = t, q, yy, err, int(degree), ranges

    def __add__(self, other):
        """Two results over the same outputs, degree, center and scale and disjoint columns -> the result over both"""
        if not isinstance(other, Moments):
            return NotImplemented
        if self.degree != other.degree or self.t.shape != other.t.shape:
            raise ValueError("the two results are not over the same outputs, degree and number of ranges")
        if self.t.dim() == 3:
            ranges = [list(a) + list(b) for a, b in zip(self.ranges, other.ranges)]
        else:
            ranges = list(self.ranges) + list(other.ranges)
        return Moments(self.t + other.t, self.q + other.q, self.yy + other.yy, self.err + other.err, self.degree, ranges)

    def __radd__(self, other):  # sum() starts from 0
        return self if other == 0 else NotImplemented

    def __getitem__(self, r):
        """the result of range r alone, without the leading axis"""
        if self.t.dim() != 3:
            raise ValueError("total() has been taken: there is no axis of ranges")
        return Moments(self.t[r], self.q[r], self.yy[r], self.err[r], self.degree, list(self.ranges[r]))

    def total(self):
        """the sum over the ranges -> Moments without the leading axis"""
        if self.t.dim() != 3:
            return self
        return Moments(self.t.sum(0), self.q.sum(0), self.yy.sum(0), self.err.sum(0), self.degree, [ab for r in self.ranges for ab in r])

    @property
    def n(self):
        return self.t[..., 0]

    def rmse(self):
        """sqrt(E / n), float64 [R, K]"""
        return torch.sqrt(self.err / self.n)

    def cc(self):
        """Pearson's r of u against y from the sums, float64 [R, K]: (n Q_1 - T_1 Q_0) / sqrt((n T_2 - T_1^2)(n YY - Q_0^2))"""
        n, t1, t2, q0, q1 = self.n, self.t[..., 1], self.t[..., 2], self.q[..., 0], self.q[..., 1]
        return (n * q1 - t1 * q0) / torch.sqrt((n * t2 - t1 * t1) * (n * self.yy - q0 * q0))


def _rows(p, what):
    if not (isinstance(p, torch.Tensor) and p.is_cuda):
        raise ValueError("%s is a device tensor: there is no CPU path" % what)
    if p.dim() == 1:
        p = p.unsqueeze(0)
    if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] < 1:
        raise ValueError("%s is a float32 tensor [K, columns]" % what)
    if p.shape[1] > 1 and p.stride(1) != 1:
        raise ValueError("the columns of %s lie back to back (unit stride along the last axis)" % what)
    return p


def _degree(degree):
    from ._cascade import MAX_DEGREE
    d = int(degree)
    if not 1 <= d <= MAX_DEGREE:
        raise ValueError("degree %d outside 1..%d" % (d, MAX_DEGREE))
    return d


def _column_ranges(ranges, cols):
    if ranges is None:
        return [(0, cols)]
    out = [(int(a), int(b)) for a, b in ranges]
    end = 0
    for a, b in out:
        if not end <= a <= b <= cols:
            raise ValueError("range [%d, %d) is not inside the columns [0, %d), or not behind the one in front" % (a, b, cols))
        end = b
    if not out:
        raise ValueError("at least one range")
    return out


def moments(p, y, ranges=None, degree=1, center=None, scale=None):
    """The power sums of the prediction p against the target y -> Moments with one leading index per range.  p, y: float32
    device tensors [K, columns] (or [columns]) of one shape, unit stride along the last axis, any pitch; ranges: [(a, b)] of
    columns, ascending and disjoint (default: all columns); degree 1..6; center, scale: None or float64 [K], u = (p -
    center) / scale (the kernel multiplies by 1 / scale, taken in float64)."""
    from . import _cascade
    p, y = _rows(p, "the prediction"), _rows(y, "the target")
    if y.device != p.device or y.shape != p.shape:
        raise ValueError("the prediction and the target have one shape and one device")
    K, cols = int(p.shape[0]), int(p.shape[1])
    if not 1 <= K <= _cascade.MAX_K:
        raise ValueError("%d outputs outside 1..%d" % (K, _cascade.MAX_K))
    D = _degree(degree)
    rs = _column_ranges(ranges, cols)
    dev = p.device
    c = None if center is None else torch.as_tensor(center, dtype=torch.float64, device=dev).reshape(K).contiguous()
    s = None if scale is None else (1.0 / torch.as_tensor(scale, dtype=torch.float64, device=dev).reshape(K)).contiguous()
    per = _cascade.per(D)
    out = torch.empty((len(rs), K, per), dtype=torch.float64, device=dev)
    for i in range(0, len(rs), _cascade.MAX_RANGES):
        part = rs[i:i + _cascade.MAX_RANGES]
        scratch = torch.empty((max(_cascade.moments_scratch_bytes(cols, K, D, len(part)), 8),), dtype=torch.uint8, device=dev)
        _cascade.moments(p, y, part, D, c, s, out[i:i + len(part)], scratch)
    return Moments(out[..., :2 * D + 1], out[..., 2 * D + 1:3 * D + 2], out[..., 3 * D + 2], out[..., 3 * D + 3], D, [[ab] for ab in rs])


def polyfit(moments, degree):  # noqa: A002
    """The least-squares polynomial of y on u from the sums -> float64 [R, K, degree + 1] ([K, degree + 1] after total()),
    the highest power first as numpy.polyfit gives it.  Normal equations H c = Q with the Hankel matrix H[a][b] = T_(a+b),
    a, b = 0..degree, solved by Cholesky in float64; degree may be below the one the sums were taken at (the leading
    block).  Runs where the sums are: on host tensors too."""
    m, d = moments, _degree(degree)
    if not isinstance(m, Moments) or d > m.degree:
        raise ValueError("polyfit takes Moments of at least the degree asked for")
    if float(m.n.min()) < 1:
        raise ValueError("polyfit takes the Moments of at least one column per range")
    ab = torch.arange(d + 1, device=m.t.device)
    h = m.t[..., ab.unsqueeze(1) + ab.unsqueeze(0)]                                # [..., d+1, d+1]
    rhs = m.q[..., :d + 1].unsqueeze(-1)
    chol, info = torch.linalg.cholesky_ex(h)
    # not positive definite, or only by rounding: a pivot at the level of the factorisation's own error (WienerFilter.fit)
    diag = torch.diagonal(h, dim1=-2, dim2=-1)
    floor = 64 * 2.0 ** -52 * (d + 1) * diag.max(-1).values
    pivots = (torch.diagonal(chol, dim1=-2, dim2=-1) ** 2).min(-1).values
    if bool((info != 0).any()) or bool((pivots <= floor).any()):
        raise ValueError("the polynomial's normal equations are not positive definite (too few distinct predictions, or "
                         "sums taken without center and scale): use a lower degree")
    return torch.flip(torch.cholesky_solve(rhs, chol).squeeze(-1), [-1])


def _linear_spread(s, f):
    """The mean and the standard deviation (ddof 0) of the linear prediction over the design rows of the Stats s the
    filter f was fitted on, from the statistics and the weights alone -> float64 [K] each.  The mean is bias + w . mean(x),
    which is mean(y) by the intercept's construction; the variance w^T Cov(x) w."""
    n = float(s.n)
    w = f.weights.reshape(f.weights.shape[0], -1)                                  # [K, L*C], feature l*C + c
    mean = s.sum_x.double() / n
    wm = w @ mean
    var = ((w @ s.gram.double()) * w).sum(1) / n - wm * wm
    if not bool((var > 0).all()):
        raise ValueError("the linear prediction is constant on the training rows: there is no polynomial to fit")
    return f.bias + wm, torch.sqrt(var)


class WienerCascade:
    """WienerFilter followed by a polynomial of the given degree per output (the study's WienerCascadeDecoder).  After
    fit(): linear (the WienerFilter), center and scale float64 [K], coef float64 [K, degree + 1] (highest power first):
    the estimate is polyval(coef[k], (linear estimate - center[k]) / scale[k])."""

    def __init__(self, alpha=0.0, degree=3):
        self.linear = wiener.WienerFilter(alpha)
        self.degree = _degree(degree)
        self.center = self.scale = self.coef = None

    def _targets(self, pred, y):
        """the views [K, n] of the prediction and of the covariates whose columns belong together"""
        L, g = self.linear.lags, self.linear.lead
        y = _rows(y, "the covariates")
        n = pred.shape[1] - g
        if n < 1 or y.shape[0] != pred.shape[0] or y.shape[1] != pred.shape[1] + L - 1 or y.device != pred.device:
            raise ValueError("counts and covariates do not match, or no target lies inside them")
        return pred[:, :n], y[:, L - 1 + g:], n

    def _columns(self, ranges, n):
        """ranges of design rows -> ranges of prediction columns"""
        L = self.linear.lags
        if ranges is None:
            return [(0, n)]
        rs = [(int(a), int(b)) for a, b in ranges]
        for a, b in rs:
            if a < L - 1:
                raise ValueError("range [%d, %d) starts before the first design row %d" % (a, b, L - 1))
        return _column_ranges([(a - (L - 1), b - (L - 1)) for a, b in rs], n)

    def fit(self, stats, x, y, ranges=None):  # noqa: A002
        """stats: the (summed) wiener.Stats of the training ranges; x, y: the counts and covariates they were taken from;
        ranges: the same ranges of design rows, ascending (default: all design rows).  One solve, one mhw_fir over the
        recording, one mhc_moments over the training ranges, one small solve per output.  The polynomial is fitted in
        u = (prediction - center) / scale with the prediction's own mean and standard deviation on the training rows,
        which keep the Hankel matrix well conditioned; they come from the Stats and the weights (_linear_spread), not
        from a pass over the prediction."""
        s = stats[0] if isinstance(stats, (list, tuple)) and len(stats) == 1 else stats
        self.linear.fit(s)
        return self._fit_stage(s, self.linear.predict(x), y, ranges)

    def _fit_stage(self, s, pred, y, ranges=None):
        """fit behind the linear fit: pred is the fitted linear filter's prediction over the recording (predict, or
        predict_from on a file)"""
        self.center, self.scale = _linear_spread(s, self.linear)
        p, t, n = self._targets(pred, y)
        m = moments(p, t, self._columns(ranges, n), self.degree, self.center, self.scale).total()
        if int(m.n[0]) != s.n:
            raise ValueError("the ranges hold %d design rows, the statistics %d" % (int(m.n[0]), s.n))
        self.coef = polyfit(m, self.degree)
        return self

    def _apply(self, pred, coef, out):
        from . import _cascade
        f32 = lambda v: v.to(device=pred.device, dtype=torch.float32).contiguous()  # noqa: E731
        _cascade.polyval(pred, f32(coef), f32(self.center), f32(1.0 / self.scale), out)
        return out

    def predict(self, x):
        """-> float32 [K, T - L + 1]: column i is the estimate of y[:, i + L-1 + lead].  mhw_fir, then mhc_polyval in place"""
        if self.coef is None:
            raise ValueError("predict comes after fit")
        pred = self.linear.predict(x)
        return self._apply(pred, self.coef, pred)

    def score(self, x, y, ranges=None):
        """-> (rmse, cc), float64 [R, K]: per range of design rows (default: the one range of all of them), from mhc_moments
        at degree 1 on the final prediction"""
        return self._score_stage(self.linear.predict(x), y, ranges)

    def _score_stage(self, pred, y, ranges=None):
        """score behind the linear prediction `pred`, which is overwritten with the cascade's"""
        if self.coef is None:
            raise ValueError("predict comes after fit")
        p, t, n = self._targets(self._apply(pred, self.coef, pred), y)
        m = moments(p, t, self._columns(ranges, n), 1)
        return m.rmse(), m.cc()



def cross_validate(x, y, lags, lead=0, clip=None, alphas=(0.0,), degrees=(3,), num_fold=5, window=1):
    """The study's cross-validation -> {(alpha, degree): dict(rmse_valid, rmse_test, cc_valid, cc_test)}, each float64
    [num_fold, K] on the device: split i validates on fold i, tests on fold i + 1 (cyclically) and trains on the others
    (wiener.folds).  degree None is the linear decoder alone.  One wiener.stats pass; per (fold, alpha) one solve, one
    mhw_fir over the recording and one mhc_moments at the largest degree over the training ranges; per degree one
    mhc_polyval and one mhc_moments over the two held-out folds.

    window > 1 is the study's moving-average window (wiener.stats(window=)); every prediction then passes through
    mhs_box_f32.  With a window a channel that is constant over the recording is a constant FEATURE only behind the
    warm-up of window - 1 rows, where its partial sums still grow.  A fold that holds the warm-up therefore keeps that
    channel's features, and since its lags are exactly collinear there (each is the other, shifted, and all are the same
    ramp), alpha = 0 raises the "not positive definite" error of WienerFilter.fit: use alpha > 0, or ranges that leave
    the warm-up out."""
    x, rows, cols = _matrix(x, "cascade.cross_validate")
    y, K = wiener._covariates(y, x, cols)
    L, g = wiener._settings(lags, lead, rows, cols)
    alphas, degrees, F = _cv_settings(alphas, degrees, num_fold)
    fr = wiener.fold_ranges(cols - g - (L - 1), F, L - 1)
    st = wiener.stats(x, y, L, g, clip, ranges=fr, window=window)
    return _validate_folds(x, y, st, fr, alphas, degrees)


def _cv_settings(alphas, degrees, num_fold):
    alphas, degrees = [float(a) for a in alphas], [None if d is None else _degree(d) for d in degrees]
    if not alphas or not degrees or len(set(alphas)) != len(alphas) or len(set(degrees)) != len(degrees):
        raise ValueError("at least one alpha and one degree, each once")
    if int(num_fold) < 3:
        raise ValueError("%d folds leave none to train on (at least 3)" % int(num_fold))
    return alphas, degrees, int(num_fold)


def _validate_folds(x, y, st, fr, alphas, degrees, predictions=None):
    """cross_validate behind its statistics: st the wiener.Stats of the folds fr (ranges of design rows), x and y the
    checked counts and covariates, alphas and degrees as _cv_settings returns them -> cross_validate's result.
    predictions: None, or what stands in for WienerFilter.predict(x): a function of the list of fitted filters that
    gives their predictions one at a time, in order (the file route, where x is None)"""
    F = len(fr)
    top = max([d for d in degrees if d is not None], default=None)
    names = ("rmse_valid", "rmse_test", "cc_valid", "cc_test")
    res = {(a, d): {k: [] for k in names} for a in alphas for d in degrees}
    fits = []
    for i in range(F):
        v, t = i, (i + 1) % F
        train = [k for k in range(F) if k not in (v, t)]
        tot = sum(st[k] for k in train)
        for a in alphas:
            c = WienerCascade(a, top or 1)
            c.linear.fit(tot)
            if top is not None:
                c.center, c.scale = _linear_spread(tot, c.linear)
            fits.append((i, a, c))
    if predictions is None:
        preds = (c.linear.predict(x) for _i, _a, c in fits)
    else:
        preds = predictions([c.linear for _i, _a, c in fits])
    tmp = None
    for (i, a, c), pred in zip(fits, preds):
        v, t = i, (i + 1) % F
        train = [k for k in range(F) if k not in (v, t)]
        held = sorted((v, t))                                                      # mhc_moments takes ascending ranges
        iv, it = held.index(v), held.index(t)
        p, tg, n = c._targets(pred, y)
        if top is not None:
            m = moments(p, tg, c._columns([fr[k] for k in train], n), top, c.center, c.scale).total()
            if tmp is None:
                tmp = torch.empty_like(pred)
        for d in degrees:
            if d is None:
                q = p
            else:
                q = c._apply(pred, polyfit(m, d), tmp)[:, :n]
            s = moments(q, tg, c._columns([fr[k] for k in held], n), 1)
            rmse, cc = s.rmse(), s.cc()
            r = res[(a, d)]
            r["rmse_valid"].append(rmse[iv]), r["rmse_test"].append(rmse[it])
            r["cc_valid"].append(cc[iv]), r["cc_test"].append(cc[it])
    return {key: {k: torch.stack(vals) for k, vals in r.items()} for key, r in res.items()}


def sweep_clips(x, y, lags, lead=0, clips=range(2, 40), alphas=(0.0,), degrees=(3,), num_fold=5, window=1):
    """The study's dynamic-range sweep (`for S in S_vector: X_in[X_in > S] = S` around the whole grid) -> {clip: what
    cross_validate(x, y, lags, lead, clip, alphas, degrees, num_fold, window) returns}, the same bits.  clips: 1..255,
    strictly ascending (default: S = 2..39).  The fold statistics of all clips come from wiener.iter_stats_clips -- one
    mhq_gram_clips and one mhq_xty_clips per group of clips --; the solves, mhw_fir and the moments per (clip, fold,
    alpha) are cross_validate's own.

    window > 1 clamps before the box sum, so the fused kernels do not apply: that case is the loop over
    wiener.stats(clip=q, window=) it replaces, inside this function."""
    x, rows, cols = _matrix(x, "cascade.sweep_clips")
    y, K = wiener._covariates(y, x, cols)
    L, g = wiener._settings(lags, lead, rows, cols)
    alphas, degrees, F = _cv_settings(alphas, degrees, num_fold)
    qs = wiener._clip_list(clips)
    fr = wiener.fold_ranges(cols - g - (L - 1), F, L - 1)
    if int(window) != 1:
        return {q: _validate_folds(x, y, wiener.stats(x, y, L, g, q, ranges=fr, window=window), fr, alphas, degrees) for q in qs}
    return {q: _validate_folds(x, y, st, fr, alphas, degrees) for q, st in wiener.iter_stats_clips(x, y, L, g, qs, ranges=fr)}


def _source_settings(src, y, lags, lead, alphas, degrees, num_fold, who):
    rows, cols = wiener._source(src, who)
    y, _K = wiener._source_covariates(y, src)
    L, g = wiener._settings(lags, lead, rows, cols)
    alphas, degrees, F = _cv_settings(alphas, degrees, num_fold)
    return y, L, g, alphas, degrees, wiener.fold_ranges(cols - g - (L - 1), F, L - 1)


def cross_validate_from(src, y, lags, lead=0, clip=None, alphas=(0.0,), degrees=(3,), num_fold=5, window=1):
    """cross_validate with the counts in a gram.BinSource (archive.Reader.bins, container_io.bins) -> the same dict.  y:
    float32 [K, src.n] on the source's bin grid.  One pass over the source for the fold statistics (wiener.stats_from),
    then wiener.predict_many_from over the fitted (split, alpha) filters: one more pass per group of them whose
    predictions fit the source's max_bytes.  The polynomial fits and the fold scores run on the resident predictions,
    as in cross_validate."""
    y, L, g, alphas, degrees, fr = _source_settings(src, y, lags, lead, alphas, degrees, num_fold, "cascade.cross_validate_from")
    st = wiener.stats_from(src, y, L, g, clip, ranges=fr, window=window)
    return _validate_folds(None, y, st, fr, alphas, degrees, lambda fs: wiener.iter_predict_from(src, fs))


def sweep_clips_from(src, y, lags, lead=0, clips=range(2, 40), alphas=(0.0,), degrees=(3,), num_fold=5, window=1):
    """sweep_clips with the counts in a gram.BinSource -> {clip: what cross_validate_from gives at that clip}.  The fold
    statistics of all clips come from one pass (wiener.stats_clips_from; with a window, one wiener.stats_from pass per
    clip), the predictions from cross_validate_from's passes per clip."""
    y, L, g, alphas, degrees, fr = _source_settings(src, y, lags, lead, alphas, degrees, num_fold, "cascade.sweep_clips_from")
    qs = wiener._clip_list(clips)
    predictions = lambda fs: wiener.iter_predict_from(src, fs)  # noqa: E731
    if int(window) != 1:
        return {q: _validate_folds(None, y, wiener.stats_from(src, y, L, g, q, ranges=fr, window=window), fr, alphas, degrees,
                                   predictions) for q in qs}
    return {q: _validate_folds(None, y, st, fr, alphas, degrees, predictions)
            for q, st in wiener.stats_clips_from(src, y, L, g, qs, ranges=fr)}
