"""Behavioural decoding from spike counts: the Wiener filter -- a ridge regression of covariates (hand or cursor velocity)
onto the last `lags` bins of every channel -- fitted from sufficient statistics and applied on the device, with no design
matrix ever built.

Counts x are uint8 [C, T], covariates y float32 [K, T].  With L lags, a lead of g >= 0 bins (neural data precede the
kinematics) and a clip q (xq = min(x, q)), DESIGN ROW t, for t in [L-1, T-g), has the features f = l*C + c = xq[c][t-l]
(l = 0..L-1) and the targets y[k][t+g].  A range of design rows is [t0, t1) with L-1 <= t0 <= t1 <= T-g.

stats() gives, per range, what the normal equations need: the exact int64 Gram matrix of the features from mhi_gram
(one call per lag difference plus two small edge terms), the float64 products with the covariates from mhw_xty, and the
covariates' own sums.  Stats of disjoint ranges add, so cross-validation over contiguous folds (folds()) costs one pass
over the recording plus one small solve per fold.  WienerFilter.fit() restates z-scoring, centring and the ridge solve
from the statistics alone; predict() is mhw_fir on raw counts.  stats(window=) adds the study's moving-average window:
the features become box sums of the clipped counts (mhs_box, smooth.py), predict() the box sum of mhw_fir's output
(mhs_box_f32).  iter_stats_clips() / stats_clips() are stats() for a whole list of clips -- the study's dynamic-range sweep --
from one mhq_gram_clips and one mhq_xty_clips per group of clips.  stats_from(), stats_clips_from(), predict_from() and
predict_many_from() are the same on a gram.BinSource -- a recording file walked in batches, never resident (the end of
this module).  There is no CPU path: host matrices are refused."""
import numpy as np
import torch

from .windows import MAX_BYTES, _matrix

MAX_FEATURES = 16384  # lags * channels at most: the int64 Gram matrix is then 2 GiB


class Stats:
    """The sufficient statistics of n design rows.  sum_x int64 [L*C], gram int64 [L*C, L*C], xty float64 [L*C, K], sum_y
    float64 [K], sum_yy float64 [K, K]; lags, lead, clip (1..255, 255 = none), channels; window (1 = none): the features
    are the integer sums of `window` clipped bins, at most window * clip."""

    def __init__(self, n, sum_x, gram, xty, sum_y, sum_yy, lags, lead, clip, channels, window=1):
        self.n, self.sum_x, self.gram, self.xty, self.sum_y, self.sum_yy = int(n), sum_x, gram, xty, sum_y, sum_yy
        self.lags, self.lead, self.clip, self.channels, self.window = int(lags), int(lead), int(clip), int(channels), int(window)

    def __add__(self, other):
        """Two results over the same channels, covariates and settings and disjoint design rows -> the result over both"""
        if not isinstance(other, Stats):
            return NotImplemented
        if ((self.lags, self.lead, self.clip, self.channels, self.window)
                != (other.lags, other.lead, other.clip, other.channels, other.window) or self.xty.shape != other.xty.shape):
            raise ValueError("the two results are not over the same features and targets")
        return Stats(self.n + other.n, self.sum_x + other.sum_x, self.gram + other.gram, self.xty + other.xty,
                     self.sum_y + other.sum_y, self.sum_yy + other.sum_yy, self.lags, self.lead, self.clip, self.channels,
                     self.window)

    def __radd__(self, other):  # sum() starts from 0
        return self if other == 0 else NotImplemented

    def to(self, device):
        m = lambda t: t.to(device)  # noqa: E731
        return Stats(self.n, m(self.sum_x), m(self.gram), m(self.xty), m(self.sum_y), m(self.sum_yy), self.lags, self.lead,
                     self.clip, self.channels, self.window)


def _clip(clip):
    q = 255 if clip is None else int(clip)
    if not 1 <= q <= 255:
        raise ValueError("clip %d outside 1..255" % q)
    return q


def _covariates(y, x, cols):
    if not (isinstance(y, torch.Tensor) and y.is_cuda):
        raise ValueError("covariates are a device tensor: there is no CPU path")
    if y.dim() == 1:
        y = y.unsqueeze(0)
    if y.dtype != torch.float32 or y.dim() != 2:
        raise ValueError("covariates are a float32 tensor [K, bins]")
    if y.device != x.device:
        raise ValueError("counts and covariates are on the same device")
    from ._wiener import MAX_K
    K = int(y.shape[0])
    if not 1 <= K <= MAX_K:
        raise ValueError("%d covariates outside 1..%d" % (K, MAX_K))
    if int(y.shape[1]) != cols:
        raise ValueError("counts and covariates have the same number of bins (%d, %d)" % (cols, int(y.shape[1])))
    if cols > 1 and y.stride(1) != 1:
        raise ValueError("the bins of a covariate lie back to back (unit stride along the last axis)")
    return y, K


def _settings(lags, lead, rows, cols):
    from ._wiener import MAX_LAGS, MAX_ROWS
    L, g = int(lags), int(lead)
    if not 1 <= L <= MAX_LAGS:
        raise ValueError("lags %d outside 1..%d" % (L, MAX_LAGS))
    if g < 0:
        raise ValueError("lead %d is negative" % g)
    if rows > MAX_ROWS:
        raise ValueError("%d channels above %d" % (rows, MAX_ROWS))
    if L * rows > MAX_FEATURES:
        raise ValueError("lags * channels = %d above %d" % (L * rows, MAX_FEATURES))
    if cols - g < L:
        raise ValueError("%d bins leave no design row at lags %d, lead %d" % (cols, L, g))
    return L, g


def _ranges(ranges, L, g, cols):
    if ranges is None:
        return [(L - 1, cols - g)]
    out = [(int(a), int(b)) for a, b in ranges]
    for a, b in out:
        if not L - 1 <= a <= b <= cols - g:
            raise ValueError("range [%d, %d) is not inside the design rows [%d, %d)" % (a, b, L - 1, cols - g))
    return out


def _edge_products(xe, L, d):
    """xe: int64 [C, L-1], the clipped columns [e-(L-1), e) before an edge e.  -> int64 [L-d, C, C]: entry l1 is
    F_d(e-l1, e) = sum over u in [e-l1, e) of x[:, u] x[:, u-d]^T (entry 0 is zero); l1 + d <= L-1, so no column before
    e-(L-1) is needed."""
    n = xe.shape[1]
    a = xe[:, n - (L - 1 - d):]                        # u = e-(L-1-d) .. e-1
    b = xe[:, n - (L - 1 - d) - d:n - d]               # u - d
    outer = a.t().unsqueeze(2) * b.t().unsqueeze(1)    # [L-1-d, C, C], in ascending u
    cum = torch.flip(torch.cumsum(torch.flip(outer, [0]), 0), [0])  # entry i: the sum over u >= e-(L-1-d)+i
    zero = torch.zeros((1,) + tuple(outer.shape[1:]), dtype=torch.int64, device=xe.device)
    return torch.flip(torch.cat([cum, zero], 0), [0])  # entry l1: the sum over u in [e-l1, e)


def _range_stats(x, rows, y, K, L, g, q, t0, t1, max_bytes, scratch_xty):
    dev, n, F = x.device, t1 - t0, L * rows
    xty = torch.zeros((F, K), dtype=torch.float64, device=dev)
    yr = y[:, t0 + g:t1 + g].double()
    sum_y, sum_yy = yr.sum(1), yr @ yr.t()
    if n == 0:
        G = torch.zeros((F, F), dtype=torch.int64, device=dev)
        sx = torch.zeros((F,), dtype=torch.int64, device=dev)
        return Stats(0, sx, G, xty, sum_y, sum_yy, L, g, q, rows)
    base, s0 = _range_parts(x, rows, y, K, L, g, q, t0, t1, max_bytes, scratch_xty, xty)
    # ---- the edges: at most L - 1 outer products on either side
    lo = torch.clamp(x[:, t0 - (L - 1):t0], max=q).long()        # columns [t0-(L-1), t0): all that is read before t0
    hi = torch.clamp(x[:, t1 - (L - 1):t1], max=q).long()
    G, sx = _assemble(base, s0, lo, hi, L, rows)
    return Stats(n, sx, G, xty, sum_y, sum_yy, L, g, q, rows)


def _range_parts(x, rows, y, K, L, g, q, t0, t1, max_bytes, scratch_xty, xty):
    """What the design rows [t0, t1), t1 > t0, give before their edges are known: xty [L*C, K] (written) and -> (base int64
    [L, C, C], the count products F_d(t0, t1) per lag difference d; s0 int64 [C], the row sums over [t0, t1)).  Both add
    over adjoining ranges, which _assemble does not need to see one by one: only the first range's columns before t0
    and the last one's before t1."""
    from . import _wiener
    from .gram import batches, enqueue
    dev, n = x.device, t1 - t0
    # ---- the float part: one call, out [L, C, K] is xty's own layout
    _wiener.xty(x.data_ptr() + t0 - (L - 1), x.stride(0) if rows > 1 else n + L - 1, rows, n, L, q,
                y.data_ptr() + 4 * (t0 + g), 4 * y.stride(0) if K > 1 else 4 * n, K, xty, scratch_xty)
    # ---- the integer part: F_d(t0, t1) for every lag difference d, with the row sums of the d = 0 call
    base = torch.zeros((L, rows, rows), dtype=torch.int64, device=dev)
    s0 = torch.zeros((rows,), dtype=torch.int64, device=dev)
    if q == 255:
        for d in range(L):
            if d == 0:
                enqueue(x, rows, n, None, 0, base[0], s0, None, False, t0)
            else:
                enqueue(x, rows, n, x, rows, base[d], None, None, False, t0, t0 - d)
    else:  # mhi_gram has no clip: a clamped copy, in column batches, added up
        plan = batches(n, rows, max_bytes)
        scratch = torch.empty((rows, plan[0][1] + L - 1), dtype=torch.uint8, device=dev)
        for b0, nb in plan:
            view = scratch[:, :nb + L - 1]
            view.copy_(torch.clamp(x[:, t0 + b0 - (L - 1):t0 + b0 + nb], max=q))
            for d in range(L):
                if d == 0:
                    enqueue(view, rows, nb, None, 0, base[0], s0, None, True, L - 1)
                else:
                    enqueue(view, rows, nb, view, rows, base[d], None, None, True, L - 1, L - 1 - d)
    return base, s0


def _assemble(base, s0, lo, hi, L, rows):
    """base int64 [L, C, C]: F_d(t0, t1) per lag difference d; s0 int64 [C]: the row sums over [t0, t1); lo, hi: int64
    [C, L-1], the L-1 columns before t0 and before t1 -> (gram [L*C, L*C], sum_x [L*C]) of the design rows [t0, t1)"""
    dev, F = base.device, L * rows
    G = torch.zeros((F, F), dtype=torch.int64, device=dev)
    for d in range(L):
        blocks = base[d].unsqueeze(0) + _edge_products(lo, L, d) - _edge_products(hi, L, d)   # [L-d, C, C]: l1 = 0..L-1-d
        for l1 in range(L - d):
            r, c = l1 * rows, (l1 + d) * rows
            G[r:r + rows, c:c + rows] = blocks[l1]
            if d:
                G[c:c + rows, r:r + rows] = blocks[l1].t()
    zero = torch.zeros((rows, 1), dtype=torch.int64, device=dev)
    before = torch.cat([zero, torch.cumsum(torch.flip(lo, [1]), 1)], 1)   # [:, l]: the sum over [t0-l, t0)
    after = torch.cat([zero, torch.cumsum(torch.flip(hi, [1]), 1)], 1)
    sx = (s0.unsqueeze(0) + before.t() - after.t()).reshape(F).contiguous()
    return G, sx


def _edge_products_clips(xe, L, d):
    """_edge_products with leading axes: xe int64 [..., C, L-1] -> int64 [..., L-d, C, C]"""
    n = xe.shape[-1]
    a = xe[..., n - (L - 1 - d):].transpose(-1, -2)                 # [..., L-1-d, C]: u = e-(L-1-d) .. e-1
    b = xe[..., n - (L - 1 - d) - d:n - d].transpose(-1, -2)        # u - d
    outer = a.unsqueeze(-1) * b.unsqueeze(-2)                       # [..., L-1-d, C, C], in ascending u
    cum = torch.flip(torch.cumsum(torch.flip(outer, [-3]), -3), [-3])
    zero = torch.zeros(tuple(outer.shape[:-3]) + (1,) + tuple(outer.shape[-2:]), dtype=torch.int64, device=xe.device)
    return torch.flip(torch.cat([cum, zero], -3), [-3])


def _assemble_clips(base, s0, lo, hi, L, rows):
    """_assemble with leading axes (range, clip): base int64 [..., L, C, C], s0 [..., C], lo, hi [..., C, L-1] ->
    (gram [..., L*C, L*C], sum_x [..., L*C]).  Integers: the same values as _assemble gives slice by slice."""
    dev, F, lead = base.device, L * rows, tuple(base.shape[:-3])
    G = torch.zeros(lead + (F, F), dtype=torch.int64, device=dev)
    for d in range(L):
        blocks = base[..., d, :, :].unsqueeze(-3) + _edge_products_clips(lo, L, d) - _edge_products_clips(hi, L, d)   # [..., L-d, C, C]
        for l1 in range(L - d):
            r, c = l1 * rows, (l1 + d) * rows
            G[..., r:r + rows, c:c + rows] = blocks[..., l1, :, :]
            if d:
                G[..., c:c + rows, r:r + rows] = blocks[..., l1, :, :].transpose(-1, -2)
    zero = torch.zeros(lead + (rows, 1), dtype=torch.int64, device=dev)
    before = torch.cat([zero, torch.cumsum(torch.flip(lo, [-1]), -1)], -1)   # [..., C, l]: the sum over [t0-l, t0)
    after = torch.cat([zero, torch.cumsum(torch.flip(hi, [-1]), -1)], -1)
    sx = (s0.unsqueeze(-2) + before.transpose(-1, -2) - after.transpose(-1, -2)).reshape(lead + (F,)).contiguous()
    return G, sx


def _box_edge(x, e, L, w, q):
    """int64 [C, L-1]: the box sums B[:, u] = sum over j < w of xq[:, u-j] of the columns u in [e-(L-1), e), by cumsum on
    the L+w-2 columns before e; e >= L-1 + w-1"""
    seg = torch.clamp(x[:, e - (L - 1) - (w - 1):e], max=q).long()
    zero = torch.zeros((seg.shape[0], 1), dtype=torch.int64, device=x.device)
    cs = torch.cat([zero, torch.cumsum(seg, 1)], 1)                # cs[:, i]: the sum of the first i columns
    return cs[:, w:] - cs[:, :L - 1]


def _pure_stats(x, rows, y, K, L, g, q, w, t0, t1, max_bytes, scratch_xty):
    """-> (gram, sum_x, xty) of the design rows [t0, t1) behind the warm-up (t0 >= L-1 + w-1), whose features are the
    box sums B[c][t-l]: _range_stats with B = lo + 256 hi in the place of the counts"""
    base, s0, xty = _pure_parts(x, rows, y, K, L, g, q, w, t0, t1, max_bytes, scratch_xty)
    G, sx = _assemble(base, s0, _box_edge(x, t0, L, w, q), _box_edge(x, t1, L, w, q), L, rows)
    return G, sx, xty


def _pure_parts(x, rows, y, K, L, g, q, w, t0, t1, max_bytes, scratch_xty):
    """_range_parts for the box sums -> (base, s0, xty [L*C, K]).  Per column batch one mhs_box
    writes the planes [C, nb + L-1]; the Gram matrix is G(lo,lo) + 256 (G(lo,hi) + G(hi,lo)) + 65536 G(hi,hi), 4L - 1
    calls of mhi_gram (L where one plane is enough), and mhw_xty runs once per plane."""
    from . import _wiener, smooth
    from .gram import batches, enqueue
    dev, n, F = x.device, t1 - t0, L * rows
    two = w * q > 255
    P = 2 if two else 1
    plan = batches(n, rows, max_bytes)
    lo, hi = smooth.planes(rows, plan[0][1] + L - 1, two, dev)
    acc = torch.zeros((4 if two else 1, L, rows, rows), dtype=torch.int64, device=dev)   # (lo,lo), (hi,hi), (lo,hi), (hi,lo)
    s = torch.zeros((P, rows), dtype=torch.int64, device=dev)
    xt = torch.zeros((P, L, rows, K), dtype=torch.float64, device=dev)
    for b0, nb in plan:
        m = nb + L - 1
        pl, ph = lo[:, :m], (hi[:, :m] if two else None)
        smooth.enqueue(x, rows, m, w, q, pl, ph, t0 + b0 - (L - 1) - (w - 1))
        for d in range(L):
            if d == 0:
                enqueue(pl, rows, nb, None, 0, acc[0, 0], s[0], None, True, L - 1)
                if two:
                    enqueue(ph, rows, nb, None, 0, acc[1, 0], s[1], None, True, L - 1)
                    enqueue(pl, rows, nb, ph, rows, acc[2, 0], None, None, True, L - 1, L - 1)
            else:
                enqueue(pl, rows, nb, pl, rows, acc[0, d], None, None, True, L - 1, L - 1 - d)
                if two:
                    enqueue(ph, rows, nb, ph, rows, acc[1, d], None, None, True, L - 1, L - 1 - d)
                    enqueue(pl, rows, nb, ph, rows, acc[2, d], None, None, True, L - 1, L - 1 - d)
                    enqueue(ph, rows, nb, pl, rows, acc[3, d], None, None, True, L - 1, L - 1 - d)
        for i, pv in enumerate((pl, ph)[:P]):
            _wiener.xty(pv.data_ptr(), pv.stride(0) if rows > 1 else m, rows, nb, L, 255, y.data_ptr() + 4 * (t0 + b0 + g),
                        4 * y.stride(0) if K > 1 else 4 * nb, K, xt[i], scratch_xty, True)
    if two:
        acc[3, 0] = acc[2, 0].t()                                  # G(hi,lo) at d = 0 is the transpose of G(lo,hi)
        base = acc[0] + 256 * (acc[2] + acc[3]) + 65536 * acc[1]
        s0, xty = s[0] + 256 * s[1], xt[0] + 256.0 * xt[1]
    else:
        base, s0, xty = acc[0], s[0], xt[0]
    return base, s0, xty.reshape(F, K)


def _warm_stats(x, y, L, g, q, a, b):
    """-> (gram, sum_x, xty) of the warm-up rows [a, b), all before L-1 + w-1, built explicitly: the reference pads its
    design matrix with zeros in front of the first row, so feature (l, c) of row L-1 + r is the sum of the r + 1 design
    entries xq[c][L-1-l .. L-1-l+r].  The Gram matrix is a float64 product: its entries stay below 255 * 65280^2 < 2^53,
    so it is exact (there is no int64 matmul on the device)."""
    r0, r1 = a - (L - 1), b - (L - 1)
    xs = torch.clamp(x[:, :L - 1 + r1], max=q).long()
    X = torch.cat([torch.cumsum(xs[:, L - 1 - l:L - 1 - l + r1], 1)[:, r0:].t() for l in range(L)], 1)   # [b-a, L*C]
    Xd = X.double()
    return (Xd.t() @ Xd).long(), X.sum(0), Xd.t() @ y[:, a + g:b + g].double().t()


def _range_stats_window(x, rows, y, K, L, g, q, w, t0, t1, max_bytes, scratch_xty):
    dev, F = x.device, L * rows
    yr = y[:, t0 + g:t1 + g].double()
    sum_y, sum_yy = yr.sum(1), yr @ yr.t()
    end = L - 1 + w - 1                                             # the first row whose window is whole
    parts = []
    if t0 < min(t1, end):
        parts.append(_warm_stats(x, y, L, g, q, t0, min(t1, end)))
    if t1 > max(t0, end):
        parts.append(_pure_stats(x, rows, y, K, L, g, q, w, max(t0, end), t1, max_bytes, scratch_xty))
    if not parts:                                                   # an empty range
        parts.append((torch.zeros((F, F), dtype=torch.int64, device=dev), torch.zeros((F,), dtype=torch.int64, device=dev),
                      torch.zeros((F, K), dtype=torch.float64, device=dev)))
    G, sx, xty = parts[0]
    for pg, ps, px in parts[1:]:
        G, sx, xty = G + pg, sx + ps, xty + px
    return Stats(t1 - t0, sx, G, xty, sum_y, sum_yy, L, g, q, rows, w)


def stats(x, y, lags, lead=0, clip=None, ranges=None, max_bytes=MAX_BYTES, window=1):
    """The sufficient statistics of a Wiener filter -> [Stats], one per range of design rows (default: the single range
    of all of them).  x: counts, a 2-D uint8 device tensor with unit stride along its last axis or a ChannelSet of
    equal-length channels; y: float32 device tensor [K, bins] (or [bins]) of as many bins; lags 1..32; lead >= 0 bins by
    which the counts precede the covariates; clip: None or 1..255, counts enter as min(x, clip).  The integers are exact
    (mhi_gram), xty is float64 and deterministic (mhw_xty).  With a clip the count products go through a clamped scratch
    copy in column batches of at most max_bytes.

    window > 1 (at most 256, window * clip <= 65535) is the study's moving average over the lag-stacked, clipped design
    matrix, kept as integer sums: feature l*C + c of design row t is the sum over j = 0..min(window-1, t-(L-1)) of
    min(x[c][t-l-j], clip).  Zeros stand in front of the first design row, as in the reference, so the first window - 1
    rows (the warm-up) hold partial sums; they are built explicitly.  From row L-1 + window-1 on the features are box
    sums, which mhs_box writes as two byte planes per column batch for mhi_gram and mhw_xty (smooth.py)."""
    x, rows, cols = _matrix(x, "wiener.stats")
    y, K = _covariates(y, x, cols)
    L, g = _settings(lags, lead, rows, cols)
    q = _clip(clip)
    w = int(window)
    if w != 1:
        from .smooth import _window
        w = _window(w, q)
    rs = _ranges(ranges, L, g, cols)
    from . import _wiener
    longest = max(b - a for a, b in rs)
    scratch = torch.empty((max(_wiener.xty_scratch_bytes(rows, max(longest, 1), L, K), 8),), dtype=torch.uint8, device=x.device)
    if w == 1:
        return [_range_stats(x, rows, y, K, L, g, q, a, b, max_bytes, scratch) for a, b in rs]
    return [_range_stats_window(x, rows, y, K, L, g, q, w, a, b, max_bytes, scratch) for a, b in rs]


def _clip_list(clips):
    qs = [_clip(q) for q in clips]
    if not qs or any(b <= a for a, b in zip(qs, qs[1:])):
        raise ValueError("clips: at least one, strictly ascending")
    return qs


def _clip_groups(qs, R, L, rows, max_bytes):
    """the clips in groups whose int64 block [R, n, L, C, C] stays within max_bytes (at least one clip), and within what
    one call takes"""
    from ._sweep import MAX_CLIPS
    per = max(R, 1) * L * rows * rows * 8
    n = min(max(int(max_bytes) // per, 1), MAX_CLIPS)
    return [qs[i:i + n] for i in range(0, len(qs), n)]


def iter_stats_clips(x, y, lags, lead=0, clips=range(2, 40), ranges=None, max_bytes=MAX_BYTES):
    """stats() for every clip of a list in one pass -> an iterator of (clip, [Stats per range]) in clip order; every
    Stats is what stats(x, y, lags, lead, clip=q, ranges=ranges) returns -- gram and sum_x the same integers, xty the
    same bits.  clips: 1..255, strictly ascending (default: the study's S = 2..39); ranges: ascending and disjoint.

    The clips are taken in groups whose count products, an int64 block [ranges, clips, lags, C, C], stay within
    max_bytes (at least one clip a group); the Gram matrices assembled from it are `lags` times that and live until
    the next group is asked for.  Per group ONE mhq_gram_clips gives the count products of every (range, clip, lag
    difference) and ONE mhq_xty_clips the products with the covariates (muahuff_sweep.h): the counts are clamped in
    registers, no clamped copy is written.  The edge terms and the assembly run batched over (range, clip).  There is
    no window here: see cascade.sweep_clips."""
    from . import _sweep
    x, rows, cols = _matrix(x, "wiener.iter_stats_clips")
    y, K = _covariates(y, x, cols)
    L, g = _settings(lags, lead, rows, cols)
    qs = _clip_list(clips)
    rs = _ranges(ranges, L, g, cols)
    if any(b[0] < a[1] for a, b in zip(rs, rs[1:])):
        raise ValueError("the ranges are ascending and disjoint")
    groups = _clip_groups(qs, len(rs), L, rows, max_bytes)

    def walk():
        R, F = len(rs), L * rows
        ysum = []
        for t0, t1 in rs:                                           # as _range_stats: the same operations, the same bits
            yr = y[:, t0 + g:t1 + g].double()
            ysum.append((yr.sum(1), yr @ yr.t()))
        nmax = len(groups[0])
        scratch = torch.empty((max(_sweep.xty_clips_scratch_bytes(rows, cols, L, K, min(R, _sweep.MAX_RANGES), nmax), 8),),
                              dtype=torch.uint8, device=x.device)
        ys = 4 * y.stride(0) if K > 1 else 4 * cols
        for part in groups:
            G, sx, xt = _clips_group(x, rows, cols, y.data_ptr(), ys, K, L, g, rs, part, scratch)
            for i, q in enumerate(part):
                yield q, [Stats(t1 - t0, sx[r, i], G[r, i], xt[r, i].reshape(F, K), ysum[r][0], ysum[r][1], L, g, q, rows)
                          for r, (t0, t1) in enumerate(rs)]

    return walk()


def _clips_group(x, rows, cols, y_ptr, ys, K, L, g, rs, part, scratch):
    """One group of clips over the ranges rs of the checked matrix x: one mhq_gram_clips and one mhq_xty_clips per 16
    ranges, the edge terms and the assembly batched over (range, clip) -> (gram [R, n, L*C, L*C], sum_x [R, n, L*C], xty
    [R, n, L, C, K]).  y_ptr: the address of the covariate of column 0, rows ys bytes apart."""
    xlo = torch.stack([x[:, t0 - (L - 1):t0] for t0, _t1 in rs]).long()      # [R, C, L-1]: the columns before t0
    xhi = torch.stack([x[:, t1 - (L - 1):t1] for _t0, t1 in rs]).long()
    base, s0, xt = _clips_parts(x, rows, cols, y_ptr, ys, K, L, g, rs, part, scratch)
    G, sx = _assemble_group(base, s0, xlo, xhi, part, L, rows)
    return G, sx, xt


def _assemble_group(base, s0, xlo, xhi, part, L, rows):
    """_assemble_clips for the clips `part`, clamping the raw edge columns xlo, xhi [R, C, L-1] per clip"""
    qt = torch.tensor(part, dtype=torch.int64, device=base.device).reshape(1, len(part), 1, 1)
    return _assemble_clips(base, s0, torch.minimum(xlo.unsqueeze(1), qt), torch.minimum(xhi.unsqueeze(1), qt), L, rows)


def _clips_parts(x, rows, cols, y_ptr, ys, K, L, g, rs, part, scratch):
    """_clips_group before the edges -> (base [R, n, L, C, C], s0 [R, n, C], xty [R, n, L, C, K]): what adds over
    adjoining ranges"""
    from . import _sweep
    dev, R, n = x.device, len(rs), len(part)
    xs = x.stride(0) if rows > 1 else cols
    base = torch.zeros((R, n, L, rows, rows), dtype=torch.int64, device=dev)
    s0 = torch.zeros((R, n, rows), dtype=torch.int64, device=dev)
    xt = torch.empty((R, n, L, rows, K), dtype=torch.float64, device=dev)
    for r0 in range(0, R, _sweep.MAX_RANGES):
        sub = rs[r0:r0 + _sweep.MAX_RANGES]
        m = len(sub)
        _sweep.gram_clips(x.data_ptr(), xs, rows, cols, sub, part, L, base[r0:r0 + m], s0[r0:r0 + m])
        _sweep.xty_clips(x.data_ptr(), xs, rows, cols, sub, part, L, g, y_ptr, ys, K, xt[r0:r0 + m], scratch)
    return base, s0, xt


def stats_clips(x, y, lags, lead=0, clips=range(2, 40), ranges=None, max_bytes=MAX_BYTES):
    """iter_stats_clips as a list [(clip, [Stats per range])], for shapes where the statistics of all clips fit at once"""
    return list(iter_stats_clips(x, y, lags, lead, clips, ranges, max_bytes))


def fold_ranges(n, num_fold, first=0):
    """The contiguous folds of n rows: floor(n / num_fold) rows each, what is left over at the end belongs to none.
    -> [(t0, t1)], shifted by `first`"""
    n, num_fold = int(n), int(num_fold)
    if num_fold < 2 or n < num_fold:
        raise ValueError("%d rows do not make %d folds (at least 2, at most one per row)" % (n, num_fold))
    per = n // num_fold
    return [(first + i * per, first + (i + 1) * per) for i in range(num_fold)]


def folds(n_rows_or_x, num_fold, lags=1, lead=0):
    """Contiguous cross-validation splits as ranges of design rows -> [(train, valid, test)] for i in range(num_fold):
    valid is fold i, test the fold i + 1 (cyclically), train the list of the other folds' ranges.  n_rows_or_x: a number
    of rows (the ranges then start at 0) or the counts (the ranges are over the design rows [lags-1, bins-lead))."""
    if isinstance(n_rows_or_x, (int, np.integer)):
        n, first = int(n_rows_or_x), 0
    else:
        _x, _rows, cols = _matrix(n_rows_or_x, "wiener.folds")
        n, first = cols - int(lead) - (int(lags) - 1), int(lags) - 1
    fr = fold_ranges(n, num_fold, first)
    out = []
    for i in range(num_fold):
        v, t = i, (i + 1) % num_fold
        out.append(([fr[k] for k in range(num_fold) if k not in (v, t)], fr[v], fr[t]))
    return out


class WienerFilter:
    """Ridge regression onto the z-scored lagged counts, from Stats alone.  After fit(): weights float64 [K, L, C] and
    bias float64 [K], which apply to raw clipped counts: estimate of y[k][t + lead] = bias[k] + sum over l, c of
    weights[k][l][c] * min(x[c][t - l], clip).  Fitted on Stats with a window, the weights apply to the box SUMS of
    stats(window=) -- not to the study's means, which are the sums over the window: z-scoring makes the fit the same and
    the weights differ by that factor."""

    def __init__(self, alpha=0.0):
        if alpha < 0:
            raise ValueError("alpha is not negative")
        self.alpha = float(alpha)
        self.weights = self.bias = None
        self.lags = self.lead = self.clip = self.channels = None
        self.window = 1                                                           # until fit() reads the Stats' own

    def fit(self, stats):  # noqa: A002
        s = stats[0] if isinstance(stats, (list, tuple)) and len(stats) == 1 else stats
        if not isinstance(s, Stats) or s.n < 1:
            raise ValueError("fit takes the Stats of at least one design row")
        n = float(s.n)
        G, sx = s.gram.double(), s.sum_x.double()
        mean = sx / n
        # the variance times n^2, an integer: exactly zero for a constant feature wherever int64 holds it
        diag = torch.diagonal(s.gram)
        top = s.window * s.clip                                                   # the largest value of a feature
        if s.n * top * top * s.n < 2 ** 63:
            keep = (s.n * diag - s.sum_x * s.sum_x) > 0
        else:
            num = n * diag.double() - sx * sx
            keep = num > 2.0 ** -40 * n * diag.double()
        idx = torch.nonzero(keep).flatten()
        if idx.numel() == 0:
            raise ValueError("every feature is constant: nothing to fit")
        m = mean[idx]
        std = torch.sqrt(torch.diagonal(G)[idx] / n - m * m)                       # ddof = 0
        ybar = s.sum_y / n
        ztz = (G[idx][:, idx] - n * m.unsqueeze(1) * m.unsqueeze(0)) / (std.unsqueeze(1) * std.unsqueeze(0))
        zty = (s.xty[idx] - m.unsqueeze(1) * s.sum_y.unsqueeze(0)) / std.unsqueeze(1)
        a = ztz + self.alpha * torch.eye(idx.numel(), dtype=torch.float64, device=G.device)
        chol, info = torch.linalg.cholesky_ex(a)
        # not positive definite, or only by rounding: a pivot at the level of the factorisation's own error
        floor = 64 * 2.0 ** -52 * idx.numel() * float(torch.diagonal(a).max())
        if int(info) != 0 or float((torch.diagonal(chol) ** 2).min()) <= floor:
            raise ValueError("the normal equations are not positive definite (collinear features or too few rows): "
                             "use alpha > 0")
        wz = torch.cholesky_solve(zty, chol)                                      # [kept, K]
        w = torch.zeros((s.gram.shape[0], s.xty.shape[1]), dtype=torch.float64, device=G.device)
        w[idx] = wz / std.unsqueeze(1)
        self.bias = ybar - (w * mean.unsqueeze(1)).sum(0)
        self.weights = w.t().reshape(s.xty.shape[1], s.lags, s.channels).contiguous()
        self.lags, self.lead, self.clip, self.channels, self.window = s.lags, s.lead, s.clip, s.channels, s.window
        return self

    def predict(self, x):
        """-> float32 [K, T - L + 1]: column i is design row L-1 + i, the estimate of y[:, i + L-1 + lead].  With a window the
        box and the filter commute: mhw_fir with a zero bias on the raw counts, then mhs_box_f32 with the real bias sums
        the last `window` columns of that -- fewer in front, where the reference's zero padding stands."""
        from . import _wiener
        if self.weights is None:
            raise ValueError("predict comes after fit")
        x, rows, cols = _matrix(x, "WienerFilter.predict")
        if rows != self.channels:
            raise ValueError("the filter was fitted on %d channels, not %d" % (self.channels, rows))
        if cols < self.lags:
            raise ValueError("%d bins are fewer than the %d lags" % (cols, self.lags))
        K, n = int(self.weights.shape[0]), cols - self.lags + 1
        w = self.weights.to(device=x.device, dtype=torch.float32).contiguous()
        b = self.bias.to(device=x.device, dtype=torch.float32).contiguous()
        out = torch.empty((K, n), dtype=torch.float32, device=x.device)
        if self.window > 1:
            from . import _smooth
            raw = torch.empty((K, n), dtype=torch.float32, device=x.device)
            _wiener.fir(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, n, self.lags, self.clip, w, torch.zeros_like(b), K, raw)
            _smooth.box_f32(raw, self.window, b, out)
            return out
        _wiener.fir(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, n, self.lags, self.clip, w, b, K, out)
        return out

    def score(self, x, y):
        """-> (rmse [K], cc [K]), float64: the root mean squared error and Pearson's r of the prediction against y over
        the columns where the target exists"""
        return self._score(self.predict(x), y)

    def predict_from(self, src):
        """predict on the bins of a gram.BinSource (archive.Reader.bins, container_io.bins), without holding them ->
        float32 [K, n - L + 1]: one mhw_fir per batch into its columns of the result, the batch keeping the L-1 bins in
        front of it; with a window one mhs_box_f32 over the whole raw result, as predict orders the two."""
        return predict_many_from(src, [self])[0]

    def score_from(self, src, y):
        """score on the result of predict_from"""
        return self._score(self.predict_from(src), y)

    def _score(self, pred, y):
        if y.dim() == 1:
            y = y.unsqueeze(0)
        n = pred.shape[1] - self.lead
        if n < 1 or y.shape[0] != pred.shape[0] or y.shape[1] != pred.shape[1] + self.lags - 1:
            raise ValueError("counts and covariates do not match, or no target lies inside them")
        p = pred[:, :n].double()
        t = y[:, self.lags - 1 + self.lead:].to(p.device).double()
        rmse = torch.sqrt(((p - t) ** 2).mean(1))
        pc, tc = p - p.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
        cc = (pc * tc).sum(1) / torch.sqrt((pc * pc).sum(1) * (tc * tc).sum(1))
        return rmse, cc


# ---- the file routes: the same statistics and predictions from a gram.BinSource, batch by batch -----------------------
def _source(src, who):
    from .gram import BinSource
    if not isinstance(src, BinSource):
        raise ValueError("%s takes a gram.BinSource (archive.Reader.bins, container_io.bins, BinSource.of)" % who)
    if src.rows < 1 or src.n < 1:
        raise ValueError("at least one channel and one bin")
    return src.rows, src.n


def _source_covariates(y, src):
    """_covariates against a source, which has what it reads of the counts: the device and the number of bins"""
    return _covariates(y, src, src.n)


def _zero_stats(rows, K, L, g, q, w, dev):
    F = L * rows
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    return Stats(0, torch.zeros((F,), dtype=torch.int64, device=dev), torch.zeros((F, F), dtype=torch.int64, device=dev),
                 z(F, K), z(K), z(K, K), L, g, q, rows, w)


def _batch_cols(src, cols):
    """the most bins a batch of the source's walks brings of its own"""
    return min(cols, max(src.max_bytes // max(src.rows, 1), 1))


def stats_from(src, y, lags, lead=0, clip=None, ranges=None, window=1):
    """stats() on the bins of a gram.BinSource, without holding them -> [Stats], one per range.  y: float32 [K, src.n] on
    the source's device, on its bin grid; ranges: design rows in the source's bins, as in stats.  The source is walked
    once (gram.walk_ranges: the bins no range needs are not read) with a halo of lags-1 + window-1 bins, and per batch
    the kernels of stats() run on the scratch for what every range has in the batch.  What adds over the pieces of a
    range is added as it comes -- the count products per lag difference [lags, C, C], the row sums, xty --; the edge
    terms of adjoining pieces cancel, so the [lags*C, lags*C] matrix is assembled once per range, from the columns in
    front of its first and of its last row, kept when their batch was resident.  The warm-up rows of window > 1 are
    relative to the source's first bin: a batch behind the first has its halo in front of every row.  gram, sum_x and n
    are the integers of stats(read(...), y, ...); xty, sum_y and sum_yy are float64 sums taken batch by batch, in
    another order.  Next to the walk's scratch a clip or a window takes a clamped copy or the box planes of a batch: up
    to three times max_bytes in all."""
    from .gram import walk_ranges
    rows, cols = _source(src, "wiener.stats_from")
    y, K = _source_covariates(y, src)
    L, g = _settings(lags, lead, rows, cols)
    q = _clip(clip)
    w = int(window)
    if w != 1:
        from .smooth import _window
        w = _window(w, q)
    rs = _ranges(ranges, L, g, cols)
    from . import _wiener
    scratch = torch.empty((max(_wiener.xty_scratch_bytes(rows, _batch_cols(src, cols), L, K), 8),), dtype=torch.uint8, device=y.device)
    dev, F, halo = y.device, L * rows, L - 1 + w - 1
    # per range: [base, s0, xty, lo, hi] of its rows behind the warm-up, (gram, sum_x, xty) of those in it, sum_y, sum_yy
    pure, warm = [None] * len(rs), [None] * len(rs)
    sy = [torch.zeros((K,), dtype=torch.float64, device=dev) for _ in rs]
    syy = [torch.zeros((K, K), dtype=torch.float64, device=dev) for _ in rs]
    for b0, _nb, h, view, pieces in walk_ranges(src, halo, rs):
        o = b0 - h                                                  # the view's first bin
        yv = y[:, o:]
        for i, a, b in pieces:
            a0, b0_ = a - o, b - o                                  # the piece in the view's columns
            yr = yv[:, a0 + g:b0_ + g].double()
            sy[i] += yr.sum(1)
            syy[i] += yr @ yr.t()
            if w > 1 and a0 < halo:                                 # warm-up rows: the view starts at the source's first bin
                part = _warm_stats(view, yv, L, g, q, a0, min(b0_, halo))
                warm[i] = part if warm[i] is None else tuple(u + v for u, v in zip(warm[i], part))
                a0 = min(b0_, halo)
            if a0 == b0_:
                continue
            if w == 1:
                xty = torch.zeros((F, K), dtype=torch.float64, device=dev)
                base, s0 = _range_parts(view, rows, yv, K, L, g, q, a0, b0_, src.max_bytes, scratch, xty)
                edge = lambda e: torch.clamp(view[:, e - (L - 1):e], max=q).long()  # noqa: E731
            else:
                base, s0, xty = _pure_parts(view, rows, yv, K, L, g, q, w, a0, b0_, src.max_bytes, scratch)
                edge = lambda e: _box_edge(view, e, L, w, q)  # noqa: E731
            if pure[i] is None:
                pure[i] = [base, s0, xty, edge(a0), None]
            else:
                for k, t in enumerate((base, s0, xty)):
                    pure[i][k] += t
            if b == rs[i][1]:
                pure[i][4] = edge(b0_)
    out = []
    for i, (t0, t1) in enumerate(rs):
        if pure[i] is None and warm[i] is None:                     # an empty range
            out.append(_zero_stats(rows, K, L, g, q, w, dev))
            continue
        if pure[i] is None:
            G, sx, xty = warm[i]
        else:
            G, sx = _assemble(pure[i][0], pure[i][1], pure[i][3], pure[i][4], L, rows)
            xty = pure[i][2]
            if warm[i] is not None:                                 # in place: no third matrix next to the two
                G += warm[i][0]
                sx += warm[i][1]
                xty += warm[i][2]
        pure[i] = warm[i] = None
        out.append(Stats(t1 - t0, sx, G, xty, sy[i], syy[i], L, g, q, rows, w))
    return out


def stats_clips_from(src, y, lags, lead=0, clips=range(2, 40), ranges=None):
    """stats_clips() on the bins of a gram.BinSource -> [(clip, [Stats per range])], every Stats what stats_from(src, y,
    lags, lead, clip=q, ranges=ranges) returns: the same integers, xty summed batch by batch.  One walk with a halo of
    lags-1 bins; per batch and group of clips (the groups of iter_stats_clips, for what the ranges have in the batch) one
    mhq_gram_clips and one mhq_xty_clips, added into the count products [ranges, clips, lags, C, C] of the walk; the
    matrices are assembled once at its end, from every range's own edge columns.  The statistics of ALL clips are
    returned together, ranges * clips * (lags*C)^2 * 8 bytes: cut a long list of clips where that is too much."""
    from . import _sweep
    from .gram import walk_ranges
    rows, cols = _source(src, "wiener.stats_clips_from")
    y, K = _source_covariates(y, src)
    L, g = _settings(lags, lead, rows, cols)
    qs = _clip_list(clips)
    rs = _ranges(ranges, L, g, cols)
    if any(b[0] < a[1] for a, b in zip(rs, rs[1:])):
        raise ValueError("the ranges are ascending and disjoint")
    dev, R, F = y.device, len(rs), L * rows
    groups = _clip_groups(qs, R, L, rows, src.max_bytes)
    base = torch.zeros((R, len(qs), L, rows, rows), dtype=torch.int64, device=dev)
    s0 = torch.zeros((R, len(qs), rows), dtype=torch.int64, device=dev)
    xt = torch.zeros((R, len(qs), L, rows, K), dtype=torch.float64, device=dev)
    xlo = torch.zeros((R, rows, L - 1), dtype=torch.int64, device=dev)           # the raw columns in front of a range's first
    xhi = torch.zeros((R, rows, L - 1), dtype=torch.int64, device=dev)           # and of its last row, kept as they pass
    sy = torch.zeros((R, K), dtype=torch.float64, device=dev)
    syy = torch.zeros((R, K, K), dtype=torch.float64, device=dev)
    scratch = None
    ys = 4 * y.stride(0) if K > 1 else 4 * cols
    for b0, _nb, h, view, pieces in walk_ranges(src, L - 1, rs):
        o, width = b0 - h, int(view.shape[1])
        idx = torch.tensor([i for i, _a, _b in pieces], dtype=torch.int64, device=dev)
        local = [(a - o, b - o) for _i, a, b in pieces]
        for i, a, b in pieces:
            yr = y[:, a + g:b + g].double()
            sy[i] += yr.sum(1)
            syy[i] += yr @ yr.t()
            if a == rs[i][0]:
                xlo[i] = view[:, a - o - (L - 1):a - o]
            if b == rs[i][1]:
                xhi[i] = view[:, b - o - (L - 1):b - o]
        need =max(_sweep.xty_clips_scratch_bytes(rows, width, L, K, min(len(local), _sweep.MAX_RANGES), len(groups[0])), 8)
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
        c0 = 0
        for part in groups:                                         # the lead is in the address: column t meets y[t + g]
            pb, ps, px = _clips_parts(view, rows, width, y.data_ptr() + 4 * (o + g), ys, K, L, 0, local, part, scratch)
            base[idx, c0:c0 + len(part)] += pb
            s0[idx, c0:c0 + len(part)] += ps
            xt[idx, c0:c0 + len(part)] += px
            c0 += len(part)
    out, c0 = [], 0
    for part in groups:                                             # assembled once per range and clip, from the range's own edges
        G, sx = _assemble_group(base[:, c0:c0 + len(part)], s0[:, c0:c0 + len(part)], xlo, xhi, part, L, rows)
        for i, q in enumerate(part):
            out.append((q, [Stats(t1 - t0, sx[r, i], G[r, i], xt[r, c0 + i].reshape(F, K), sy[r], syy[r], L, g, q, rows)
                            for r, (t0, t1) in enumerate(rs)]))
        c0 += len(part)
    return out


def _fitted(src, filters, who):
    rows, cols = _source(src, who)
    for f in filters:
        if not isinstance(f, WienerFilter) or f.weights is None:
            raise ValueError("predict comes after fit")
        if rows != f.channels:
            raise ValueError("the filter was fitted on %d channels, not %d" % (f.channels, rows))
        if cols < f.lags:
            raise ValueError("%d bins are fewer than the %d lags" % (cols, f.lags))
    return rows, cols


def iter_predict_from(src, filters):
    """predict_many_from as a generator, one prediction at a time in the order of `filters`: what a group's pass made is
    handed out before the next group's pass begins."""
    from . import _wiener
    from .gram import walk
    filters = list(filters)
    rows, cols = _fitted(src, filters, "wiener.predict_many_from")
    dev = src.device
    size = lambda f: 4 * int(f.weights.shape[0]) * (cols - f.lags + 1) * (2 if f.window > 1 else 1)  # noqa: E731
    groups, room = [], 0
    for f in filters:
        if groups and room + size(f) <= src.max_bytes:
            groups[-1].append(f)
            room += size(f)
        else:
            groups.append([f])
            room = size(f)
    for group in groups:
        jobs = []
        for f in group:
            K, L = int(f.weights.shape[0]), f.lags
            w = f.weights.to(device=dev, dtype=torch.float32).contiguous()
            b = f.bias.to(device=dev, dtype=torch.float32).contiguous()
            raw = torch.empty((K, cols - L + 1), dtype=torch.float32, device=dev)
            jobs.append((f, K, L, w, b, torch.zeros_like(b) if f.window > 1 else b, raw))
        for b0, nb, h, view in walk(src, max(f.lags for f in group) - 1):
            o, pitch = b0 - h, (view.stride(0) if rows > 1 else int(view.shape[1]))
            for f, K, L, w, _b, b_fir, raw in jobs:
                first = max(b0, L - 1)                              # the first design row of this batch
                m = b0 + nb - first
                if m > 0:
                    _wiener.fir(view.data_ptr() + first - o - (L - 1), pitch, rows, m, L, f.clip, w, b_fir, K,
                                raw[:, first - (L - 1):first - (L - 1) + m])
        while jobs:
            f, K, L, w, b, _b_fir, raw = jobs.pop(0)
            if f.window > 1:
                from . import _smooth
                out = torch.empty_like(raw)
                _smooth.box_f32(raw, f.window, b, out)
                raw = out
            yield raw


def predict_many_from(src, filters):
    """WienerFilter.predict_from for several fitted filters -> [float32 [K, n - L + 1]] in their order: every batch of
    the source meets, while it is resident, one mhw_fir per filter.  One pass over the source per group of filters whose
    results (twice that with a window) fit the source's max_bytes; at least one filter a pass."""
    return list(iter_predict_from(src, filters))
