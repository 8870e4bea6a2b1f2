"""Spike-count covariance: the channel-by-channel Gram matrix sum_t x_i[t] * y_j[t] of uint8 counts, exact in int64, in
one call on the int8 matrix cores (mhi_gram, include/muahuff_ingest.h), with the row sums from the same pass -- what the
covariance and correlation matrices, PCA, factor analysis and the normal equations of a linear decoder start from; at
one lag, the all-pairs cross-correlogram.

gram works on matrices that are resident on the device.  read_gram is what the readers (archive.Reader.read_gram,
container_io.decompress_gram) share: it walks a range in batches of whole bins, decodes each batch into one reused
scratch matrix and adds its products to the result.  BinSource, halo_plan and walk are what every decoder's file route
(source_gram here, wiener.stats_from, WienerFilter.predict_from, ...) stands on: batches of whole bins that keep a halo of
the bins in front of them, carried on the device from one batch to the next.  There is no CPU path: host matrices are
refused."""
import numpy as np
import torch

from .windows import MAX_BIN, MAX_BYTES, _matrix


class Gram:
    """n: the number of bins summed over (an int, or a list of them with a leading lag axis); sum_a [ra], sum_b [rb] and
    gram [ra, rb]: int64 device tensors, gram[i, j] = sum_t a_i[t] * b_j[t].  symmetric: b is a."""

    def __init__(self, n, sum_a, sum_b, gram, symmetric=False):
        self.n, self.sum_a, self.sum_b, self.gram, self.symmetric = n, sum_a, sum_b, gram, bool(symmetric)

    def _n(self, like):
        """n as a float64 device tensor that broadcasts against `like`: a tensor divisor is a true division, where a
        Python scalar would be turned into a multiplication by its reciprocal"""
        if isinstance(self.n, (list, tuple)):
            n = torch.tensor(list(self.n), dtype=torch.float64, device=like.device)
            return n.reshape((-1,) + (1,) * (like.dim() - 1))
        return torch.tensor(float(self.n), dtype=torch.float64, device=like.device)

    def mean(self):
        """-> (mean of a's rows, mean of b's rows), float64"""
        return self.sum_a.double() / self._n(self.sum_a), self.sum_b.double() / self._n(self.sum_b)

    def _centred(self, ddof):
        """(G - s_a s_b^T / n) / (n - ddof), every step one correctly rounded float64 operation"""
        n = self._n(self.gram)
        outer = self.sum_a.double().unsqueeze(-1) * self.sum_b.double().unsqueeze(-2)
        return (self.gram.double() - outer / n) / (n - ddof)

    def cov(self, ddof=1):
        """The covariance of a's rows with b's rows: (G - s_a s_b^T / n) / (n - ddof), float64 [ra, rb].  The integers
        are exact; above 2^53 their conversion to float64 rounds."""
        return self._centred(ddof)

    def corr(self):
        """The correlation matrix cov / sqrt(var_i var_j), float64, of the symmetric form (the variances are its
        diagonal).  An element whose row or column has zero variance is nan."""
        if not self.symmetric:
            raise ValueError("corr needs the symmetric form: the variances are the diagonal of the matrix")
        c = self._centred(0)
        d = torch.diagonal(c, dim1=-2, dim2=-1)
        den = torch.sqrt(d.unsqueeze(-1) * d.unsqueeze(-2))
        return torch.where(den > 0, c / den, torch.full_like(c, float("nan")))

    def __add__(self, other):
        """Two results over the same channels and disjoint bins -> the result over both"""
        if not isinstance(other, Gram):
            return NotImplemented
        if self.gram.shape != other.gram.shape or self.symmetric != other.symmetric:
            raise ValueError("the two results are not over the same channels")
        if isinstance(self.n, (list, tuple)) or isinstance(other.n, (list, tuple)):
            if not (isinstance(self.n, (list, tuple)) and isinstance(other.n, (list, tuple)) and len(self.n) == len(other.n)):
                raise ValueError("the two results are not over the same lags")
            n = [x + y for x, y in zip(self.n, other.n)]
        else:
            n = self.n + other.n
        return Gram(n, self.sum_a + other.sum_a, self.sum_b + other.sum_b, self.gram + other.gram, self.symmetric)


def enqueue(x, rows, cols, y, y_rows, out, sum_a, sum_b, add, x_shift=0, y_shift=0):
    """Enqueue one mhi_gram on the current stream: the `cols` columns from x_shift on of x's rows against those from
    y_shift on of y's (y None: the symmetric form) into out (int64 [rows, y_rows], contiguous rows) and the sums (int64,
    or None), overwritten or with `add` added to."""
    from . import _ingest
    _ingest.gram(x.data_ptr() + x_shift, x.stride(0) if rows > 1 else cols, rows,
                 None if y is None else y.data_ptr() + y_shift, 0 if y is None else (y.stride(0) if y_rows > 1 else cols),
                 0 if y is None else y_rows, cols, out, sum_a, sum_b, add)


def _lags(lag):
    many = not isinstance(lag, (int, np.integer))
    lags = [int(v) for v in lag] if many else [int(lag)]
    if not lags or min(lags) < 0:
        raise ValueError("lag is an int >= 0 or a non-empty sequence of them")
    return lags, many


def gram(x, y=None, lag=0):
    """sum_t x_i[t] * y_j[t + lag] over the cols - lag bins where both exist -> Gram (int64, exact).  x, y: a 2-D uint8
    device tensor with unit stride along its last axis (any pitch or offset: what the decoders return, or a slice of
    it), or a ChannelSet of equal-length channels; both have the same number of bins.  y=None is x itself, and with
    lag=0 the symmetric form is used: only the tiles on or above the diagonal are computed.  lag: an int >= 0 below the
    number of bins, or a sequence of them: the fields of the result then carry a leading lag axis and n is a list."""
    lags, many = _lags(lag)
    x, rows, cols = _matrix(x, "gram")
    if y is None:
        yy, y_rows = x, rows
    else:
        yy, y_rows, y_cols = _matrix(y, "gram")
        if y_cols != cols:
            raise ValueError("x and y have the same number of bins (%d, %d)" % (cols, y_cols))
        if yy.device != x.device:
            raise ValueError("x and y are on the same device")
    if max(lags) >= cols:
        raise ValueError("lag %d leaves no bin of the %d" % (max(lags), cols))
    L = len(lags)
    g = torch.empty((L, rows, y_rows), dtype=torch.int64, device=x.device)
    sa = torch.empty((L, rows), dtype=torch.int64, device=x.device)
    sb = torch.empty((L, y_rows), dtype=torch.int64, device=x.device)
    sym = y is None and lags == [0]
    for k, lg in enumerate(lags):
        if y is None and lg == 0:
            enqueue(x, rows, cols, None, 0, g[k], sa[k], sb[k], False)
        else:
            enqueue(x, rows, cols - lg, yy, y_rows, g[k], sa[k], sb[k], False, 0, lg)
    n = [cols - lg for lg in lags]
    return Gram(n, sa, sb, g, False) if many else Gram(n[0], sa[0], sb[0], g[0], sym)


# ---- what the two readers share --------------------------------------------------------------------------------------
def gram_args(start, stop, bin, T):  # noqa: A002
    """The argument rules of read_gram / decompress_gram, before anything is read -> (start, r, n): n whole bins of r
    samples from start on; what lies behind the last whole bin is left out."""
    start, stop = int(start), int(stop)
    r = 1 if bin is None else int(bin)
    if not 1 <= r <= MAX_BIN:
        raise ValueError("bin factor %d outside 1..%d" % (r, MAX_BIN))
    if not 0 <= start <= stop <= T:
        raise ValueError("range [%d, %d) is not inside [0, %d)" % (start, stop, T))
    if start % r:
        raise ValueError("start %d is not a multiple of the bin factor %d" % (start, r))
    return start, r, (stop - start) // r


def batches(n, rows, max_bytes):
    """[(first bin, bins)] that cover n bins in batches of at most max_bytes / rows bins, at least one"""
    per = max(int(max_bytes) // max(rows, 1), 1)
    return [(b, min(per, n - b)) for b in range(0, n, per)]


def read_gram(read_bins, rows, n, max_bytes, device="cuda"):
    """One scratch [rows, bins of a batch], read_bins(b0, nb, view) for every batch -- it fills the uint8 view [rows, nb]
    with the bins [b0, b0 + nb) -- and one symmetric mhi_gram that adds the batch to the result.  -> Gram"""
    g = torch.zeros((rows, rows), dtype=torch.int64, device=device)
    s = torch.zeros((rows,), dtype=torch.int64, device=device)
    if rows and n:
        plan = batches(n, rows, max_bytes)
        scratch = torch.empty((rows, plan[0][1]), dtype=torch.uint8, device=device)
        for b0, nb in plan:
            view = scratch[:, :nb]
            read_bins(b0, nb, view)
            enqueue(view, rows, nb, None, 0, g, s, None, True)
    return Gram(n, s, s.clone(), g, True)


# ---- decoders from a file: one source of bins, one walker that carries a halo ------------------------------------------
def halo_plan(n, rows, halo, max_bytes):
    """[(first bin, bins)] that tile [0, n) in order, for a walk in which every batch also keeps the min(halo, first bin)
    bins in front of it: the scratch of a batch, rows * (bins + min(halo, first bin)) bytes, is at most max_bytes.  A
    budget that does not exceed the halo gives batches of one bin instead of a walk that stalls.  Pure Python."""
    n, rows, halo = int(n), max(int(rows), 1), int(halo)
    if halo < 0:
        raise ValueError("halo %d is negative" % halo)
    cap = int(max_bytes) // rows                                    # the columns of the scratch
    out, b = [], 0
    while b < n:
        nb = min(max(cap - min(halo, b), 1), n - b)
        out.append((b, nb))
        b += nb
    return out


class BinSource:
    """Where the file routes of the decoders take their counts from: rows channels of n whole bins on `device`, read in
    batches of at most max_bytes bytes.  read_bins(b0, nb, view) fills the uint8 view [rows, nb] (unit stride along its
    last axis, any pitch) with the bins [b0, b0 + nb).  archive.Reader.bins and container_io.bins make one over a file,
    BinSource.of over a matrix that is resident."""

    def __init__(self, rows, n, device, max_bytes, read_bins, close=None):
        self.rows, self.n, self.device = int(rows), int(n), torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("a source of bins lives on a device: there is no CPU path")
        if self.device.index is None:                               # "cuda" is the current device, named as a tensor's is
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_bytes = MAX_BYTES if max_bytes is None else int(max_bytes)
        self._read, self._close = read_bins, close

    def read_bins(self, b0, nb, view):
        b0, nb = int(b0), int(nb)
        if not 0 <= b0 <= b0 + nb <= self.n:
            raise ValueError("bins [%d, %d) are not inside [0, %d)" % (b0, b0 + nb, self.n))
        if view.dtype != torch.uint8 or tuple(view.shape) != (self.rows, nb):
            raise ValueError("the view is a uint8 tensor [%d, %d]" % (self.rows, nb))
        self._read(b0, nb, view)

    @classmethod
    def of(cls, x, max_bytes=None):
        """a resident matrix (what gram takes) as a source: read_bins copies its columns"""
        x, rows, cols = _matrix(x, "BinSource.of")
        return cls(rows, cols, x.device, max_bytes, lambda b0, nb, view: view.copy_(x[:, b0:b0 + nb]))

    def close(self):
        """what the source opened itself (container_io.bins on a path) is closed; anything else is left as it is"""
        if self._close is not None:
            self._close()
            self._close = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def walk(src, halo, lo=0, hi=None):
    """Walk the bins [lo, hi) of a BinSource in the batches of halo_plan -> a generator of (b0, nb, h, view): view is
    uint8 [rows, h + nb] and holds the bins [b0 - h, b0 + nb), h = min(halo, b0 - lo) of them in front of the batch's own.
    One scratch serves the call, so a view is good until the next one is asked for.  The halo is not read again: the last
    h columns of the view before move to the front on the device, in stream order -- through a temporary where the two
    overlap (nb < halo).  Nothing outside [lo, hi) is read."""
    halo, lo = int(halo), int(lo)
    hi = src.n if hi is None else int(hi)
    if not 0 <= lo <= hi <= src.n:
        raise ValueError("bins [%d, %d) are not inside [0, %d)" % (lo, hi, src.n))
    plan = halo_plan(hi - lo, src.rows, halo, src.max_bytes)
    if not plan or src.rows < 1:
        return
    width = max(nb + min(halo, b) for b, nb in plan)
    scratch = torch.empty((src.rows, width), dtype=torch.uint8, device=src.device)
    before = 0                                                      # the columns of the view before
    for b, nb in plan:
        h = min(halo, b)
        if h:
            tail = scratch[:, before - h:before]
            scratch[:, :h].copy_(tail.clone() if before - h < h else tail)
        view = scratch[:, :h + nb]
        src.read_bins(lo + b, nb, view[:, h:])
        before = h + nb
        yield lo + b, nb, h, view


def walk_ranges(src, halo, ranges):
    """walk for ranges [(a, b)] of bins, each of which needs the halo bins in front of it (fewer at the source's first
    bin): ranges that touch or lie within a halo of each other share one walk, bins between ranges further apart are
    not read.  -> a generator of (b0, nb, h, view, pieces), pieces: [(index of the range, a, b)], what the ranges have
    inside [b0, b0 + nb); batches without a piece are left out (they are read: the next halo is in them)."""
    order = sorted((i for i, (a, b) in enumerate(ranges) if b > a), key=lambda i: ranges[i][0])
    groups = []
    for i in order:
        a, b = ranges[i]
        if groups and max(a - halo, 0) <= groups[-1][1]:
            groups[-1][1] = max(groups[-1][1], b)
            groups[-1][2].append(i)
        else:
            groups.append([max(a - halo, 0), b, [i]])
    for lo, hi, members in groups:
        for b0, nb, h, view in walk(src, halo, lo, hi):
            pieces = [(i, max(ranges[i][0], b0), min(ranges[i][1], b0 + nb)) for i in members]
            pieces = [p for p in pieces if p[1] < p[2]]
            if pieces:
                yield b0, nb, h, view, pieces


def source_gram(src, lag=0):
    """gram(x, lag=lag) of the bins of a BinSource, without holding them: the halo is max(lag), and a batch adds the
    products whose LATER bin lies in it.  lag=0 is read_gram's symmetric single call per batch.  -> Gram"""
    lags, many = _lags(lag)
    if lags == [0] and not many:
        return read_gram(src.read_bins, src.rows, src.n, src.max_bytes, src.device)
    if src.rows < 1 or src.n < 1:
        raise ValueError("at least one channel and one bin")
    if max(lags) >= src.n:
        raise ValueError("lag %d leaves no bin of the %d" % (max(lags), src.n))
    rows, dev = src.rows, src.device
    g = torch.zeros((len(lags), rows, rows), dtype=torch.int64, device=dev)
    sa = torch.zeros((len(lags), rows), dtype=torch.int64, device=dev)
    sb = torch.zeros((len(lags), rows), dtype=torch.int64, device=dev)
    for b0, nb, h, view in walk(src, max(lags)):
        for k, lg in enumerate(lags):
            first = max(b0, lg)                                     # the first later bin of this batch
            m = b0 + nb - first
            if m <= 0:
                continue
            at = first - (b0 - h)
            if lg == 0:
                enqueue(view, rows, m, None, 0, g[k], sa[k], sb[k], True, at)
            else:
                enqueue(view, rows, m, view, rows, g[k], sa[k], sb[k], True, at - lg, at)
    n = [src.n - lg for lg in lags]
    return Gram(n, sa, sb, g, False) if many else Gram(n[0], sa[0], sb[0], g[0], False)
