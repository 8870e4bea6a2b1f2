"""Spike-count covariance: the channel-by-channel Gram matrix sum_t x_i[t] * y_j[t] of uint8 counts, exact in int64, in
one call on the int8 matrix cores (mhi_gram, include/muahuff_ingest.h), with the row sums from the same pass -- what the
covariance and correlation matrices, PCA, factor analysis and the normal equations of a linear decoder start from; at
one lag, the all-pairs cross-correlogram.

gram works on matrices that are resident on the device.  read_gram is what the readers (archive.Reader.read_gram,
container_io.decompress_gram) share: it walks a range in batches of whole bins, decodes each batch into one reused
scratch matrix and adds its products to the result.  There is no CPU path: host matrices are refused."""
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
