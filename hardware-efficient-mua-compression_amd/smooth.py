"""The moving-average window of the behavioural study on the device: the sums of `window` consecutive clipped bins of
every channel (mhs_box, include/muahuff_smooth.h).

A box sum of up to 256 bins clipped at up to 255 does not fit the uint8 every other kernel reads, so box_sum returns it
as two byte planes, B = lo + 256 * hi, which needs window * clip <= 65535; where window * clip <= 255 one plane is
enough and hi is None.  The planes are what wiener.stats(window=) feeds to mhi_gram and mhw_xty.  The study clips with
X[X > S] = S, so its clip is S (not the codec's S - 1), and divides the sums by the window: moving_average does that;
the decoders keep the integer sums, since z-scoring removes the scale.  There is no CPU path: host matrices are refused."""
import torch

from .windows import _matrix


def _window(window, q):
    from ._smooth import MAX_SUM, MAX_WINDOW
    w = int(window)
    if not 1 <= w <= MAX_WINDOW:
        raise ValueError("window %d outside 1..%d" % (w, MAX_WINDOW))
    if w * q > MAX_SUM:
        raise ValueError("window * clip = %d is above %d: a box sum would not fit two byte planes" % (w * q, MAX_SUM))
    return w


def planes(rows, cols, two, device):
    """-> (lo, hi | None): uint8 [rows, cols] views with a row pitch that is a multiple of 16, as mhs_box writes them"""
    pitch = (cols + 15) // 16 * 16
    buf = torch.empty((2 if two else 1, rows, pitch), dtype=torch.uint8, device=device)
    return buf[0, :, :cols], (buf[1, :, :cols] if two else None)


def enqueue(x, rows, n, window, q, lo, hi, x_shift=0):
    """Enqueue one mhs_box on the current stream: the n box sums of x's rows from column x_shift on (n + window - 1
    columns are read) into the planes lo and hi (hi None: one plane)."""
    from . import _smooth
    _smooth.box(x.data_ptr() + x_shift, x.stride(0) if rows > 1 else n + window - 1, rows, n, window, q, lo, hi)


def box_sum(x, window, clip=None):
    """The sums of `window` consecutive bins -> (lo, hi): uint8 device tensors [channels, bins - window + 1] with
    lo[c][i] + 256 * hi[c][i] = sum over j < window of min(x[c][i + j], clip); hi is None where window * clip <= 255.  x: a
    2-D uint8 device tensor with unit stride along its last axis (any pitch or offset) or a ChannelSet of equal-length
    channels; window 1..256; clip None or 1..255 with window * clip <= 65535."""
    from .wiener import _clip
    x, rows, cols = _matrix(x, "smooth.box_sum")
    q = _clip(clip)
    w = _window(window, q)
    if cols < w:
        raise ValueError("%d bins are fewer than the window of %d" % (cols, w))
    n = cols - w + 1
    lo, hi = planes(rows, n, w * q > 255, x.device)
    enqueue(x, rows, n, w, q, lo, hi)
    return lo, hi


def moving_average(x, window, clip=None):
    """-> float32 [channels, bins - window + 1]: the mean of `window` consecutive clipped bins, (lo + 256 * hi) / window"""
    lo, hi = box_sum(x, window, clip)
    s = lo.to(torch.float32)
    if hi is not None:
        s += 256.0 * hi.to(torch.float32)
    return s / float(int(window))
