"""Trial-aligned reads: the same window around many trigger times, per channel, in one call (mhi_windows,
include/muahuff_ingest.h) -- stacked as [trials, channels, bins] or summed over the trials into a PSTH, the sum per
channel and bin with, for the variance, the sum of squares.  Each window is re-binned on its OWN grid: bin b of a window
holds its samples [b*r, b*r + r), wherever the window starts.

gather / psth work on a matrix that is resident on the device.  plan_spans is the host planner of the readers
(archive.Reader.read_windows, container_io.decompress_windows): it joins the windows into spans that are read and decoded
ONCE each, packs the spans side by side into a scratch matrix, and read_windows runs one mhi_windows per such batch.
There is no CPU path: host matrices are refused."""
from collections import namedtuple

import numpy as np
import torch

from ._lib import CHUNK

# The scratch matrix of one batch of spans holds at most this many bytes by default (rows x columns).  A memory knob, not
# a measurement: large enough that a thousand trials of a few seconds at 1 ms bins over a thousand channels are one or
# two batches, small against the device's memory.
MAX_BYTES = 1 << 30
MAX_BIN = 4096      # the readers' bin factors, as codec.query_args

Batch = namedtuple("Batch", "spans base cols first last offsets early")
Plan = namedtuple("Plan", "order batches")


def _matrix(x, who):
    if hasattr(x, "matrix") and hasattr(x, "ch_off"):
        x = x.matrix()
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise ValueError("%s takes a ChannelSet or a device tensor: there is no CPU path" % who)
    if x.dtype != torch.uint8 or x.dim() != 2:
        raise ValueError("counts are a 2-D uint8 tensor [channels, bins]")
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if rows < 1 or cols < 1:
        raise ValueError("at least one channel and one bin")
    if cols > 1 and x.stride(1) != 1:
        raise ValueError("the bins of a channel lie back to back (unit stride along the last axis)")
    if rows > 1 and x.stride(0) < cols:
        raise ValueError("the row pitch is at least the row length")
    return x, rows, cols


def _width(W, bin, top=(1 << 32) - 1):  # noqa: A002
    W, r = int(W), 1 if bin is None else int(bin)
    if not 1 <= W < 1 << 32:
        raise ValueError("window length %d outside 1..2^32 - 1" % W)
    if not 1 <= r <= top:
        raise ValueError("bin factor %d outside 1..%d" % (r, top))
    return W, r, (W + r - 1) // r


def _offsets(offsets, cols, W, device):
    """-> (int64 device tensor, whether the host has checked them)"""
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        if offsets.dtype != torch.int64 or offsets.dim() != 1:
            raise ValueError("device offsets are a 1-D int64 tensor")
        return offsets.contiguous(), False
    off = np.asarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets)
    if off.size == 0:
        off = off.astype(np.int64)
    if off.ndim != 1 or off.dtype.kind not in "iu":
        raise ValueError("offsets are a 1-D integer array")
    if off.size >= 1 << 32:
        raise ValueError("fewer than 2^32 windows")
    off = off.astype(np.int64)      # (a uint64 of 2^63 and more wraps below 0: refused as well)
    bad = np.nonzero((off < 0) | (off > cols - W))[0]
    if bad.size:
        raise ValueError("window %d: offset %d is not inside [0, %d]" % (bad[0], int(off[bad[0]]), cols - W))
    return torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(device), True


def _raise_bad(bad, off):
    n_bad, first = (int(v) for v in bad.cpu())      # synchronises
    if n_bad:
        raise ValueError("%d windows are not inside the matrix; the first is window %d (offset %d)" %
                         (n_bad, first, int(off[first])))


def stack(x, rows, cols, off, idx, W, r, out, bad):
    """Enqueue the STACK form: the windows `off` (int64 device tensor) of x's rows into out[slot] ([n_out, rows, nb],
    contiguous, uint8 saturating or int32 exact), slot = idx[k] (int64 device tensor) or k."""
    from . import _ingest
    e = out.element_size()
    nb = int(out.shape[2])
    _ingest.windows(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, off, idx, int(out.shape[0]), W, r,
                    _ingest.WIN_STACK, out.data_ptr(), 8 * e, rows * nb * e, nb * e, bad)


def accumulate(x, rows, cols, off, W, r, out, sumsq, add, bad):
    """Enqueue the SUM form: out (int32 [rows, nb]) and sumsq (None or int64 [rows, nb]), both contiguous, overwritten or
    with `add` added to."""
    from . import _ingest
    nb = int(out.shape[1])
    _ingest.windows(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, off, None, 0, W, r, _ingest.WIN_SUM,
                    out.data_ptr(), 32, 0, 4 * nb, bad, sumsq, 8 * nb, add)


def _sum_bound(n, W, r):
    if n * 255 * min(r, W) >= 1 << 31:
        raise ValueError("%d windows of bins of %d samples can exceed the int32 sums" % (n, min(r, W)))


def gather(x, offsets, W, bin=None, saturate=True):  # noqa: A002
    """The windows x[:, o:o + W] for every o of `offsets`, each summed in bins of `bin` samples from its own first sample
    (the last bin may be cut) -> device tensor [n, rows, ceil(W / bin)]: uint8 = min(sum, 255), or int32 sums with
    saturate=False.  x: a 2-D uint8 device tensor with unit stride along its last axis (any pitch or offset: what the
    decoders return, or a slice of it), or a ChannelSet of equal-length channels.  offsets: a host integer array --
    ValueError names the first one outside [0, cols - W] -- or a device int64 tensor, which the kernel checks: one
    synchronisation after the call, and the same ValueError."""
    from . import _ingest
    x, rows, cols = _matrix(x, "gather")
    W, r, nb = _width(W, bin)
    off, checked = _offsets(offsets, cols, W, x.device)
    n = int(off.numel())
    out = torch.empty((n, rows, nb), dtype=torch.uint8 if saturate else torch.int32, device=x.device)
    if n == 0:
        return out
    bad = _ingest.verify_state(x.device)
    stack(x, rows, cols, off, None, W, r, out, bad)
    if not checked:
        _raise_bad(bad, off)
    return out


def psth(x, offsets, W, bin=None, moments=1):  # noqa: A002
    """The sum over the windows of what gather(..., saturate=False) stacks, without storing the stack: int32 [rows,
    ceil(W / bin)]; with moments=2 -> (sum, sumsq), sumsq int64: the sum of the squares of the per-window bin values.
    x and offsets as gather.  ValueError when n * 255 * min(bin, W) reaches 2^31: the sums are int32."""
    from . import _ingest
    x, rows, cols = _matrix(x, "psth")
    W, r, nb = _width(W, bin)
    if moments not in (1, 2):
        raise ValueError("moments is 1 or 2")
    off, checked = _offsets(offsets, cols, W, x.device)
    n = int(off.numel())
    _sum_bound(n, W, r)
    out = torch.empty((rows, nb), dtype=torch.int32, device=x.device)
    sq = torch.empty((rows, nb), dtype=torch.int64, device=x.device) if moments == 2 else None
    bad = _ingest.verify_state(x.device)
    accumulate(x, rows, cols, off, W, r, out, sq, False, bad)
    if not checked:
        _raise_bad(bad, off)
    return out if sq is None else (out, sq)


# ---- the host planner ------------------------------------------------------------------------------------------------
def plan_spans(starts, W, T, join=CHUNK, budget=None):
    """Which sample ranges to read for the windows [s, s + W), s in `starts` (any order, repeats allowed), of a recording of
    T samples, so that every sample is read once.  Pure NumPy: no device, no file.
    The windows are taken in ascending order of s (stable).  A window joins the open span when it starts at or before
    the span's end + join -- join defaults to one chunk: a separate query would decode the chunk that holds its first
    sample anyway, so bridging a shorter gap costs no more than not bridging it.  A span is the range [a, b) from its
    first window's start to its windows' furthest end.  Consecutive spans are packed side by side into one scratch matrix
    of at most `budget` columns (None: no limit), a BATCH; a span that would grow past the budget is closed early, at a
    window boundary -- only such a span may overlap the one behind it, every other pair of spans is disjoint.
    -> Plan(order, batches): order[i] is the caller's index of the i-th window in ascending order; every Batch has spans
    (int64 [m, 2]: a, b), base (int64 [m]: the span's first column in the scratch), cols (the scratch's width), first /
    last (the batch holds the sorted windows first .. last - 1), offsets (int64: where each of those windows starts in the
    scratch, base[span] + s - a) and early (bool [m]: the budget closed the span).
    ValueError: a window that is not inside [0, T) (the first such s is named), W wider than the budget."""
    s = np.asarray(starts)
    if s.size == 0:
        return Plan(np.zeros(0, np.int64), [])
    if s.ndim != 1 or s.dtype.kind not in "iu":
        raise ValueError("starts are a 1-D integer array")
    W, T, join = int(W), int(T), int(join)
    if W < 1 or join < 0:
        raise ValueError("W >= 1 and join >= 0")
    s = s.astype(np.int64)
    out = np.nonzero((s < 0) | (s > T - W))[0]
    if out.size:
        raise ValueError("window %d: [%d, %d) is not inside [0, %d)" % (out[0], int(s[out[0]]), int(s[out[0]]) + W, T))
    if budget is not None and W > int(budget):
        raise ValueError("a window of %d samples is wider than the budget of %d columns" % (W, int(budget)))
    order = np.argsort(s, kind="stable")
    s = s[order]
    # spans: (a, b, first window, one past the last, closed early)
    spans, a, b, first = [], int(s[0]), int(s[0]) + W, 0
    for i in range(1, s.size):
        st = int(s[i])
        fits = budget is None or st + W - a <= budget    # s ascends: st + W is the furthest end
        if st <= b + join and fits:
            b = st + W
        else:
            spans.append((a, b, first, i, st <= b + join))
            a, b, first = st, st + W, i
    spans.append((a, b, first, s.size, False))
    batches, i = [], 0
    while i < len(spans):
        j, cols = i, 0
        while j < len(spans) and (j == i or budget is None or cols + spans[j][1] - spans[j][0] <= budget):
            cols += spans[j][1] - spans[j][0]
            j += 1
        part = np.array(spans[i:j], np.int64)
        base = np.concatenate([[0], np.cumsum(part[:, 1] - part[:, 0])[:-1]]).astype(np.int64)
        lo, hi = int(part[0, 2]), int(part[-1, 3])
        which = np.repeat(np.arange(j - i), part[:, 3] - part[:, 2])
        offsets = base[which] + s[lo:hi] - part[which, 0]
        batches.append(Batch(part[:, :2].copy(), base, int(cols), lo, hi, offsets, part[:, 4].astype(bool)))
        i = j
    return Plan(order, batches)


# ---- what the two readers share --------------------------------------------------------------------------------------
def window_args(triggers, pre, post, bin, reduce, moments, T):  # noqa: A002
    """The argument rules of read_windows / decompress_windows, before anything is read -> (starts int64, W, r, nb)"""
    pre, post = int(pre), int(post)
    if pre < 0 or post < 0 or pre + post < 1:
        raise ValueError("pre >= 0, post >= 0 and pre + post >= 1")
    W, r, nb = _width(pre + post, bin, MAX_BIN)
    if reduce not in (None, "sum"):
        raise ValueError('reduce is None or "sum"')
    if moments not in (1, 2):
        raise ValueError("moments is 1 or 2")
    if isinstance(triggers, torch.Tensor):
        triggers = triggers.cpu().numpy()
    t = np.asarray(triggers)
    if t.size == 0:
        t = t.astype(np.int64).reshape(-1)
    if t.ndim != 1 or t.dtype.kind not in "iu":
        raise ValueError("triggers are a 1-D integer array")
    t = t.astype(np.int64)          # (a uint64 of 2^63 and more wraps below 0: refused as well)
    out = np.nonzero((t < pre) | (t > T - post))[0]
    if out.size:
        k = int(t[out[0]])
        raise ValueError("trigger %d: the window [%d, %d) is not inside [0, %d)" % (k, k - pre, k + post, T))
    if reduce == "sum":
        _sum_bound(int(t.size), W, r)
    return t - pre, W, r, nb


def read_windows(read_span, rows, starts, W, r, nb, reduce, moments, saturate, T, join, max_bytes, device="cuda"):
    """plan_spans, then per batch one scratch [rows, cols], read_span(a, b, view) for every span -- it fills the uint8
    view [rows, b - a] with the samples [a, b) -- and one mhi_windows: STACK through the plan's permutation, or SUM that
    adds from the second batch on.  One synchronisation at the end, for the kernel's own count of refused windows."""
    from . import _ingest
    n = int(starts.size)
    stacked = reduce is None
    if stacked:
        res = torch.empty((n, rows, nb), dtype=torch.uint8 if saturate else torch.int32, device=device)
        sq = None
    else:
        res = torch.zeros((rows, nb), dtype=torch.int32, device=device)
        sq = torch.zeros((rows, nb), dtype=torch.int64, device=device) if moments == 2 else None
    if n and rows:
        budget = max(int(max_bytes) // rows, 1)
        plan = plan_spans(starts, W, T, join, budget)
        bad = _ingest.verify_state(device)
        order = torch.from_numpy(plan.order).to(device)
        for k, bt in enumerate(plan.batches):
            scratch = torch.empty((rows, bt.cols), dtype=torch.uint8, device=device)
            for (a, b), base in zip(bt.spans.tolist(), bt.base.tolist()):
                read_span(a, b, scratch[:, base:base + b - a])
            off = torch.from_numpy(bt.offsets).to(device)
            if stacked:
                stack(scratch, rows, bt.cols, off, order[bt.first:bt.last], W, r, res, bad)
            else:
                accumulate(scratch, rows, bt.cols, off, W, r, res, sq, k > 0, bad)
        n_bad = int(bad[0])     # synchronises: the scratch of the last batch is free to go after this
        if n_bad:
            raise RuntimeError("read_windows: %d windows fell outside their scratch" % n_bad)
    return res if stacked or sq is None else (res, sq)
