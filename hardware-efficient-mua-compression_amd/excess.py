"""Exact counts: what the codec's clip at S-1 drops, kept as a sparse side list (mhi_excess_count / mhi_excess_emit /
mhi_excess_apply, include/muahuff_ingest.h).  The codec stores min(x, S-1) -- the reference's design
(get_BR_with_approx_sort.py:143,164 clips before it prices anything) -- and with exact=True the writers keep every
element x > S-1 as one entry (pos = the sample inside its channel, val = x - (S-1)): channel-major, ascending in pos.
The Huffman stream is what it is without the list; a reader adds the list back onto the decoded counts.

This module holds what the container, the stream and the archive share: making the list on the device, indexing it by
directory segment on the host, range-checking one that came from a file, and putting it back.
"""
import numpy as np

ENTRY_BITS = 40   # a stored entry: uint32 pos + uint8 val
NAMES = (("exc_seg", np.uint64), ("exc_pos", np.uint32), ("exc_val", np.uint8))   # the container's arrays, in file order


def _i64(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(device)


def _make(form, x, row_off, lo, hi, rows, cols, thr, channels, device):
    """count -> ONE read of total (synchronises the current stream) -> emit.  -> (exc_off int64 [channels + 1] device,
    pos int32 [n] device holding uint32 values, val uint8 [n] device)"""
    import torch

    from . import _ingest
    scratch = torch.empty(_ingest.excess_scratch_bytes(form, rows, cols), dtype=torch.uint8, device=device)
    exc_off = torch.empty(channels + 1, dtype=torch.int64, device=device)
    state = torch.zeros(2, dtype=torch.int64, device=device)   # total, over
    _ingest.excess_count(form, x, row_off, lo, hi, rows, cols, thr, exc_off, state[0:1], scratch)
    n = int(state[0].item())
    pos = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    val = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    if n:
        _ingest.excess_emit(form, x, row_off, lo, hi, rows, cols, thr, pos, val, state[1:2], scratch, capacity=n)
    return exc_off, pos[:n], val[:n]


def from_rows(data, ch_off, lo, hi, cols, thr):
    """The list of a channel-major buffer (ROWS form): row i = data[ch_off[i]:], its columns [lo[i], hi[i]) examined.
    data: uint8 device tensor; ch_off, lo, hi: host integer arrays; cols: the longest row."""
    from . import _ingest
    dev = data.device
    rows = len(ch_off)
    return _make(_ingest.EXCESS_ROWS, data, _i64(ch_off, dev), _i64(lo, dev), _i64(hi, dev), rows, int(cols), int(thr), rows, dev)


def from_time_major(block, thr):
    """The list of a contiguous time-major [T, C] uint8 device block (COLS form): what from_rows gives on block.T."""
    from . import _ingest
    T, C = int(block.shape[0]), int(block.shape[1])
    return _make(_ingest.EXCESS_COLS, block, None, None, None, T, C, int(thr), C, block.device)


def segment_bounds(ch_len, h, window, seg_chunks, revision):
    """-> int64 arrays (channel, lo, hi) of every directory entry: its channel and its samples [lo, hi) (Directory.bounds)."""
    from .container_io import Directory
    return Directory.build(ch_len, h, window, seg_chunks, revision).bounds()


def segment_index(exc_off, pos, seg_ch, seg_lo):
    """exc_seg u64 [n_segments + 1]: the first entry of every directory segment, by searchsorted on (channel, pos)."""
    exc_off = np.asarray(exc_off, np.int64)
    key = (np.repeat(np.arange(len(exc_off) - 1, dtype=np.int64), np.diff(exc_off)) << 32) | np.asarray(pos, np.uint32).astype(np.int64)
    q = (np.asarray(seg_ch, np.int64) << 32) | np.asarray(seg_lo, np.int64)
    return np.concatenate([np.searchsorted(key, q, side="left"), [len(key)]]).astype(np.uint64)


def crc32(exc_seg, exc_pos, exc_val):
    """zlib's CRC-32 over the three arrays as a container holds them: little-endian, each padded to 8 bytes."""
    from .container_io import crc32_padded
    return crc32_padded((np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8), None)
                        for a, (_name, dt) in zip((exc_seg, exc_pos, exc_val), NAMES))


def check_index(exc_seg, n_segments, n, what="container"):
    seg = np.asarray(exc_seg, np.uint64)
    if len(seg) != n_segments + 1:
        raise ValueError("corrupt %s: exc_seg has %d entries for %d segments" % (what, len(seg), n_segments))
    if int(seg[0]) != 0 or int(seg[-1]) != n or int(seg.max()) > n or (seg[1:] < seg[:-1]).any():
        raise ValueError("corrupt %s: exc_seg is not a monotone index of %d entries" % (what, n))


def check_entries(pos, val, counts, seg_lo, seg_hi, thr, what="container"):
    """The range check of the entries of some segments: counts[s] consecutive entries of (pos, val) belong to a segment of
    samples [seg_lo[s], seg_hi[s]) -- inside it, ascending, 1 <= val and thr + val <= 255.  ValueError."""
    pos, val = np.asarray(pos, np.uint32).astype(np.int64), np.asarray(val, np.uint8).astype(np.int64)
    counts = np.asarray(counts, np.int64)
    if int(counts.sum()) != len(pos) or len(pos) != len(val):
        raise ValueError("corrupt %s: the excess list does not have the entries its index gives" % what)
    if len(pos) == 0:
        return
    s = np.repeat(np.arange(len(counts)), counts)
    if (pos < np.asarray(seg_lo, np.int64)[s]).any() or (pos >= np.asarray(seg_hi, np.int64)[s]).any():
        raise ValueError("corrupt %s: an excess entry lies outside its segment" % what)
    if ((pos[1:] <= pos[:-1]) & (s[1:] == s[:-1])).any():
        raise ValueError("corrupt %s: excess entries of a segment do not ascend" % what)
    if val.min() < 1 or int(thr) + int(val.max()) > 255:
        raise ValueError("corrupt %s: an excess value is out of range" % what)


def check_container(c, what="container"):
    """Everything check_index and check_entries can say about a whole `Compressed` with lists.  ValueError."""
    from .container_io import Directory
    check_index(c.exc_seg, len(c.seg_words), len(c.exc_pos), what)
    _ch, lo, hi = Directory.of(c).bounds()
    check_entries(c.exc_pos, c.exc_val, np.diff(np.asarray(c.exc_seg, np.uint64).astype(np.int64)), lo, hi,
                  int(c.header["S"]) - 1, what)


def upload(pos, val, device):
    import torch
    p = torch.from_numpy(np.ascontiguousarray(pos, np.uint32).view(np.int32)).to(device)
    v = torch.from_numpy(np.ascontiguousarray(val, np.uint8)).to(device)
    return p, v


def apply(pos, val, first, last, start, stop, r, lead, out, row_stride=None, col_stride=None, ptr=None):
    """Enqueue mhi_excess_apply on the current stream: add the entries [first[i], last[i]) of the device list (pos, val)
    onto row i of `out` (uint8: saturating, or int32: exact).  first / last: host integer arrays.  The strides (bytes)
    default to those of the 2-D tensor `out`; ptr: the address of element (0, 0) when it is not out's."""
    from . import _ingest
    if len(first) == 0 or pos.numel() == 0 or stop <= start:
        return
    es = out.element_size()
    rs = (out.stride(0) if out.dim() == 2 else 0) * es if row_stride is None else int(row_stride)
    cs = (out.stride(-1)) * es if col_stride is None else int(col_stride)
    import torch
    dev = lambda a: a if isinstance(a, torch.Tensor) else _i64(a, pos.device)  # noqa: E731
    _ingest.excess_apply(pos, val, dev(first), dev(last), start, stop, r, lead,
                         out.data_ptr() if ptr is None else ptr, 8 * es, rs, cs)
