"""ctypes binding of libmuahuff_ingest.so (include/muahuff_ingest.h), the companion of libmuahuff.so: spike time stamps ->
binned counts in front of the codec, per-segment payload checksums and the way back from counts to events behind it.  Fails loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_ingest.so")

# every symbol include/muahuff_ingest.h declares, with its prototype
PROTOTYPES = {
    "mhi_version": (_int, []),
    "mhi_last_error": (ct.c_char_p, []),
    "mhi_bin_events": (_int, [_vp, _vp, _u32, _u64, _u64, _u64, _u32, _vp, _vp, _u64, _vp]),
    "mhi_aer_scratch_bytes": (_int, [_u64, _u32, ct.POINTER(_u64)]),
    "mhi_aer_to_csr": (_int, [_vp, _vp, _u32, _u64, _u32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "mhi_seg_crc32": (_int, [_vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "mhi_unbin_scratch_bytes": (_int, [_u32, _u64, _u64, ct.POINTER(_u64)]),
    "mhi_unbin_count": (_int, [_u32, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp]),
    "mhi_unbin_emit": (_int, [_u32, _vp, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _vp, _u32, _u64, _vp, _vp, _u64, _vp]),
    "mhi_excess_scratch_bytes": (_int, [_u32, _u64, _u64, ct.POINTER(_u64)]),
    "mhi_excess_count": (_int, [_u32, _vp, _vp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _vp]),
    "mhi_excess_emit": (_int, [_u32, _vp, _vp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "mhi_excess_apply": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _u32, _u64, _u64, _vp]),
    "mhi_windows": (_int, [_vp, _u64, _u64, _u64, _vp, _vp, _u64, _u64, _u64, _u64, _u32, _vp, _u32, _u64, _u64, _vp, _u64, _u32,
                           _vp, _vp]),
    "mhi_gram": (_int, [_vp, _u64, _u64, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _u32, _vp]),
}
WIN_STACK, WIN_SUM = 0, 1         # MHI_WIN_STACK, MHI_WIN_SUM
EXCESS_ROWS, EXCESS_COLS = 0, 1   # MHI_EXCESS_ROWS, MHI_EXCESS_COLS
UNBIN_CSR, UNBIN_AER = 0, 1       # MHI_UNBIN_CSR, MHI_UNBIN_AER
AER_MAX_CHANNELS = 16384  # MHI_AER_MAX_CHANNELS

_library = Library(globals(), "libmuahuff_ingest.so", "mhi_last_error")
lib, check = _library.lib, _library.check


def bin_events(ev, origin, period, T, bits, out, d_off, chunk_stride=0):
    """Enqueue mhi_bin_events on the current stream: the events of `ev` (an events.EventSet) into `out` (uint8 device
    tensor) at the device offsets `d_off` (int64 / uint64 tensor of C entries)."""
    import torch
    check(lib().mhi_bin_events(_vp(ev.ticks.data_ptr()), _vp(ev.ev_off.data_ptr()), ev.C, int(origin), int(period), int(T),
                               int(bits), _vp(out.data_ptr()), _vp(d_off.data_ptr()), int(chunk_stride),
                               _vp(torch.cuda.current_stream().cuda_stream)))


def aer_scratch_bytes(n, C):
    """mhi_aer_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhi_aer_scratch_bytes(int(n), int(C), ct.byref(b)))
    return int(b.value)


def aer_to_csr(ticks, channels, C, out_ticks, ev_off, dropped, scratch):
    """Enqueue mhi_aer_to_csr on the current stream: the pairs (ticks[i], channels[i]) -- 64-bit and 16- or 32-bit device
    tensors -- partitioned by channel into out_ticks (64-bit, n entries), ev_off (64-bit, C + 1) and dropped (64-bit, 1);
    scratch: uint8 device tensor of at least aer_scratch_bytes(n, C) bytes."""
    import torch
    check(lib().mhi_aer_to_csr(_vp(ticks.data_ptr()), _vp(channels.data_ptr()), 8 * channels.element_size(),
                               int(ticks.numel()), int(C), _vp(out_ticks.data_ptr()), _vp(ev_off.data_ptr()),
                               _vp(dropped.data_ptr()), _vp(scratch.data_ptr()), int(scratch.numel()),
                               _vp(torch.cuda.current_stream().cuda_stream)))


def unbin_scratch_bytes(form, rows, cols):
    """mhi_unbin_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhi_unbin_scratch_bytes(int(form), int(rows), int(cols), ct.byref(b)))
    return int(b.value)


def unbin_count(form, x, row_off, rows, cols, ev_off, total, scratch):
    """Enqueue mhi_unbin_count on the current stream.  x: uint8 device tensor whose data_ptr() is the matrix's first byte;
    row_off: 64-bit device tensor of `rows` byte offsets (UNBIN_CSR) or None (UNBIN_AER, a contiguous [rows, cols] block);
    ev_off: 64-bit device tensor [rows + 1] (CSR) or None; total: 64-bit device tensor [1]; scratch: uint8 device tensor of
    at least unbin_scratch_bytes(form, rows, cols) bytes."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    check(lib().mhi_unbin_count(int(form), p(x), p(row_off), int(rows), int(cols), p(ev_off), p(total), p(scratch),
                                int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))


def unbin_emit(form, x, row_off, rows, cols, origin, period, phase, out_ticks, out_ch, over, scratch, capacity=None):
    """Enqueue mhi_unbin_emit on the current stream, after unbin_count on the same (form, x, row_off, rows, cols, scratch).
    out_ticks: 64-bit device tensor; out_ch: 16- or 32-bit device tensor of as many entries (AER) or None; capacity: the
    entries they hold (default: all of out_ticks); over: 64-bit device tensor [1], zeroed by the caller."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    cap = int(out_ticks.numel()) if capacity is None else int(capacity)
    check(lib().mhi_unbin_emit(int(form), p(x), p(row_off), int(rows), int(cols), int(origin), int(period), int(phase),
                               p(out_ticks), p(out_ch), 8 * out_ch.element_size() if out_ch is not None else 0, cap, p(over),
                               p(scratch), int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))


def excess_scratch_bytes(form, rows, cols):
    """mhi_excess_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhi_excess_scratch_bytes(int(form), int(rows), int(cols), ct.byref(b)))
    return int(b.value)


def excess_count(form, x, row_off, lo, hi, rows, cols, threshold, exc_off, total, scratch):
    """Enqueue mhi_excess_count on the current stream.  x: uint8 device tensor whose data_ptr() is the matrix's first byte;
    row_off / lo / hi: 64-bit device tensors of `rows` entries (EXCESS_ROWS; lo and hi may be None) or None (EXCESS_COLS, a
    contiguous time-major [rows, cols] block); exc_off: 64-bit device tensor [channels + 1]; total: 64-bit device tensor
    [1]; scratch: uint8 device tensor of at least excess_scratch_bytes(form, rows, cols) bytes."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    check(lib().mhi_excess_count(int(form), p(x), p(row_off), p(lo), p(hi), int(rows), int(cols), int(threshold), p(exc_off),
                                 p(total), p(scratch), int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))


def excess_emit(form, x, row_off, lo, hi, rows, cols, threshold, pos, val, over, scratch, capacity=None):
    """Enqueue mhi_excess_emit on the current stream, after excess_count on the same arguments and scratch.  pos: int32 /
    uint32 device tensor, val: uint8 device tensor of as many entries; capacity: the entries they hold (default: all of
    pos); over: 64-bit device tensor [1], zeroed by the caller."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    cap = int(pos.numel()) if capacity is None else int(capacity)
    check(lib().mhi_excess_emit(int(form), p(x), p(row_off), p(lo), p(hi), int(rows), int(cols), int(threshold), p(pos), p(val),
                                cap, p(over), p(scratch), int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))


def excess_apply(pos, val, first, last, start, stop, r, lead, out_ptr, out_bits, row_stride, col_stride, n_entries=None):
    """Enqueue mhi_excess_apply on the current stream.  pos (int32 / uint32) and val (uint8): the list, device tensors;
    first / last: 64-bit device tensors of one entry per output row; out_ptr: the address of element (0, 0); the strides
    are in bytes."""
    import torch
    n = int(pos.numel()) if n_entries is None else int(n_entries)
    check(lib().mhi_excess_apply(_vp(pos.data_ptr()) if n else None, _vp(val.data_ptr()) if n else None, n,
                                 _vp(first.data_ptr()), _vp(last.data_ptr()), int(first.numel()), int(start), int(stop), int(r),
                                 int(lead), _vp(int(out_ptr)), int(out_bits), int(row_stride), int(col_stride),
                                 _vp(torch.cuda.current_stream().cuda_stream)))


def windows(x_ptr, row_stride, rows, cols, win_off, win_idx, n_out, W, r, mode, out_ptr, out_bits, out_win_stride,
            out_row_stride, bad, sumsq=None, sq_row_stride=0, accumulate=False, n_win=None):
    """Enqueue mhi_windows on the current stream.  x_ptr: the address of the matrix's first byte (row i at
    x_ptr + i*row_stride, cols bytes); win_off: 64-bit device tensor of window starts (columns); win_idx: None or a 64-bit
    device tensor of output slots; out_ptr: the address of element (0, 0, 0), the strides in bytes; bad: verify_state();
    sumsq: None or an int64 device tensor whose rows are sq_row_stride bytes apart (WIN_SUM)."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    n = int(win_off.numel()) if n_win is None else int(n_win)
    check(lib().mhi_windows(_vp(int(x_ptr)), int(row_stride), int(rows), int(cols), p(win_off), p(win_idx), n, int(n_out),
                            int(W), int(r), int(mode), _vp(int(out_ptr)), int(out_bits), int(out_win_stride),
                            int(out_row_stride), p(sumsq), int(sq_row_stride), int(bool(accumulate)), p(bad),
                            _vp(torch.cuda.current_stream().cuda_stream)))


def gram(a_ptr, a_row_stride, a_rows, b_ptr, b_row_stride, b_rows, cols, out, sum_a=None, sum_b=None, accumulate=False):
    """Enqueue mhi_gram on the current stream.  a_ptr / b_ptr: the address of each matrix's first byte (row i at
    ptr + i*row_stride, cols bytes); b_ptr None: the symmetric form.  out: int64 device tensor [a_rows, b_rows] with unit
    stride along its last axis; sum_a / sum_b: None or contiguous int64 device tensors of one entry per row."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    if out.dtype != torch.int64 or out.dim() != 2 or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError("the result is an int64 [a_rows, b_rows] tensor with unit stride along its last axis")
    stride = 8 * (int(out.stride(0)) if out.shape[0] > 1 else int(out.shape[1]))
    check(lib().mhi_gram(_vp(int(a_ptr)), int(a_row_stride), int(a_rows), None if b_ptr is None else _vp(int(b_ptr)),
                         int(b_row_stride), int(b_rows), int(cols), p(out), stride, p(sum_a), p(sum_b), int(bool(accumulate)),
                         _vp(torch.cuda.current_stream().cuda_stream)))


def seg_crc32(payload, seg_off, seg_words, n_segments, seg_idx=None, crc=None, expect=None, bad=None, payload_words=None):
    """Enqueue mhi_seg_crc32 on the current stream.  payload: int32 device words (payload_words of them: default all);
    seg_off / seg_words: 64-bit device tensors of n_segments entries; seg_idx: optional 64-bit device list of directory
    indices; crc: int32 / uint32 device tensor [n_segments] to fill; expect: the stored values in the same form and bad: a
    64-bit device tensor [2] the caller set to {0, -1} (verify_state) -- the verify form."""
    import torch
    p = lambda t: _vp(t.data_ptr()) if t is not None else None  # noqa: E731
    check(lib().mhi_seg_crc32(p(payload), int(payload.numel() if payload_words is None else payload_words), p(seg_off),
                              p(seg_words), int(n_segments), p(seg_idx), int(seg_idx.numel()) if seg_idx is not None else 0,
                              p(crc), p(expect), p(bad), _vp(torch.cuda.current_stream().cuda_stream)))


def verify_state(device):
    """-> the `bad` tensor of one checked block or query: int64 [2] = {0 mismatches, -1 = no index yet}"""
    import torch
    return torch.tensor([0, -1], dtype=torch.int64, device=device)
