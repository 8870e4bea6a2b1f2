"""ctypes binding of libmuahuff_sweep.so (include/muahuff_sweep.h), the fifth companion of libmuahuff.so: the Wiener
statistics of every clip of the dynamic-range sweep, every lag difference and every range of columns in one pass over
the counts.  Fails loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_sweep.so")

# every symbol include/muahuff_sweep.h declares, with its prototype
PROTOTYPES = {
    "mhq_version": (_int, []),
    "mhq_last_error": (ct.c_char_p, []),
    "mhq_gram_clips": (_int, [_vp, _u64, _u64, _u64, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp]),
    "mhq_xty_clips_scratch_bytes": (_int, [_u64, _u64, _u32, _u32, _u32, _u32, ct.POINTER(_u64)]),
    "mhq_xty_clips": (_int, [_vp, _u64, _u64, _u64, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
}
# mh_sweep_layout.hpp: kSweepMaxRanges, kSweepMaxClips, kSweepMaxBlocks, kSweepXtyMaxBlocks
MAX_RANGES, MAX_CLIPS, MAX_BLOCKS, XTY_MAX_BLOCKS = 16, 64, 2048, 4096

_library = Library(globals(), "libmuahuff_sweep.so", "mhq_last_error")
lib, check = _library.lib, _library.check


def _host(ranges, clips):
    """the host arrays of a call: 2 * n_ranges uint64 and n_clips uint32"""
    flat = [int(v) for ab in ranges for v in ab]
    return (_u64 * len(flat))(*flat), len(flat) // 2, (_u32 * len(clips))(*[int(q) for q in clips]), len(clips)


def gram_clips(x_ptr, x_row_stride, rows, cols, ranges, clips, lags, gram, sums):
    """Enqueue mhq_gram_clips on the current stream.  x_ptr: the address of the counts' first byte (row c at
    x_ptr + c*x_row_stride, cols bytes); ranges: [(a, b)] of columns; clips: ascending ints; gram, sums: contiguous int64
    device tensors of n_ranges*n_clips*lags*rows*rows and n_ranges*n_clips*rows elements, which the call ADDS to."""
    import torch
    r, nr, q, nq = _host(ranges, clips)
    for t, n in ((gram, nr * nq * lags * rows * rows), (sums, nr * nq * rows)):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("gram and sums are contiguous int64 tensors of ranges * clips * lags * rows * rows and ranges * clips * rows elements")
    check(lib().mhq_gram_clips(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), r, nr, q, nq, int(lags),
                               _vp(gram.data_ptr()), _vp(sums.data_ptr()), _vp(torch.cuda.current_stream().cuda_stream)))


def xty_clips_scratch_bytes(rows, cols, lags, k, n_ranges, n_clips):
    """mhq_xty_clips_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhq_xty_clips_scratch_bytes(int(rows), int(cols), int(lags), int(k), int(n_ranges), int(n_clips), ct.byref(b)))
    return int(b.value)


def xty_clips(x_ptr, x_row_stride, rows, cols, ranges, clips, lags, lead, y_ptr, y_row_stride, k, out, scratch):
    """Enqueue mhq_xty_clips on the current stream.  x_ptr as for gram_clips; y_ptr: the address of the covariates' first
    float (row j at y_ptr + j*y_row_stride bytes, cols floats); out: contiguous float64 device tensor of
    n_ranges*n_clips*lags*rows*k elements; scratch: uint8 device tensor of at least xty_clips_scratch_bytes(...) bytes."""
    import torch
    r, nr, q, nq = _host(ranges, clips)
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != nr * nq * lags * rows * k:
        raise ValueError("the result is a contiguous float64 tensor of ranges * clips * lags * rows * k elements")
    check(lib().mhq_xty_clips(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), r, nr, q, nq, int(lags), int(lead),
                              _vp(int(y_ptr)), int(y_row_stride), int(k), _vp(out.data_ptr()), _vp(scratch.data_ptr()),
                              int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))
