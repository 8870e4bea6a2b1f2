"""ctypes binding of libmuahuff_kalman.so (include/muahuff_kalman.h), the sixth companion of libmuahuff.so: the prediction
of a Kalman filter decoder, a constant projection of the clipped counts and the scan of an affine recurrence over ranges
of columns.  Fails loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_kalman.so")

# every symbol include/muahuff_kalman.h declares, with its prototype
PROTOTYPES = {
    "mhk_version": (_int, []),
    "mhk_last_error": (ct.c_char_p, []),
    "mhk_project": (_int, [_vp, _u64, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _u64, _vp]),
    "mhk_scan_scratch_bytes": (_int, [_u64, _u32, _u32, ct.POINTER(_u64)]),
    "mhk_scan": (_int, [_vp, _u64, _u32, _u64, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _u64, _vp]),
}
# mh_kalman_layout.hpp: kKalmanMaxK, kKalmanMaxRows, kKalmanMaxGains, kKalmanMaxRanges, kProjTileCols, kProjMaxBlocks,
# kScanTile, kScanThreads, kScanMaxBlocks
MAX_K, MAX_ROWS, MAX_GAINS, MAX_RANGES = 8, 65536, 4096, 16
PROJ_TILE_COLS, PROJ_MAX_BLOCKS, SCAN_TILE, SCAN_THREADS, SCAN_MAX_BLOCKS = 1024, 4096, 512, 64, 512

_library = Library(globals(), "libmuahuff_kalman.so", "mhk_last_error")
lib, check = _library.lib, _library.check


def _rows(t, what):
    import torch
    if t.dtype != torch.float64 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s is a float64 [k, cols] tensor with unit stride along its last axis" % what)


def _row_stride(t, k, cols):
    return 8 * (int(t.stride(0)) if k > 1 else cols)


def project(x_ptr, x_row_stride, rows, cols, clip, m, m0, v):
    """Enqueue mhk_project on the current stream.  x_ptr: the address of the counts' first byte (row c at
    x_ptr + c*x_row_stride, cols bytes); m: contiguous float64 device tensor [k, rows]; m0: None or a contiguous float64
    device tensor of k; v: float64 device tensor [k, cols] with unit stride along its last axis."""
    import torch
    _rows(v, "the projection")
    k = int(v.shape[0])
    if int(v.shape[1]) != cols:
        raise ValueError("the projection has one column per bin")
    if m.dtype != torch.float64 or not m.is_contiguous() or tuple(m.shape) != (k, rows):
        raise ValueError("the matrix is a contiguous float64 tensor [k, rows]")
    if m0 is not None and (m0.dtype != torch.float64 or not m0.is_contiguous() or m0.numel() != k):
        raise ValueError("the offset is a contiguous float64 tensor of k elements")
    check(lib().mhk_project(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), int(clip), _vp(m.data_ptr()),
                            _vp(m0.data_ptr() if m0 is not None else 0), k, _vp(v.data_ptr()), _row_stride(v, k, cols),
                            _vp(torch.cuda.current_stream().cuda_stream)))


def scan_scratch_bytes(cols, k, n_ranges):
    """mhk_scan_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhk_scan_scratch_bytes(int(cols), int(k), int(n_ranges), ct.byref(b)))
    return int(b.value)


def scan(v, ranges, F, B, init, out, scratch):
    """Enqueue mhk_scan on the current stream.  v, out: float64 device tensors [k, cols], unit stride along the last axis
    (out may be v); ranges: [(a, b)] of columns; F, B: contiguous float64 device tensors [n_gain, k, k]; init: contiguous
    float64 device tensor [len(ranges), k]; scratch: uint8 device tensor of at least scan_scratch_bytes(cols, k,
    len(ranges)) bytes."""
    import torch
    _rows(v, "the projection"), _rows(out, "the result")
    k, cols = int(v.shape[0]), int(v.shape[1])
    if tuple(out.shape) != (k, cols):
        raise ValueError("the projection and the result have the same shape")
    flat = [int(u) for ab in ranges for u in ab]
    if min(flat, default=0) < 0:
        raise ValueError("a range starts below 0")
    for t in (F, B):
        if t.dtype != torch.float64 or not t.is_contiguous() or t.dim() != 3 or tuple(t.shape[1:]) != (k, k) or t.shape != F.shape:
            raise ValueError("F and B are contiguous float64 tensors [n_gain, k, k]")
    if init.dtype != torch.float64 or not init.is_contiguous() or tuple(init.shape) != (len(ranges), k):
        raise ValueError("init is a contiguous float64 tensor [ranges, k]")
    host = (_u64 * max(len(flat), 1))(*flat)  # read during the call, by value into the kernel parameters
    check(lib().mhk_scan(_vp(v.data_ptr()), _row_stride(v, k, cols), k, cols, ct.cast(host, _vp), len(ranges), _vp(F.data_ptr()),
                         _vp(B.data_ptr()), int(F.shape[0]), _vp(init.data_ptr()), _vp(out.data_ptr()), _row_stride(out, k, cols),
                         _vp(scratch.data_ptr()), int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))
