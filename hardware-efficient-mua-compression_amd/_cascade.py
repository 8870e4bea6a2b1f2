"""ctypes binding of libmuahuff_cascade.so (include/muahuff_cascade.h), the third companion of libmuahuff.so: the power
sums of a prediction against its target over ranges of columns and the polynomial stage of the Wiener cascade.  Fails
loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_cascade.so")

# every symbol include/muahuff_cascade.h declares, with its prototype
PROTOTYPES = {
    "mhc_version": (_int, []),
    "mhc_last_error": (ct.c_char_p, []),
    "mhc_moments_scratch_bytes": (_int, [_u64, _u32, _u32, _u32, ct.POINTER(_u64)]),
    "mhc_moments": (_int, [_vp, _u64, _vp, _u64, _u32, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _u64, _vp]),
    "mhc_polyval": (_int, [_vp, _u64, _u32, _u64, _vp, _u32, _vp, _vp, _vp, _u64, _vp]),
}
# mh_cascade_layout.hpp: kCascadeMaxK, kCascadeMaxDegree, kMomMaxRanges, kMomRun
MAX_K, MAX_DEGREE, MAX_RANGES, RUN = 8, 6, 16, 16384

_library = Library(globals(), "libmuahuff_cascade.so", "mhc_last_error")
lib, check = _library.lib, _library.check


def per(degree):
    """the sums of one (range, output): T_0..T_2D, Q_0..Q_D, YY, E"""
    return 3 * int(degree) + 4


def moments_scratch_bytes(cols, k, degree, n_ranges):
    """mhc_moments_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhc_moments_scratch_bytes(int(cols), int(k), int(degree), int(n_ranges), ct.byref(b)))
    return int(b.value)


def _row_stride(t, k, cols):
    return 4 * (int(t.stride(0)) if k > 1 else cols)


def _rows(t, what):
    import torch
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s is a float32 [k, cols] tensor with unit stride along its last axis" % what)


def moments(p, y, ranges, degree, center, inv_scale, out, scratch, accumulate=False):
    """Enqueue mhc_moments on the current stream.  p, y: float32 device tensors [k, cols], unit stride along the last
    axis; ranges: [(a, b)] of columns; center, inv_scale: None or contiguous float64 device tensors of k; out: contiguous
    float64 device tensor of len(ranges) * k * per(degree) elements; scratch: uint8 device tensor of at least
    moments_scratch_bytes(cols, k, degree, len(ranges)) bytes."""
    import torch
    _rows(p, "the prediction"), _rows(y, "the target")
    k, cols = int(p.shape[0]), int(p.shape[1])
    if tuple(y.shape) != (k, cols):
        raise ValueError("the prediction and the target have the same shape")
    flat = [int(v) for ab in ranges for v in ab]
    if min(flat, default=0) < 0:
        raise ValueError("a range starts below 0")
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != len(ranges) * k * per(degree):
        raise ValueError("the result is a contiguous float64 tensor of ranges * k * (3 * degree + 4) elements")
    for t in (center, inv_scale):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != k):
            raise ValueError("center and inv_scale are contiguous float64 tensors of k elements")
    host = (_u64 * max(len(flat), 1))(*flat)  # read during the call, by value into the kernel parameters
    check(lib().mhc_moments(_vp(p.data_ptr()), _row_stride(p, k, cols), _vp(y.data_ptr()), _row_stride(y, k, cols), k, cols,
                            ct.cast(host, _vp), len(ranges), int(degree), _vp(center.data_ptr() if center is not None else 0),
                            _vp(inv_scale.data_ptr() if inv_scale is not None else 0), _vp(out.data_ptr()), int(bool(accumulate)),
                            _vp(scratch.data_ptr()), int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))


def polyval(p, coef, center, inv_scale, out):
    """Enqueue mhc_polyval on the current stream.  p, out: float32 device tensors [k, cols], unit stride along the last
    axis (out may be p); coef: contiguous float32 device tensor [k, degree + 1], highest power first; center, inv_scale:
    None or contiguous float32 device tensors of k."""
    import torch
    _rows(p, "the prediction"), _rows(out, "the result")
    k, cols = int(p.shape[0]), int(p.shape[1])
    if tuple(out.shape) != (k, cols):
        raise ValueError("the prediction and the result have the same shape")
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.dim() != 2 or coef.shape[0] != k or coef.shape[1] < 2:
        raise ValueError("the coefficients are a contiguous float32 tensor [k, degree + 1]")
    for t in (center, inv_scale):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != k):
            raise ValueError("center and inv_scale are contiguous float32 tensors of k elements")
    check(lib().mhc_polyval(_vp(p.data_ptr()), _row_stride(p, k, cols), k, cols, _vp(coef.data_ptr()), int(coef.shape[1]) - 1,
                            _vp(center.data_ptr() if center is not None else 0),
                            _vp(inv_scale.data_ptr() if inv_scale is not None else 0), _vp(out.data_ptr()), _row_stride(out, k, cols),
                            _vp(torch.cuda.current_stream().cuda_stream)))
