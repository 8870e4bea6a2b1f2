"""ctypes binding of libmuahuff_wiener.so (include/muahuff_wiener.h), the second companion of libmuahuff.so: the products
of spike counts with float covariates at every lag and the prediction of a lagged linear filter.  Fails loudly: there is
no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_wiener.so")

# every symbol include/muahuff_wiener.h declares, with its prototype
PROTOTYPES = {
    "mhw_version": (_int, []),
    "mhw_last_error": (ct.c_char_p, []),
    "mhw_xty_scratch_bytes": (_int, [_u64, _u64, _u32, _u32, ct.POINTER(_u64)]),
    "mhw_xty": (_int, [_vp, _u64, _u64, _u64, _u32, _u32, _vp, _u64, _u32, _vp, _u32, _vp, _u64, _vp]),
    "mhw_fir": (_int, [_vp, _u64, _u64, _u64, _u32, _u32, _vp, _vp, _u32, _vp, _u64, _vp]),
}
MAX_LAGS, MAX_K, MAX_ROWS = 32, 8, 65536  # mh_wiener_layout.hpp: kWienerMaxLags, kWienerMaxK, kWienerMaxRows

_library = Library(globals(), "libmuahuff_wiener.so", "mhw_last_error")
lib, check = _library.lib, _library.check


def xty_scratch_bytes(rows, cols, lags, k):
    """mhw_xty_scratch_bytes: host arithmetic, no device."""
    b = _u64(0)
    check(lib().mhw_xty_scratch_bytes(int(rows), int(cols), int(lags), int(k), ct.byref(b)))
    return int(b.value)


def xty(x_ptr, x_row_stride, rows, cols, lags, clip, y_ptr, y_row_stride, k, out, scratch, accumulate=False):
    """Enqueue mhw_xty on the current stream.  x_ptr: the address of the counts' first byte (row c at
    x_ptr + c*x_row_stride, cols + lags - 1 bytes); y_ptr: the address of the covariates' first float (row j at
    y_ptr + j*y_row_stride bytes, cols floats); out: contiguous float64 device tensor of lags*rows*k elements; scratch:
    uint8 device tensor of at least xty_scratch_bytes(rows, cols, lags, k) bytes."""
    import torch
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != lags * rows * k:
        raise ValueError("the result is a contiguous float64 tensor of lags * rows * k elements")
    check(lib().mhw_xty(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), int(lags), int(clip), _vp(int(y_ptr)),
                        int(y_row_stride), int(k), _vp(out.data_ptr()), int(bool(accumulate)), _vp(scratch.data_ptr()),
                        int(scratch.numel()), _vp(torch.cuda.current_stream().cuda_stream)))


def fir(x_ptr, x_row_stride, rows, cols, lags, clip, w, bias, k, out):
    """Enqueue mhw_fir on the current stream.  x_ptr: as for xty; w: contiguous float32 device tensor of k*lags*rows
    weights, bias: of k; out: float32 device tensor [k, cols] with unit stride along its last axis."""
    import torch
    for t, n in ((w, k * lags * rows), (bias, k)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("weights and bias are contiguous float32 tensors of k * lags * rows and k elements")
    if out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (k, cols) or (cols > 1 and out.stride(1) != 1):
        raise ValueError("the result is a float32 [k, cols] tensor with unit stride along its last axis")
    stride = 4 * (int(out.stride(0)) if k > 1 else cols)
    check(lib().mhw_fir(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), int(lags), int(clip), _vp(w.data_ptr()),
                        _vp(bias.data_ptr()), int(k), _vp(out.data_ptr()), stride,
                        _vp(torch.cuda.current_stream().cuda_stream)))
