"""ctypes binding of libmuahuff_smooth.so (include/muahuff_smooth.h), the fourth companion of libmuahuff.so: the box sums
of the decoders' moving-average window, as byte planes of the clipped counts and on a float prediction.  Fails loudly:
there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_smooth.so")

# every symbol include/muahuff_smooth.h declares, with its prototype
PROTOTYPES = {
    "mhs_version": (_int, []),
    "mhs_last_error": (ct.c_char_p, []),
    "mhs_box": (_int, [_vp, _u64, _u64, _u64, _u32, _u32, _vp, _vp, _u64, _vp]),
    "mhs_box_f32": (_int, [_vp, _u64, _u32, _u64, _u32, _vp, _vp, _u64, _vp]),
}
# mh_smooth_layout.hpp: kBoxMaxWindow, kBoxfMaxK, kBoxMaxRows, kBoxTileCols, kBoxMaxBlocks
MAX_WINDOW, MAX_K, MAX_ROWS, TILE_COLS, MAX_BLOCKS = 256, 8, 65536, 3824, 2048
MAX_SUM = 65535  # window * clip at most: a box sum fits two byte planes

_library = Library(globals(), "libmuahuff_smooth.so", "mhs_last_error")
lib, check = _library.lib, _library.check


def box(x_ptr, x_row_stride, rows, cols, window, clip, lo, hi):
    """Enqueue mhs_box on the current stream.  x_ptr: the address of the counts' first byte (row c at
    x_ptr + c*x_row_stride, cols + window - 1 bytes); lo, hi: uint8 device tensors [rows, cols] with unit stride along the
    last axis, a row pitch and a first byte that are multiples of 16, and one pitch for both; hi None: one plane."""
    import torch
    for t in (lo, hi):
        if t is None:
            continue
        if t.dtype != torch.uint8 or t.dim() != 2 or tuple(t.shape) != (rows, cols) or (cols > 1 and t.stride(1) != 1):
            raise ValueError("a plane is a uint8 [rows, cols] tensor with unit stride along its last axis")
        if rows > 1 and t.stride(0) != lo.stride(0):
            raise ValueError("the two planes have one row pitch")
    stride = int(lo.stride(0)) if rows > 1 else 0
    check(lib().mhs_box(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), int(window), int(clip), _vp(lo.data_ptr()),
                        _vp(hi.data_ptr() if hi is not None else 0), stride, _vp(torch.cuda.current_stream().cuda_stream)))


def box_f32(p, window, bias, out):
    """Enqueue mhs_box_f32 on the current stream.  p, out: float32 device tensors [k, cols], unit stride along the last
    axis; bias: contiguous float32 device tensor of k."""
    import torch
    for t in (p, out):
        if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("the prediction and the result are float32 [k, cols] tensors with unit stride along the last axis")
    k, cols = int(p.shape[0]), int(p.shape[1])
    if tuple(out.shape) != (k, cols):
        raise ValueError("the prediction and the result have the same shape")
    if bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != k:
        raise ValueError("the bias is a contiguous float32 tensor of k elements")
    check(lib().mhs_box_f32(_vp(p.data_ptr()), 4 * int(p.stride(0)) if k > 1 else 0, k, cols, int(window), _vp(bias.data_ptr()),
                            _vp(out.data_ptr()), 4 * int(out.stride(0)) if k > 1 else 0, _vp(torch.cuda.current_stream().cuda_stream)))
