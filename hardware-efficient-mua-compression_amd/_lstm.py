"""ctypes binding of libmuahuff_lstm.so (include/muahuff_lstm.h), the seventh companion of libmuahuff.so: the prediction
of an LSTM decoder, the input half of the gate pre-activations once per bin and the recurrence over every window of
`lags` bins.  Fails loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_lstm.so")

# every symbol include/muahuff_lstm.h declares, with its prototype
PROTOTYPES = {
    "mhl_version": (_int, []),
    "mhl_last_error": (ct.c_char_p, []),
    "mhl_inproj": (_int, [_vp, _u64, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _vp]),
    "mhl_windows": (_int, [_vp, _u64, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _u64, _vp]),
}
# mh_lstm_layout.hpp: kLstmMaxUnits, kLstmMaxLags, kLstmMaxK, kLstmMaxRows, kInTileCols, kInGTile, kInMaxBlocks, kWinTile,
# kWinWaves, kWinBlockUnits, kWinKGroup, kWinMaxBlocks
MAX_UNITS, MAX_LAGS, MAX_K, MAX_ROWS = 128, 32, 8, 65536
IN_TILE_COLS, IN_GTILE, IN_MAX_BLOCKS = 512, 32, 8192
WIN_TILE, WIN_WAVES, WIN_BLOCK_UNITS, WIN_KGROUP, WIN_MAX_BLOCKS = 32, 8, 8, 8, 4096

_library = Library(globals(), "libmuahuff_lstm.so", "mhl_last_error")
lib, check = _library.lib, _library.check


def inproj_bytes(cols, units):
    """the bytes of the scratch matrix p of `cols` bins (mh_lstm_layout.hpp: inproj_bytes)"""
    return int(cols) * 16 * int(units)


def _f32(t, shape, what):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
        raise ValueError("%s is a contiguous float32 tensor %s" % (what, list(shape)))


def inproj(x_ptr, x_row_stride, rows, cols, clip, wx, bias, p):
    """Enqueue mhl_inproj on the current stream.  x_ptr: the address of the counts' first byte (row c at
    x_ptr + c*x_row_stride, cols bytes); wx: contiguous float32 device tensor [4U, rows]; bias: contiguous float32 device
    tensor [4U]; p: contiguous float32 device tensor [cols, 4U]."""
    import torch
    if p.dim() != 2 or p.shape[1] % 4 or p.shape[1] < 4:
        raise ValueError("the pre-activations are a float32 tensor [cols, 4 units]")
    G = int(p.shape[1])
    _f32(p, (cols, G), "the pre-activations")
    _f32(wx, (G, rows), "the input weights")
    _f32(bias, (G,), "the bias")
    check(lib().mhl_inproj(_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), int(clip), _vp(wx.data_ptr()), _vp(bias.data_ptr()),
                           G // 4, _vp(p.data_ptr()), _vp(torch.cuda.current_stream().cuda_stream)))


def windows(p, lags, wh, wd, bd, out):
    """Enqueue mhl_windows on the current stream.  p: contiguous float32 device tensor [cols, 4U]; wh: [4U, U], wd: [k, U],
    bd: [k], contiguous float32 device tensors; out: float32 device tensor [k, cols - lags + 1] with unit stride along its
    last axis."""
    import torch
    if p.dim() != 2 or p.shape[1] % 4 or p.shape[1] < 4:
        raise ValueError("the pre-activations are a float32 tensor [cols, 4 units]")
    cols, G = int(p.shape[0]), int(p.shape[1])
    U, n = G // 4, cols - int(lags) + 1
    _f32(p, (cols, G), "the pre-activations")
    _f32(wh, (G, U), "the recurrent weights")
    if wd.dim() != 2:
        raise ValueError("the dense weights are a float32 tensor [k, units]")
    k = int(wd.shape[0])
    _f32(wd, (k, U), "the dense weights")
    _f32(bd, (k,), "the dense bias")
    if out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (k, n) or (n > 1 and out.stride(1) != 1):
        raise ValueError("the result is a float32 tensor [k, cols - lags + 1] with unit stride along its last axis")
    check(lib().mhl_windows(_vp(p.data_ptr()), cols, int(lags), U, _vp(wh.data_ptr()), _vp(wd.data_ptr()), _vp(bd.data_ptr()), k,
                            _vp(out.data_ptr()), 4 * (int(out.stride(0)) if k > 1 else n), _vp(torch.cuda.current_stream().cuda_stream)))
