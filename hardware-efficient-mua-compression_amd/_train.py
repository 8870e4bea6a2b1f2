"""ctypes binding of libmuahuff_train.so (include/muahuff_train.h), the eighth companion of libmuahuff.so: the loss of one
minibatch of an LSTM decoder's windows and its gradient with respect to the weights, from the uint8 counts where they lie.
Fails loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, Library, _int, _u32, _u64, _vp

SO = os.path.join(HERE, "libmuahuff_train.so")

# every symbol include/muahuff_train.h declares, with its prototype
PROTOTYPES = {
    "mht_version": (_int, []),
    "mht_last_error": (ct.c_char_p, []),
    "mht_loss_grad": (_int, [_vp, _u64, _u64, _u64, _u32, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64,
                             ct.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# mh_train_layout.hpp: kTrainMaxBatch, kTrainInRows, kTrainInMaxBlocks, kTrainMaxTiles, kBwdKSteps, kGradTile, kGradThreads,
# kGradMaxBlocks, kTrainDoutPitch
MAX_BATCH, IN_ROWS, IN_MAX_BLOCKS, MAX_TILES, BWD_KSTEPS, GRAD_TILE, GRAD_THREADS, GRAD_MAX_BLOCKS, DOUT_PITCH = 65536, 128, 4096, 1024, 32, 32, 64, 1024, 8

_library = Library(globals(), "libmuahuff_train.so", "mht_last_error")
lib, check = _library.lib, _library.check


def scratch_layout(batch, lags, units):
    """-> dict of the offsets, in floats, of act [R, 4U], dz [R, 4U], c [R, U], h [R, U] and dout [batch, 8] in the scratch,
    R = batch * lags, and `floats`, its size (mh_train_layout.hpp: train_scratch)"""
    R, U = int(batch) * int(lags), int(units)
    return dict(act=0, dz=4 * U * R, c=8 * U * R, h=9 * U * R, dout=10 * U * R, floats=10 * U * R + DOUT_PITCH * int(batch))


def scratch_bytes(batch, lags, units):
    """the bytes of the scratch of one call (mh_train_layout.hpp: scratch_bytes)"""
    return 4 * (int(batch) * int(lags) * 10 * int(units) + DOUT_PITCH * int(batch))


def _f32(t, shape, what):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s is a contiguous float32 tensor %s" % (what, list(shape)))


def prepared(x_ptr, x_row_stride, rows, cols, clip, mean, inv, lags, lead, wx, bias, wh, wd, bd, y, scratch, dwx, dbias, dwh, dwd, dbd):
    """Check once everything of mht_loss_grad that does not change from one minibatch to the next (the tensors as in
    loss_grad) -> run(idx_ptr, batch, scale, out_ptr, loss_ptr), which only enqueues the call on the current stream: a
    training loop checks its tensors before the first step, not at every one.  The closure keeps the tensors alive; the
    scratch bounds the batch, and the library checks what is left."""
    import torch
    if wh.dim() != 2 or wd.dim() != 2:
        raise ValueError("wh is [4 units, units] and wd [k, units]")
    U, k = int(wh.shape[1]), int(wd.shape[0])
    G = 4 * U
    for t, shape, what in ((mean, (rows,), "mean"), (inv, (rows,), "inv"), (wx, (G, rows), "the input weights"), (bias, (G,), "the bias"),
                           (wh, (G, U), "the recurrent weights"), (wd, (k, U), "the dense weights"), (bd, (k,), "the dense bias"),
                           (dwx, (G, rows), "dwx"), (dbias, (G,), "dbias"), (dwh, (G, U), "dwh"), (dwd, (k, U), "dwd"), (dbd, (k,), "dbd")):
        _f32(t, shape, what)
    if y.dtype != torch.float32 or y.dim() != 2 or tuple(y.shape) != (k, cols) or (cols > 1 and y.stride(1) != 1):
        raise ValueError("y is a float32 tensor [k, cols] with unit stride along its last axis")
    if scratch.dtype != torch.float32 or not scratch.is_contiguous():
        raise ValueError("the scratch is a contiguous float32 tensor")
    room, keep = scratch.numel() * 4, (mean, inv, wx, bias, wh, wd, bd, y, scratch, dwx, dbias, dwh, dwd, dbd)
    p = lambda t: _vp(t.data_ptr())  # noqa: E731
    head = (_vp(int(x_ptr)), int(x_row_stride), int(rows), int(cols), int(clip), p(mean), p(inv))
    shape = (int(lags), U, k, int(lead), p(wx), p(bias), p(wh), p(wd), p(bd), p(y), 4 * (int(y.stride(0)) if k > 1 else int(cols)))
    tail = (p(dwx), p(dbias), p(dwh), p(dwd), p(dbd))
    fn, L = lib().mht_loss_grad, int(lags)

    def run(idx_ptr, batch, scale, out_ptr, loss_ptr, _keep=keep):
        if scratch_bytes(batch, L, U) > room:
            raise ValueError("the scratch is a contiguous float32 tensor of at least %d values" % (scratch_bytes(batch, L, U) // 4))
        check(fn(*head, _vp(idx_ptr), batch, *shape, scale, p(scratch), _vp(out_ptr), _vp(loss_ptr), *tail,
                 _vp(torch.cuda.current_stream().cuda_stream)))
    run.units, run.k = U, k
    return run


def loss_grad(x_ptr, x_row_stride, rows, cols, clip, mean, inv, idx, lags, lead, wx, bias, wh, wd, bd, y, scale, scratch, out, loss,
              dwx, dbias, dwh, dwd, dbd):
    """Enqueue mht_loss_grad on the current stream.  x_ptr: the address of the counts' first byte (row c at
    x_ptr + c*x_row_stride, cols bytes); mean, inv: float32 [rows]; idx: int64 [batch]; wx [4U, rows], bias [4U], wh [4U, U],
    wd [k, U], bd [k] and the gradients of the same shapes, out [k, batch], loss [batch]: contiguous float32 device tensors;
    y: float32 [k, cols] with unit stride along its last axis; scratch: a contiguous float32 tensor of at least
    scratch_layout(batch, lags, units)["floats"] values."""
    import torch
    run = prepared(x_ptr, x_row_stride, rows, cols, clip, mean, inv, lags, lead, wx, bias, wh, wd, bd, y, scratch, dwx, dbias, dwh, dwd, dbd)
    if idx.dim() != 1 or idx.dtype != torch.int64 or not idx.is_contiguous():
        raise ValueError("idx is a contiguous int64 tensor [batch]")
    B = int(idx.shape[0])
    _f32(out, (run.k, B), "out")
    _f32(loss, (B,), "loss")
    run(idx.data_ptr(), B, float(scale), out.data_ptr(), loss.data_ptr())
