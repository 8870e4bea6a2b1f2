"""Host-side handle on the gfx950 data plane: plan once, then launch measure / encode / decode.

All tensors are torch tensors on the plan's GPU; torch is only the allocator and the stream
provider here -- every kernel is in libmuahuff.so and is launched on torch's current stream.
"""
import ctypes as ct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import (MODE_APPROX, MODE_NOSORT, WIN_AFTER_CAL, WIN_FULL,  # noqa: F401
                   WIN_REF_HALF, WIN_REF_HALF_TRUNC)


def _ptr(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu():
    if not torch.cuda.is_available():
        raise _lib.MuaHuffError(_lib.ERR_NO_DEVICE, "no MI355X visible; this package has no CPU fallback")


# ---- what every range / re-bin query shares -------------------------------------------------------
def select_channels(C, channels):
    """-> int64 channel indices (None = all C; any order, repeats allowed); IndexError outside 0..C-1"""
    sel = np.arange(C, dtype=np.int64) if channels is None else np.asarray(channels, dtype=np.int64).reshape(-1)
    if sel.size and (sel.min() < 0 or sel.max() >= C):
        raise IndexError("channel index out of range")
    return sel


def query_args(max_len, C, start, stop, channels, r=None):
    """The argument rules of every range query: 0 <= start <= stop <= max_len; with a bin factor, 1 <= r <= 4096 and
    start a multiple of r (ValueError); channel indices inside 0..C-1 (IndexError).  -> sel (select_channels)"""
    if r is not None and not 1 <= r <= 4096:
        raise ValueError("bin factor %d outside 1..4096" % r)
    if not (0 <= start <= stop <= max_len):
        raise ValueError("range [%d, %d) is not inside [0, %d)" % (start, stop, max_len))
    if r is not None and start % r:
        raise ValueError("start %d is not a multiple of the bin factor %d" % (start, r))
    return select_channels(C, channels)


def check_out(out, rows, cols, dtype, axis_name):
    """ValueError unless `out` is a [rows, cols] tensor of `dtype` with unit stride along its last axis"""
    if tuple(out.shape) != (rows, cols) or out.dtype != dtype or (cols > 1 and rows and out.stride(1) != 1):
        raise ValueError("out must be a %s [%d, %d] tensor with unit stride along %s" % (dtype, rows, cols, axis_name))


def aligned_rows(rows, n, phase, device):
    """uint8 [rows, n] view of a fresh buffer whose column t sits at a byte address congruent to phase + t mod 128 (the
    range decoder's interior row stores are then as aligned as mh_decode's)"""
    phase %= 128
    pitch = (n + phase + 127) // 128 * 128
    buf = torch.empty(max(rows * pitch, 1), dtype=torch.uint8, device=device)
    return buf.as_strided((rows, n), (pitch, 1), phase)


def upload_stream(device, payload, seg, peak, enc):
    """A host stream on the device -> (payload int32 behind four zero words of slack, seg int64, peak, enc uint8).
    payload: uint32 words; seg: the segments' offsets or sizes, 64-bit."""
    pay = torch.zeros(payload.size + 4, dtype=torch.int32, device=device)
    if payload.size:
        pay[:payload.size] = torch.from_numpy(np.ascontiguousarray(payload).view(np.int32)).to(device)
    seg = np.ascontiguousarray(seg)
    seg = seg.view(np.int64) if seg.dtype.itemsize == 8 else seg.astype(np.int64)
    return (pay, torch.from_numpy(seg).to(device), torch.from_numpy(np.array(peak, np.uint8)).to(device),
            torch.from_numpy(np.array(enc, np.uint8)).to(device))


def check_decoded(plans, what="container", unwinding=False):
    """Read and clear the status of every plan (synchronises); ValueError when a decode on one of them had to abandon
    a segment -- unless the caller is `unwinding` from an error of its own."""
    ok = all([p.decode_ok() for p in plans])
    if not (ok or unwinding):
        raise ValueError("corrupt %s: a chunk header points outside the payload (decode abandoned)" % what)


def to_time_major(rows):
    """uint8 [R, n] rows with unit stride along time (any row stride) -> contiguous [n, R] (mh_interleave)"""
    R, n = int(rows.shape[0]), int(rows.shape[1])
    tm = torch.empty((n, R), dtype=torch.uint8, device=rows.device)
    in_off = torch.arange(R, dtype=torch.int64, device=rows.device) * (rows.stride(0) if R > 1 else 0)
    _lib.check(_lib.lib().mh_interleave(_ptr(rows), _ptr(in_off), n, R, _ptr(tm), _stream()))
    return tm


@dataclass
class Measured:
    """What the reference computes per validation channel at one (S, h) --
    get_BR_with_approx_sort.py:164-193 and the numerator of :289."""
    cutoff: torch.Tensor      # uint64 [C]   (carried as int64)
    cal_hist: torch.Tensor    # int32  [C,S] calibration histogram, rank order (val_histograms)
    peak: torch.Tensor        # uint8  [C]
    enc: torch.Tensor         # uint8  [C]   first argmin over the plan's SCLV rows
    post_hist: torch.Tensor   # int64  [C,S] window histogram, rank order (val_histograms_post)
    bits: torch.Tensor        # int64  [C]   SCLV[enc] . post_hist
    skipped: torch.Tensor     # uint8  [C]


@dataclass
class Encoded:
    payload: torch.Tensor     # int32 words; segment s at word seg_off[s]
    seg_words: torch.Tensor   # int64 [n_segments] words used by each segment
    ch_bits: torch.Tensor     # int64 [C] exact code bits per channel
    peak: torch.Tensor
    enc: torch.Tensor
    skipped: torch.Tensor
    seg_off: torch.Tensor = None  # int64 [n_segments] device; None = the plan's slots
    dense: bool = False


class Plan:
    """One design point (S, h, mapper, window rule, K candidate encoders) over one channel
    layout.  Mirrors mh_plan_* of include/muahuff.h."""

    def __init__(self, ch_off, ch_len, S, h, mode, window, sclv, seg_chunks=0, input_bits=8, chunk_stride=0):
        """seg_chunks: chunks per segment; 0 = the planner's choice (info.seg_chunks tells).
        input_bits: 8 = one byte per sample; 4 / 2 = the packed pieces mh_deinterleave_packed writes
        (ch_off then counts bytes of the packed buffer; whole-channel window, preset encode only);
        chunk_stride != 0: that buffer is chunk-blocked (include/muahuff.h, mh_plan_create_packed)."""
        _need_gpu()
        self.ch_off = np.ascontiguousarray(ch_off, dtype=np.uint64)
        self.ch_len = np.ascontiguousarray(ch_len, dtype=np.uint64)
        self.sclv = np.ascontiguousarray(np.asarray(sclv, dtype=np.uint8).reshape(-1, int(S)))
        self.device = torch.device("cuda", torch.cuda.current_device())
        h_ = ct.c_void_p()
        self.input_bits = int(input_bits)
        rc = _lib.lib().mh_plan_create_packed(ct.byref(h_), self.ch_off.ctypes.data, self.ch_len.ctypes.data,
                                              len(self.ch_len), int(S), int(h), int(mode), int(window),
                                              self.sclv.ctypes.data, self.sclv.shape[0], int(seg_chunks),
                                              self.input_bits, int(chunk_stride))
        self.chunk_stride = int(chunk_stride)
        if rc == _lib.ERR_EMPTY_CHANNEL:
            # the reference fails the same way: functions_1.py:45 indexes data_in[0]
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        _lib.check(rc)
        self._h = h_
        info = _lib.PlanInfo()
        _lib.check(_lib.lib().mh_plan_info(self._h, ct.byref(info)))
        self.info = info
        self.C, self.S = int(info.C), int(info.S)
        self.seg_chunks = int(info.seg_chunks)
        self.n_segments = int(info.n_segments)
        self.payload_cap_words = int(info.payload_cap_words)
        self.window_samples = int(info.window_samples)
        self.max_len = int(self.ch_len.max()) if self.ch_len.size else 0

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().mh_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def segments(self):
        """Host copy of the segment directory."""
        n = self.n_segments
        d = dict(ch=np.zeros(n, np.uint32), first=np.zeros(n, np.uint64), n=np.zeros(n, np.uint64),
                 off=np.zeros(n, np.uint64))
        _lib.check(_lib.lib().mh_plan_segments(self._h, d["ch"].ctypes.data, d["first"].ctypes.data,
                                               d["n"].ctypes.data, d["off"].ctypes.data))
        return d

    # ---- device operations ------------------------------------------------------------
    def _z(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def measure(self, data, out=None):
        C, S = self.C, self.S
        m = out or Measured(self._z(C, torch.int64), self._z((C, S), torch.int32), self._z(C, torch.uint8),
                            self._z(C, torch.uint8), self._z((C, S), torch.int64), self._z(C, torch.int64),
                            self._z(C, torch.uint8))
        _lib.check(_lib.lib().mh_measure(self._h, _ptr(data), _ptr(m.cutoff), _ptr(m.cal_hist), _ptr(m.peak),
                                         _ptr(m.enc), _ptr(m.post_hist), _ptr(m.bits), _ptr(m.skipped),
                                         _stream()))
        return m

    def alloc_encoded(self):
        C = self.C
        return Encoded(torch.empty(self.payload_cap_words, dtype=torch.int32, device=self.device),
                       self._z(max(self.n_segments, 1), torch.int64), self._z(C, torch.int64),
                       self._z(C, torch.uint8), self._z(C, torch.uint8), self._z(C, torch.uint8))

    # ---- placement ---------------------------------------------------------------------
    # On this part the same kernel on the same data runs at one of two reproducible levels depending on WHICH physical
    # pages hold its buffers relative to each other (1024 ch x 1e7 bins: encode 2.03 or 2.19 ms, decode 1.95 or 2.02 ms;
    # six payload buffers alive at once, each keeps its level over repeated passes: profiles/r03_placement_levels.txt).
    # Nothing in a virtual address tells which it will be, so a long-lived buffer is worth choosing by measurement:
    # allocate a few candidates (all alive at once, so that they are different pages), time the real operation on
    # each, keep the fastest, free the rest.
    def alloc_encoded_probed(self, data, tries=4, reps=4):
        """alloc_encoded() chosen among `tries` candidates by the median time of `reps` encodes of `data` into each.
        -> (Encoded, [ms per candidate]).  The winner has been encoded into (its contents are a valid stream)."""
        cands = [self.alloc_encoded() for _ in range(max(1, int(tries)))]
        ms = [_median_ms(lambda e=e: self.encode(data, out=e), reps) for e in cands]
        best = int(np.argmin(ms))
        keep = cands[best]
        del cands
        return keep, ms

    def alloc_output_probed(self, enc, like, tries=3, reps=4):
        """A decode output buffer shaped like `like`, chosen among `tries` candidates by the median time of `reps`
        decodes of `enc` into each.  -> (tensor, [ms per candidate])"""
        cands = [torch.empty_like(like) for _ in range(max(1, int(tries)))]
        ms = [_median_ms(lambda o=o: self.decode(enc, o), reps) for o in cands]
        best = int(np.argmin(ms))
        keep = cands[best]
        del cands
        return keep, ms

    def encode(self, data, out=None, preset=None):
        """Calibrate + encode.  With preset=(peak, enc) (uint8 device tensors, one entry per
        channel) the calibration is skipped and that word is used instead (mh_encode_preset):
        the compression phase of a calibrate-then-stream protocol."""
        e = out or self.alloc_encoded()
        if preset is None:
            _lib.check(_lib.lib().mh_encode(self._h, _ptr(data), _ptr(e.payload), e.payload.numel(),
                                            _ptr(e.seg_words), _ptr(e.ch_bits), _ptr(e.peak), _ptr(e.enc),
                                            _ptr(e.skipped), _stream()))
        else:
            peak, enc = preset
            e.peak.copy_(peak)
            e.enc.copy_(enc)
            e.skipped.zero_()
            _lib.check(_lib.lib().mh_encode_preset(self._h, _ptr(data), _ptr(e.peak), _ptr(e.enc), _ptr(e.payload),
                                                   e.payload.numel(), _ptr(e.seg_words), _ptr(e.ch_bits), _stream()))
        return e

    def decode(self, enc, out):
        """out: uint8 tensor with the plan's channel layout; window bytes are overwritten.  The
        kernel never reads outside enc.payload whatever it holds (decode_ok() tells afterwards
        whether it had to abandon a segment)."""
        _lib.check(_lib.lib().mh_decode(self._h, _ptr(enc.payload), enc.payload.numel(), _ptr(enc.seg_off),
                                        _ptr(enc.peak), _ptr(enc.enc), _ptr(out), _stream()))
        return out

    def decode_packed(self, enc, out):
        """Packed plans (input_bits 2 for S <= 4, 4 for S >= 5): decode into the plan's packed pieces -- min(x, S-1) in the
        bit layout mh_deinterleave_packed writes (include/muahuff.h, mh_decode_packed).  out: uint8 tensor holding the
        plan's pieces; nothing outside them is written.  Same safety contract and status word as decode()."""
        _lib.check(_lib.lib().mh_decode_packed(self._h, _ptr(enc.payload), enc.payload.numel(), _ptr(enc.seg_off),
                                               _ptr(enc.peak), _ptr(enc.enc), _ptr(out), _stream()))
        return out

    def decode_range(self, payload, seg_off, peak, enc, sel, start, stop, out=None):
        """Random access in time (mh_decode_range): samples [start, stop) of the channels `sel` (indices, output rows in
        that order, repeats allowed; None = all) -> uint8 [len(sel), stop - start], row i = min(x, S-1) of channel sel[i]
        inside its window and 0 outside it and past its length.  payload: int32 words; seg_off: int64 [n_segments], where
        each segment starts in payload (only the entries of segments that overlap the range are read); peak / enc: uint8
        [C].  out: optional uint8 [len(sel), stop - start] tensor with unit stride along time (any row stride); without
        it the rows are placed so that sample t sits at a byte address congruent to t mod 128 (the decoder's interior row
        stores are then as aligned as mh_decode's) and a strided view is returned.  Not capturable into a graph: the work
        list is built on the host and uploaded (the call synchronises the current stream first)."""
        start, stop = int(start), int(stop)
        sel = query_args(self.max_len, self.C, start, stop, sel)
        sel32 = np.ascontiguousarray(sel, dtype=np.uint32)
        n, rows = stop - start, int(sel.size)
        if out is None:
            out = aligned_rows(rows, n, start, self.device)
        else:
            check_out(out, rows, n, torch.uint8, "time")
        pitch = out.stride(0) if rows > 1 else n
        _lib.check(_lib.lib().mh_decode_range(self._h, _ptr(payload), payload.numel(), _ptr(seg_off),
                                              sel32.ctypes.data if rows else None, rows, start, stop, _ptr(peak),
                                              _ptr(enc), _ptr(out) if rows and n else None, pitch, _stream()))
        return out

    def decode_rebin(self, payload, seg_off, peak, enc, sel, start, stop, r, saturate=True, out=None):
        """Decode straight to a coarser bin period (mh_decode_rebin): row i of decode_range(..., sel, start, stop) summed in
        bins of r samples, without the byte-per-sample rows ever being stored.  -> [len(sel), ceil((stop - start) / r)],
        uint8 = min(sum, 255) (saturate) or int32 exact sums; the last, partial bin is kept.  start must be a multiple of
        r, 1 <= r <= 4096.  out: optional tensor of that shape and dtype with unit stride along the bins.  Arguments
        otherwise as decode_range; not capturable into a graph."""
        start, stop, r = int(start), int(stop), int(r)
        sel = query_args(self.max_len, self.C, start, stop, sel, r)
        sel32 = np.ascontiguousarray(sel, dtype=np.uint32)
        nb, rows = (stop - start + r - 1) // r, int(sel.size)
        dtype = torch.uint8 if saturate else torch.int32
        if out is None:
            out = torch.empty((rows, nb), dtype=dtype, device=self.device)
        else:
            check_out(out, rows, nb, dtype, "the bins")
        pitch = out.stride(0) if rows > 1 else nb
        _lib.check(_lib.lib().mh_decode_rebin(self._h, _ptr(payload), payload.numel(), _ptr(seg_off),
                                              sel32.ctypes.data if rows else None, rows, start, stop, r, 1 if saturate else 0,
                                              _ptr(peak), _ptr(enc), _ptr(out) if rows and nb else None, pitch, _stream()))
        return out

    def decode_ok(self):
        """True when every decode() on this plan since the previous decode_ok() (direct calls and graph
        replays alike) stayed inside its payload; reading clears the flag (synchronises)."""
        flags = ct.c_uint32(0)
        _lib.check(_lib.lib().mh_decode_status(self._h, ct.byref(flags), _stream()))
        return flags.value == 0

    def compact(self, enc, dense=None, off=None, tot=None):
        """Pack the used words of all segments back to back (for storage / the RCCL gather).
        dense / off / tot: optional preallocated outputs (int32 words, int64 [n_segments], int64 [1]);
        with all three given the call enqueues kernels only."""
        if dense is None:
            total = int(enc.seg_words.sum().item())
            dense = torch.empty(total + 4, dtype=torch.int32, device=self.device)
        off = self._z(max(self.n_segments, 1), torch.int64) if off is None else off
        tot = self._z(1, torch.int64) if tot is None else tot
        _lib.check(_lib.lib().mh_compact(self._h, _ptr(enc.payload), _ptr(enc.seg_words), _ptr(dense),
                                         dense.numel(), _ptr(off), _ptr(tot), _stream()))
        return Encoded(dense, enc.seg_words, enc.ch_bits, enc.peak, enc.enc, enc.skipped, off, True), tot


def _median_ms(fn, reps):
    """median GPU time of fn() in ms (one warm-up call, then `reps` event-timed calls on the current stream)"""
    fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(1, int(reps)))]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def bit_rate(bits, n, BP):
    """BR = 1000/(BP/(bits/n)) in float64 in the reference's operation order
    (get_BR_with_approx_sort.py:289-292); 0/0 -> nan for skipped channels."""
    with np.errstate(invalid="ignore", divide="ignore"):
        abps = np.asarray(bits, dtype=np.float64) / np.asarray(n, dtype=np.float64)
        return np.float64(1000) / (np.float64(BP) / abps)
