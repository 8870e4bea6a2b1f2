"""Spike events in CSR form on the device, the input of the binner (include/muahuff_ingest.h, mhi_bin_events).

The reference's loaders hold ``spikes{chan}`` -- one vector of spike times per channel -- or a merged ``MUA_vec`` of
(time, channel) pairs, and bin them with histogram2 over FLOAT edges built by MATLAB's colon operator, whose last bin is
closed on both sides (Data/Load_and_bin_Sabes_store_as_mat_file.m:30-54).  Those float edges are deliberately NOT
reproduced here.  The interface is integer ticks, as in the reference's RTL (binner_f counts detections per BIN_PERIOD
clock ticks, FPGA implementation/1_binner_final.v:19-21): bin b of a channel counts the events with
origin + b*period <= tick < origin + (b+1)*period, every bin half-open.  ticks_from_seconds() is the one place where
seconds become ticks, by rounding to the nearest tick of the given clock."""
import numpy as np
import torch


def ticks_from_seconds(t, rate_hz):
    """np.rint(t * rate_hz) as uint64: spike times in seconds -> ticks of a clock of rate_hz."""
    return np.rint(np.asarray(t, dtype=np.float64) * float(rate_hz)).astype(np.uint64)


def _ticks_tensor(a, device):
    if isinstance(a, torch.Tensor):
        if a.dtype not in (torch.int64, torch.uint64):
            raise ValueError("ticks are 64-bit integers")
        return a.reshape(-1).contiguous().to(device)
    a = np.ascontiguousarray(a)
    if a.dtype.kind not in "ui":
        raise ValueError("ticks are integers (ticks_from_seconds converts times)")
    if a.dtype.kind == "i" and a.size and int(a.min()) < 0:
        raise ValueError("ticks are not negative")
    return torch.from_numpy(a.astype(np.uint64).view(np.int64).reshape(-1)).to(device)


class EventSet:
    """ticks: 64-bit device tensor, all channels' time stamps back to back (below 2^63); ev_off: C + 1 offsets into it,
    channel c owns ticks[ev_off[c]:ev_off[c+1]], non-decreasing.  check=True verifies the offsets on the host and the
    per-channel order on the device (one synchronising reduction) and raises ValueError."""

    def __init__(self, ticks, ev_off, check=True, device="cuda"):
        self.ticks = _ticks_tensor(ticks, device)
        if self.ticks.dtype == torch.uint64:
            self.ticks = self.ticks.view(torch.int64)
        off = ev_off.cpu().numpy() if isinstance(ev_off, torch.Tensor) else np.asarray(ev_off)
        off = np.ascontiguousarray(off).astype(np.uint64).reshape(-1)
        if off.size < 2:
            raise ValueError("ev_off has C + 1 entries, C >= 1")
        self.offsets = off                         # host copy
        self.ev_off = torch.from_numpy(off.view(np.int64).copy()).to(self.ticks.device)
        if check:
            n = int(self.ticks.numel())
            if int(off[0]) != 0 or int(off[-1]) != n or (np.diff(off.astype(np.int64)) < 0).any():
                raise ValueError("ev_off must rise from 0 to the number of ticks (%d)" % n)
            if n:
                if bool((self.ticks < 0).any()):
                    raise ValueError("a tick is 2^63 or more")
                if n > 1:
                    down = self.ticks[1:] < self.ticks[:-1]
                    starts = self.ev_off[1:-1]
                    starts = starts[(starts > 0) & (starts < n)]
                    down[starts - 1] = False       # a channel may begin below its predecessor's last tick
                    if bool(down.any()):
                        raise ValueError("the ticks of a channel are not in non-decreasing order")

    @property
    def C(self):
        return int(self.offsets.size) - 1

    @property
    def device(self):
        return self.ticks.device

    @classmethod
    def from_channels(cls, channels, check=True, device="cuda"):
        """channels: one array of integer ticks per channel (the loader's spikes{chan} after ticks_from_seconds)."""
        arrs = [np.ascontiguousarray(c).reshape(-1) for c in channels]
        for a in arrs:
            if a.size and a.dtype.kind not in "ui":
                raise ValueError("ticks are integers (ticks_from_seconds converts times)")
        off = np.zeros(len(arrs) + 1, np.uint64)
        off[1:] = np.cumsum([a.size for a in arrs])
        ticks = np.concatenate([a.astype(np.uint64) for a in arrs]) if arrs else np.zeros(0, np.uint64)
        return cls(ticks, off, check=check, device=device)

    @classmethod
    def from_aer(cls, ticks, channels, C, check=True, device="cuda"):
        """One merged list of (tick, channel) pairs in time order -- the MUA_vec of the loader -- stable-sorted by
        channel, so that the time order within each channel is kept.  Host arrays take the NumPy route and are uploaded;
        device tensors (64-bit ticks; 16- / 32-bit channels as they are, int64 channels narrowed on the device) are
        partitioned where they are by mhi_aer_to_csr, and only the C + 1 offsets come back to the host."""
        if isinstance(ticks, torch.Tensor) and ticks.is_cuda:
            return cls._from_aer_device(ticks, channels, C, check)
        ticks = np.ascontiguousarray(ticks).reshape(-1)
        ch = np.ascontiguousarray(channels).reshape(-1).astype(np.int64)
        if ticks.size != ch.size:
            raise ValueError("one channel per tick")
        if ch.size and (ch.min() < 0 or ch.max() >= int(C)):
            raise ValueError("channel index outside 0..%d" % (int(C) - 1))
        order = np.argsort(ch, kind="stable")
        off = np.zeros(int(C) + 1, np.uint64)
        off[1:] = np.cumsum(np.bincount(ch, minlength=int(C)))
        return cls(ticks[order], off, check=check, device=device)

    @classmethod
    def _from_aer_device(cls, ticks, channels, C, check):
        from . import _ingest
        C = int(C)
        if not (isinstance(channels, torch.Tensor) and channels.device == ticks.device):
            raise ValueError("ticks and channels are tensors of one device")
        if ticks.dtype not in (torch.int64, torch.uint64):
            raise ValueError("ticks are 64-bit integers")
        ticks, ch = ticks.reshape(-1).contiguous(), channels.reshape(-1).contiguous()
        if ticks.numel() != ch.numel():
            raise ValueError("one channel per tick")
        if ch.dtype == torch.int64:    # below 0 or at / above 2^31: -1, which no C reaches as an unsigned number
            ch = torch.where((ch < 0) | (ch > 0x7FFFFFFF), -1, ch).to(torch.int32)
        elif ch.dtype not in (torch.int16, torch.uint16, torch.int32, torch.uint32):
            raise ValueError("channels are 16-, 32- or 64-bit integers")
        n, dev = int(ticks.numel()), ticks.device
        with torch.cuda.device(dev):
            out = torch.empty(n, dtype=torch.int64, device=dev)
            meta = torch.empty(C + 2, dtype=torch.int64, device=dev)        # ev_off[0..C], dropped
            scratch = torch.empty(_ingest.aer_scratch_bytes(n, C), dtype=torch.uint8, device=dev)
            _ingest.aer_to_csr(ticks, ch, C, out, meta, meta[C + 1:], scratch)
            meta = meta.cpu().numpy()  # the one synchronisation: an EventSet keeps host offsets
        if int(meta[C + 1]):
            raise ValueError("channel index outside 0..%d" % (C - 1))
        return cls(out, meta[:C + 1].view(np.uint64), check=check, device=dev)

    @classmethod
    def from_counts(cls, x, origin=0, period=1, phase=0):
        """The inverse of ChannelSet.from_events: every bin b of channel c with count k gives k events at the tick
        origin + b*period + phase, expanded on the device (mhi_unbin_count / mhi_unbin_emit).  x: a container.ChannelSet whose
        channels have one length (ValueError otherwise, as matrix() raises), or a 2-D uint8 device tensor [channels, bins]
        with unit stride along its last axis and any row pitch or offset -- what decompress(..., start=, stop=) and
        archive.Reader.read return.  Host arrays are not taken: there is no CPU path.  -> EventSet (host offsets; the ticks
        are ordered by construction and are not checked again).  One synchronisation, for the number of events."""
        from . import _ingest
        if hasattr(x, "matrix") and hasattr(x, "ch_off"):
            x = x.matrix()
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise ValueError("from_counts takes a ChannelSet or a device tensor: there is no CPU path")
        if x.dtype != torch.uint8 or x.dim() != 2:
            raise ValueError("counts are a 2-D uint8 tensor [channels, bins]")
        rows, cols = int(x.shape[0]), int(x.shape[1])
        if rows < 1 or cols < 1:
            raise ValueError("at least one channel and one bin")
        if cols > 1 and x.stride(1) != 1:
            raise ValueError("the bins of a channel lie back to back (unit stride along the last axis)")
        if rows > 1 and x.stride(0) < 0:
            raise ValueError("the row pitch is not negative")
        origin, period, phase = _tick_args(origin, period, phase, cols)
        row_off = torch.arange(rows, dtype=torch.int64, device=x.device) * (int(x.stride(0)) if rows > 1 else 0)
        ticks, _ch, off = _unbin(_ingest.UNBIN_CSR, x, row_off, rows, cols, origin, period, phase)
        return cls(ticks, off, check=False, device=x.device)


def _tick_args(origin, period, phase, steps):
    origin, period, phase = int(origin), int(period), int(phase)
    if origin < 0 or period < 1 or not 0 <= phase < period:
        raise ValueError("origin >= 0, period >= 1 and 0 <= phase < period")
    if origin + (int(steps) - 1) * period + phase >= 1 << 63:
        raise ValueError("the largest tick reaches 2^63")
    return origin, period, phase


def _unbin(form, x, row_off, rows, cols, origin, period, phase, ch_dtype=None):
    """count, ONE read of the total, emit -> (ticks int64 [total], channels or None, ev_off host uint64 [rows + 1] or None)"""
    from . import _ingest
    dev = x.device
    with torch.cuda.device(dev):
        csr = form == _ingest.UNBIN_CSR
        meta = torch.zeros(rows + 3 if csr else 2, dtype=torch.int64, device=dev)   # [ev_off[0..rows],] total, over
        ev_off, total, over = (meta[:rows + 1] if csr else None), meta[-2:-1], meta[-1:]
        scratch = torch.empty(_ingest.unbin_scratch_bytes(form, rows, cols), dtype=torch.uint8, device=dev)
        _ingest.unbin_count(form, x, row_off, rows, cols, ev_off, total, scratch)
        host = meta.cpu().numpy()              # the one synchronisation: the output is sized by the total
        n = int(host[-2])
        ticks = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]      # a pointer also for an empty result
        ch = None if csr else torch.empty(max(n, 1), dtype=ch_dtype, device=dev)[:n]
        _ingest.unbin_emit(form, x, row_off, rows, cols, origin, period, phase, ticks, ch, over, scratch, capacity=n)
        lost = int(over.item())
        if lost:
            raise RuntimeError("the counts changed between the two passes: %d events had no place" % lost)
    return ticks, ch, (host[:rows + 1].view(np.uint64).copy() if csr else None)


def aer_from_counts(block, origin=0, period=1, phase=0, ch_dtype=torch.int32):
    """A time-major block of counts as one merged list of (tick, channel) pairs: element (t, c) with count k gives k pairs
    (origin + t*period + phase, c), in time order and in channel order within a tick -- input for EventSet.from_aer and
    archive.Writer.append_aer.  block: contiguous [T, C] uint8 device tensor.  ch_dtype: a 16- or 32-bit integer type
    (16 bits hold C <= 65536).  -> (ticks int64, channels).  One synchronisation, for the number of pairs."""
    from . import _ingest
    if not (isinstance(block, torch.Tensor) and block.is_cuda):
        raise ValueError("aer_from_counts takes a device tensor: there is no CPU path")
    if block.dtype != torch.uint8 or block.dim() != 2 or not block.is_contiguous():
        raise ValueError("counts are a contiguous 2-D uint8 tensor [time steps, channels]")
    if ch_dtype not in (torch.int16, torch.uint16, torch.int32, torch.uint32):
        raise ValueError("channels are 16- or 32-bit integers")
    rows, cols = int(block.shape[0]), int(block.shape[1])
    if rows < 1 or cols < 1:
        raise ValueError("at least one time step and one channel")
    if cols > (1 << 16) and ch_dtype in (torch.int16, torch.uint16):
        raise ValueError("%d channels do not fit 16 bits" % cols)
    origin, period, phase = _tick_args(origin, period, phase, rows)
    ticks, ch, _off = _unbin(_ingest.UNBIN_AER, block, None, rows, cols, origin, period, phase, ch_dtype)
    return ticks, ch


def aer_time_slice(ticks, t0, t1):
    """(i0, i1): the pairs of a time-ordered 64-bit tick tensor with t0 <= tick < t1 are ticks[i0:i1] -- how a long
    merged list is cut into blocks for EventSet.from_aer / archive.Writer.append_aer.  Ticks are below 2^63, as
    everywhere in an EventSet, and so are the bounds (0 <= t <= 2^63 - 1): anything else raises ValueError."""
    t = ticks.reshape(-1)
    if t.dtype == torch.uint64:
        t = t.view(torch.int64)
    elif t.dtype != torch.int64:
        raise ValueError("ticks are 64-bit integers")
    t0, t1 = int(t0), int(t1)
    if not (0 <= t0 < 1 << 63 and 0 <= t1 < 1 << 63):
        raise ValueError("the bounds of a time slice lie in 0 .. 2^63 - 1")
    if t.numel() and (int(t[-1]) < 0 or int(t[0]) < 0):   # time-ordered: the ends bound the rest
        raise ValueError("a tick is 2^63 or more")
    i = torch.searchsorted(t, torch.tensor([t0, t1], dtype=torch.int64, device=t.device))
    i0, i1 = i.tolist()
    return i0, max(i0, i1)
