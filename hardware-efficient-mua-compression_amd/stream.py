"""Calibrate-then-stream use of the codec on implant-style data.

The reference's RTL works in two phases (FPGA implementation/README.md:36-66): a CALIBRATION
phase fills, per channel, a RAM word {most frequent spike rate, selected encoder}
(RAM.v:4); in the COMPRESSION phase every later bin of every channel, arriving time-major
|CH1|CH2|...|CHN| per time step (README.md:31), is mapped and encoded with that fixed word.
`StreamEncoder` is the same protocol on the GPU: calibrate() on the first block, then
encode_block() on each later block -- de-interleave + encode with the preset word
(mh_encode_preset), no recalibration.  The channel-major intermediate between the two kernels
is PACKED: the encoder clips at S-1 anyway, so the de-interleaver writes min(x, 15) in 4 bits
per sample -- min(x, 3) in 2 bits when S <= 4 -- (mh_deinterleave_packed) and the encoder reads
those pieces directly; the intermediate's round trip through HBM shrinks from 2 x 1 byte per
sample to 2 x 1/2 resp. 2 x 1/4.
Firing rates drift, and a preset word goes stale.  encode_block_device(block, track=True) also measures the block's
packed pieces with a fresh calibration (mh_measure on a second packed plan with h = hist_bits: one more read of the
intermediate, nothing allocated, nothing synchronised); drift() tells per channel how many bits the stale word cost over
the fresh one, and adopt() takes the fresh word over on the device for the channels where that pays.
`StreamDecoder` is the receiving end of the same link: per block, the preset stream is decoded straight into packed
pieces of the same layout (mh_decode_packed) and re-interleaved to time-major bytes from them (mh_interleave_packed),
so the receive side skips the byte-per-sample intermediate as the send side does.
"""
import numpy as np
import torch

from . import MODE_APPROX, WIN_FULL, _lib, codec, container_io
from .codec import _ptr, _stream
from .container import ChannelSet


def _packed_layout(owner):
    """-> (bits per sample, bytes of one packed chunk) of the owner's blocks"""
    bits = 2 if owner.S <= 4 else 4
    return bits, 1024 * 2 * bits


def _packed_block(owner, Tb, slack=0):
    """The packed, chunk-blocked layout of a block of Tb time steps, the same on both ends of the link: min(x, S-1) in
    2 (S <= 4) or 4 bits per sample, chunk j (16384 samples = 1024 pieces) of channel c at (j * C + c) * cb -- the chunks
    of one time range are neighbours.  owner: a StreamEncoder or StreamDecoder.  -> (zeroed buffer of the pieces plus
    `slack` bytes, ch_off, plan); the buffer is allocated before the plan."""
    bits, cb = _packed_layout(owner)
    buf = torch.zeros((Tb + 16383) // 16384 * owner.C * cb + slack, dtype=torch.uint8, device=owner.device)
    ch_off = np.arange(owner.C, dtype=np.uint64) * np.uint64(cb)
    plan = codec.Plan(ch_off, np.full(owner.C, Tb, np.uint64), owner.S, 0, owner.mode, WIN_FULL, owner.sclv,
                      seg_chunks=owner.seg_chunks, input_bits=bits, chunk_stride=owner.C * cb)
    return buf, ch_off, plan


def _no_exact_events(exact):
    if exact:
        raise ValueError("exact=True is not available for blocks binned from events: the binner writes packed pieces of "
                         "min(count, S-1); bin to a time-major uint8 block and append that")


class StreamEncoder:
    def __init__(self, C, S, hist_bits, sclv, mode=MODE_APPROX, seg_chunks=2, device="cuda"):
        self.C, self.S, self.h, self.mode = int(C), int(S), int(hist_bits), int(mode)
        self.sclv = np.ascontiguousarray(np.asarray(sclv, dtype=np.uint8).reshape(-1, self.S))
        self.seg_chunks = int(seg_chunks)
        self.device = torch.device(device, torch.cuda.current_device()) if device == "cuda" else torch.device(device)
        self.peak = self.enc = None
        self._slots = {}

    def calibrate(self, block):
        """block: [T0, C] time-major counts holding at least 2^hist_bits time steps (fewer are
        accepted: the cutoff is min(2^h, T0), as functions_1.py:59-64).  Stores and returns the
        per-channel RAM word (peak, enc) as uint8 device tensors."""
        return self._calibrate(ChannelSet.from_time_major(block, device=self.device))

    def calibrate_events(self, ev, origin, period, T):
        """calibrate() on the T bins of `ev` (an events.EventSet) from `origin` at `period` ticks per bin: the counts
        are binned on the GPU (ChannelSet.from_events), no time-major block is built."""
        if ev.C != self.C:
            raise ValueError("event set has %d channels, encoder was built for %d" % (ev.C, self.C))
        return self._calibrate(ChannelSet.from_events(ev, origin, period, T))

    def _calibrate(self, cs):
        plan = codec.Plan(cs.ch_off, cs.ch_len, self.S, self.h, self.mode, WIN_FULL, self.sclv)
        m = plan.measure(cs.data)
        torch.cuda.synchronize()
        self.peak, self.enc = m.peak.clone(), m.enc.clone()
        plan.close()
        self.close()  # cached block plans point at the previous RAM word
        return self.peak, self.enc

    def _slot(self, Tb):
        """Plan and device buffers for blocks of Tb time steps, built once and reused: in the
        compression phase every block has the same shape, so nothing is planned or allocated
        per block."""
        slot = self._slots.get(Tb)
        if slot is None:
            buf, ch_off, plan = _packed_block(self, Tb, slack=16)
            cs = ChannelSet(buf, ch_off, np.full(self.C, Tb, np.uint64))
            e = plan.alloc_encoded()
            # the block's Encoded record points at the stored RAM word: nothing to copy per block
            e = codec.Encoded(e.payload, e.seg_words, e.ch_bits, self.peak, self.enc, e.skipped, e.seg_off, e.dense)
            slot = dict(cs=cs, plan=plan, enc=e,
                        d_off=torch.from_numpy(cs.ch_off.astype(np.int64)).to(self.device),
                        dense=torch.empty(plan.payload_cap_words, dtype=torch.int32, device=self.device),
                        off=torch.zeros(max(plan.n_segments, 1), dtype=torch.int64, device=self.device),
                        tot=torch.zeros(1, dtype=torch.int64, device=self.device))
            self._slots[Tb] = slot
        return slot

    def _monitor(self, slot):
        """The slot's monitor plan, built on first tracked use: a second packed plan over the same pieces and layout
        with h = hist_bits (the block plan has h = 0: it never calibrates), and the Measured record it fills."""
        if "monitor" not in slot:
            bits, cb = _packed_layout(self)
            cs = slot["cs"]
            slot["monitor"] = codec.Plan(cs.ch_off, cs.ch_len, self.S, self.h, self.mode, WIN_FULL, self.sclv,
                                         seg_chunks=self.seg_chunks, input_bits=bits, chunk_stride=self.C * cb)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
            slot["fresh"] = codec.Measured(z(self.C, torch.int64), z((self.C, self.S), torch.int32),
                                           z(self.C, torch.uint8), z(self.C, torch.uint8),
                                           z((self.C, self.S), torch.int64), z(self.C, torch.int64),
                                           z(self.C, torch.uint8))
        return slot["monitor"]

    def encode_block_device(self, block, track=False, checksum=False):
        """block: [Tb, C] time-major counts (device tensor or host array).  Enqueues
        de-interleave + preset encode + compaction on the current stream and returns
        (dense Encoded, total_words tensor, slot) without synchronising.
        checksum=True also enqueues, behind the compaction, the CRC-32 of every segment of the dense words
        (mhi_seg_crc32) into slot["crc"] (int32 [n_segments] holding the uint32 values), a slot buffer like the others.
        track=True also enqueues, behind the de-interleave and on the same stream, a measure of the block's packed
        pieces with a FRESH calibration (on the block's own first 2^hist_bits steps): slot["fresh"] is the
        codec.Measured of this block, overwritten per block like the other slot buffers -- see drift() and adopt().
        The block itself is always coded with the word in force when it was enqueued.  The buffers (dense
        words, sizes, total) belong to the shape's slot and are OVERWRITTEN by the next block of
        the same shape: a consumer that keeps a block in flight while the next one is enqueued
        (dist.gather_payload_pipelined) must copy them out -- or read the total and record an
        event -- before asking for the next block."""
        if self.peak is None:
            raise RuntimeError("calibrate() first")
        t = block if isinstance(block, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(block, np.uint8))
        t = t.to(self.device).contiguous()
        Tb, C = int(t.shape[0]), int(t.shape[1])
        if C != self.C:
            raise ValueError("block has %d channels, encoder was built for %d" % (C, self.C))
        slot = self._slot(Tb)
        cs, plan = slot["cs"], slot["plan"]
        _lib.check(_lib.lib().mh_deinterleave_packed(_ptr(t), Tb, C, plan.input_bits, _ptr(cs.data), _ptr(slot["d_off"]),
                                                     plan.chunk_stride, _stream()))
        return self._encode_slot(slot, track, checksum)

    def encode_events_device(self, ev, origin, period, T, track=False, checksum=False, exact=False):
        """encode_block_device for the block of T bins that `ev` (an events.EventSet) fills from `origin` at `period`
        ticks per bin: the slot's packed chunk-blocked pieces are written by the binner (mhi_bin_events, min(count, 3)
        in 2 bits for S <= 4, min(count, 15) in 4 bits for S >= 5) -- no time-major block, no de-interleave.  Everything
        behind the pieces is the block path's, and so is the stream, byte for byte."""
        from . import _ingest
        _no_exact_events(exact)
        if self.peak is None:
            raise RuntimeError("calibrate() first")
        if ev.C != self.C:
            raise ValueError("event set has %d channels, encoder was built for %d" % (ev.C, self.C))
        T = int(T)
        if T < 1:
            raise ValueError("T is at least 1 bin")
        slot = self._slot(T)
        cs, plan = slot["cs"], slot["plan"]
        _ingest.bin_events(ev, origin, period, T, plan.input_bits, cs.data, slot["d_off"], plan.chunk_stride)
        return self._encode_slot(slot, track, checksum)

    def _encode_slot(self, slot, track, checksum=False):
        """The block path behind the slot's packed pieces: optional drift measure, preset encode, compaction, optional
        segment checksums."""
        cs, plan = slot["cs"], slot["plan"]
        if track:
            self._monitor(slot).measure(cs.data, out=slot["fresh"])
        enc = slot["enc"]
        _lib.check(_lib.lib().mh_encode_preset(plan._h, _ptr(cs.data), _ptr(self.peak), _ptr(self.enc), _ptr(enc.payload),
                                               enc.payload.numel(), _ptr(enc.seg_words), _ptr(enc.ch_bits), _stream()))
        dense, tot = plan.compact(enc, dense=slot["dense"], off=slot["off"], tot=slot["tot"])
        if checksum:
            slot["crc"] = container_io.enqueue_seg_crc(plan, dense, out=slot.get("crc"))
        return dense, tot, slot

    def encode_block(self, block, checksum=False, exact=False):
        """block: [Tb, C] time-major counts -> container_io.Compressed covering all Tb bins of
        every channel, coded with the stored RAM word.  checksum=True: a revision-4 container with the segments'
        CRC-32 (taken on the device).  exact=True: the block also carries, as a sparse list, every count above S-1
        (excess.from_time_major: the COLS form of mhi_excess_count / mhi_excess_emit on the time-major block itself --
        the packed intermediate has already lost them -- with one read of the list's length between the two)."""
        t = block if isinstance(block, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(block, np.uint8))
        t = t.to(self.device).contiguous()
        c = self._finish_block(*self.encode_block_device(t, checksum=checksum), checksum=checksum, exact=exact)
        if exact:
            from . import excess
            exc_off, pos, val = excess.from_time_major(t, self.S - 1)
            container_io.attach_excess(c, exc_off.cpu().numpy(), pos.cpu().numpy().view(np.uint32), val.cpu().numpy())
        return c

    def _finish_block(self, dense, tot, slot, checksum=False, exact=False):
        plan = slot["plan"]
        torch.cuda.synchronize()
        hdr = container_io.make_header(self.S, 0, self.mode, WIN_FULL, plan.seg_chunks, self.sclv, checksum, exact)
        hdr["preset"] = True
        return container_io.Compressed.from_device(hdr, slot["cs"].ch_len, slot["enc"], plan.n_segments, dense.payload,
                                                   int(tot.item()), slot["crc"] if checksum else None)

    def encode_events(self, ev, origin, period, T, checksum=False, exact=False):
        """encode_block for the T bins that `ev` fills from `origin` at `period` ticks per bin.  exact=True raises
        ValueError: the binner writes packed pieces, which have lost the counts above S-1."""
        _no_exact_events(exact)
        return self._finish_block(*self.encode_events_device(ev, origin, period, T, checksum=checksum), checksum=checksum)

    def drift(self, slot):
        """int64 device tensor [C]: the code bits the slot's last tracked block spent under the word it was coded with,
        minus what it would have cost under a word calibrated on its own first 2^hist_bits steps (enc.ch_bits -
        fresh.bits).  Positive = the stored word is stale for this channel; it can be negative, since a word from 2^h
        steps may lose to the stored one over the whole block.  Enqueued on the current stream, no synchronisation."""
        if "fresh" not in slot:
            raise RuntimeError("no tracked block in this slot: encode_block_device(block, track=True) first")
        return slot["enc"].ch_bits - slot["fresh"].bits

    def adopt(self, slot, min_excess_bits=1):
        """Take the fresh (peak, enc) of the slot's last tracked block over for every channel whose drift() is at least
        min_excess_bits, on the device and without synchronising; returns the boolean device mask [C] of those
        channels.  self.peak / self.enc are updated IN PLACE: every slot's Encoded record and every later
        mh_encode_preset read those tensors.  A block is always coded with the word in force when it was enqueued, so
        the new word applies from the next block on; encode_block() ships (peak, enc) with every block, and the
        decoder needs nothing new."""
        take = self.drift(slot) >= int(min_excess_bits)
        fresh = slot["fresh"]
        torch.where(take, fresh.peak, self.peak, out=self.peak)
        torch.where(take, fresh.enc, self.enc, out=self.enc)
        return take

    def close(self):
        for slot in self._slots.values():
            slot["plan"].close()
            if "monitor" in slot:
                slot["monitor"].close()
        self._slots = {}

    @staticmethod
    def decode_block(c, device="cuda"):
        """-> [Tb, C] time-major array of min(x, S-1) (decoded and re-interleaved on the GPU)."""
        cs = container_io.decompress(c, device=device)
        if cs.C == 0:
            return np.zeros((0, 0), np.uint8)
        return cs.to_time_major().cpu().numpy()


class StreamDecoder:
    """Receiving end of StreamEncoder: [Tb, C] time-major min(x, S-1) from the dense stream of a block.

    Per block: an exclusive scan of the segment sizes (skipped when the caller has the offsets, e.g. the `seg_off` of
    the compaction that StreamEncoder.encode_block_device ran), mh_decode_packed into a packed, chunk-blocked
    intermediate of 2 (S <= 4) or 4 bits per sample, then mh_interleave_packed to time-major bytes.  Plan and buffers
    are cached per block shape, so after the first block of a shape nothing is planned, allocated or synchronised."""

    def __init__(self, C, S, sclv, mode=MODE_APPROX, seg_chunks=2, device="cuda"):
        self.C, self.S, self.mode = int(C), int(S), int(mode)
        self.sclv = np.ascontiguousarray(np.asarray(sclv, dtype=np.uint8).reshape(-1, self.S))
        self.seg_chunks = int(seg_chunks)
        self.device = torch.device(device, torch.cuda.current_device()) if device == "cuda" else torch.device(device)
        self._slots = {}

    def _slot(self, Tb):
        """Packed plan (same C, Tb, S, seg_chunks as the encoder's block plan: the segment boundaries match), pieces,
        segment offsets and the [Tb, C] output, built once per block shape."""
        slot = self._slots.get(Tb)
        if slot is None:
            pieces, ch_off, plan = _packed_block(self, Tb)
            slot = dict(plan=plan, pieces=pieces,
                        d_off=torch.from_numpy(ch_off.astype(np.int64)).to(self.device),
                        seg_off=torch.zeros(max(plan.n_segments, 1), dtype=torch.int64, device=self.device),
                        out=torch.empty((Tb, self.C), dtype=torch.uint8, device=self.device))
            self._slots[Tb] = slot
        return slot

    def decode_block_device(self, payload, seg_words, peak, enc, Tb, seg_off=None):
        """Enqueues the decode of one block on the current stream and returns its [Tb, C] uint8 device tensor of
        min(x, S-1), without synchronising.  payload: int32 device words of the dense stream (readable to its end:
        payload_words = payload.numel()); seg_words: int64 [n_segments] device sizes; peak / enc: uint8 [C] device RAM
        word; seg_off: optional int64 device segment offsets (else scanned from seg_words here).  The stream is not
        validated (the decoder never reads outside `payload`; ok() tells whether it had to abandon a segment).
        The returned tensor belongs to the shape's slot and is OVERWRITTEN by the next block of the same shape."""
        Tb = int(Tb)
        slot = self._slot(Tb)
        plan = slot["plan"]
        n = plan.n_segments
        if seg_words.numel() < n or (seg_off is not None and seg_off.numel() < n):
            raise ValueError("a block of %d steps has %d segments" % (Tb, n))
        if peak.numel() < self.C or enc.numel() < self.C:
            raise ValueError("the RAM word needs %d channels" % self.C)
        st = _stream()
        if seg_off is None:
            seg_off = slot["seg_off"]
            if n > 1:  # exclusive scan: seg_off[0] stays 0
                torch.cumsum(seg_words[:n - 1], 0, out=seg_off[1:n])
        _lib.check(_lib.lib().mh_decode_packed(plan._h, _ptr(payload), payload.numel(), _ptr(seg_off), _ptr(peak), _ptr(enc),
                                               _ptr(slot["pieces"]), st))
        out = slot["out"]
        _lib.check(_lib.lib().mh_interleave_packed(_ptr(slot["pieces"]), _ptr(slot["d_off"]), Tb, self.C, plan.input_bits,
                                                   plan.chunk_stride, _ptr(out), st))
        return out

    def ok(self):
        """True when no decode since the previous ok() had to abandon a segment (mh_decode_status over every slot's
        plan; synchronises, clears the flags)."""
        good = True
        for slot in self._slots.values():
            good = slot["plan"].decode_ok() and good
        return good

    def decode_block(self, c, check=True):
        """Checked host form: c = container_io.Compressed of one block as StreamEncoder.encode_block writes it ->
        [Tb, C] numpy array of min(x, S-1).  Raises ValueError when the container does not belong to this decoder or,
        with check, its stream is corrupt (mh_validate_stream, as container_io.decompress) or -- for a block that
        carries checksums -- a segment does not match its CRC-32 (verified on the device next to the upload)."""
        container_io.check_block(c, self.C, self.S, self.mode, self.seg_chunks, self.sclv)
        if check:
            container_io.validate(c)
        Tb = int(c.ch_len[0])
        up = codec.upload_stream(self.device, c.payload, c.seg_words, c.peak, c.enc)
        out = self.decode_block_device(*up, Tb)
        plans = [slot["plan"] for slot in self._slots.values()]
        # the block's offsets are the slot's, scanned by decode_block_device in front of this on the same stream
        container_io.check_verified(container_io.enqueue_verify(c, up[0], self._slots[Tb]["seg_off"], c.seg_words, None,
                                                                check), plans)
        codec.check_decoded(plans)  # synchronises
        return out.cpu().numpy()

    def close(self):
        for slot in self._slots.values():
            slot["plan"].close()
        self._slots = {}
