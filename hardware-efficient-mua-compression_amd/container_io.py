"""Wire / file format of a compressed channel set (format revision 3; revision 2 is still read; revision 4 = revision 3
plus checksums, written on request), and the two calls that make the codec usable end to end: compress() and decompress().

The reference never serialises a bitstream; this container is the
build's own.  File layout (little-endian):

    b"MUAHUFF1" | u32 header_len | header (UTF-8 JSON) | arrays, each padded to 8 bytes:
        ch_len u64[C] | peak u8[C] | enc u8[C] | skipped u8[C] | ch_bits u64[C]
        | seg_words u64[n_segments] | payload u32[total_words]
    revision 4 (checksum=True) puts seg_crc u32[n_segments] between seg_words and payload: zlib's CRC-32 of each segment's
    stored words as little-endian bytes (0 for a segment of 0 words), taken on the device (mhi_seg_crc32) and checked there
    on read; its header also carries "checksum": "crc32" and "arrays_crc32", the CRC-32 of the bytes of ch_len .. seg_crc
    as written (padding included), checked on the host when the head is read.  The header JSON itself is not covered.
    exact=True (any revision; the header then carries "exact": true) puts three arrays BEHIND the payload:
        exc_seg u64[n_segments + 1] | exc_pos u32[n] | exc_val u8[n]
    the sparse list of what the clip at S-1 dropped (excess.py): entry e says sample exc_pos[e] of its channel held
    S-1 + exc_val[e]; channel-major, ascending in exc_pos, and exc_seg[s] is the first entry of directory segment s.
    Everything from ch_len through payload is byte for byte what the container without the option holds.  With
    checksums the header also carries "excess_crc32", the CRC-32 of the three arrays as written.

The header carries everything a decoder needs to rebuild the plan: format revision, chunk
geometry, S, h, mapper, window rule, seg_chunks and the K SCLV rows (the static codebooks).
Per channel the stream only needs (peak, enc) -- the 3+2-bit RAM word of the reference's RTL
(FPGA implementation/RAM.v:4) -- because codebooks are static and the symbol permutation is a
closed form of the calibration peak.  `payload` is the dense concatenation of all segments in
directory order (mh_compact); segment s starts at word sum(seg_words[:s]).
"""
import builtins
import io
import json
import os
import struct
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import excess

MAGIC = b"MUAHUFF1"
FORMAT_REVISION = 3          # written; revision 2 (no head segments, include/muahuff.h MH_WIN_REV2_SEGMENTS) is still read
CHECKSUM_REVISION = 4        # revision 3 with seg_crc and arrays_crc32; written only with checksum=True
READ_REVISIONS = (2, 3, 4)
WIN_REV2_SEGMENTS = 0x100


@dataclass
class Compressed:
    header: dict
    ch_len: np.ndarray     # uint64 [C]
    peak: np.ndarray       # uint8  [C]
    enc: np.ndarray        # uint8  [C]
    skipped: np.ndarray    # uint8  [C]
    ch_bits: np.ndarray    # uint64 [C]  exact code bits (== reference histogram . SCLV)
    seg_words: np.ndarray  # uint64 [n_segments]
    payload: np.ndarray    # uint32 [sum(seg_words)]
    seg_crc: np.ndarray = None  # uint32 [n_segments], revision 4 only: CRC-32 of each segment's stored words
    exc_seg: np.ndarray = None  # uint64 [n_segments + 1]  exact=True only: first list entry of each segment
    exc_pos: np.ndarray = None  # uint32 [n]               sample index inside the channel
    exc_val: np.ndarray = None  # uint8  [n]               x - (S-1)

    @property
    def payload_bits(self):
        return int(self.ch_bits.sum())

    @property
    def container_bits(self):
        return int(self.payload.size) * 32

    @property
    def excess_bits(self):
        """What exact=True costs: 40 bits per entry plus the segment index; 0 without the lists."""
        return 0 if self.exc_pos is None else excess.ENTRY_BITS * int(len(self.exc_pos)) + 64 * int(len(self.exc_seg))

    @property
    def payload_words(self):
        return int(self.payload.size)

    @property
    def excess_entries(self):
        return int(len(self.exc_pos))

    def read_words(self, first, n):
        return self.payload[first:first + n]

    def read_excess(self, first, n):
        return self.exc_pos[first:first + n], self.exc_val[first:first + n]

    def tobytes(self):
        buf = io.BytesIO()
        write(buf, self)
        return buf.getvalue()

    @classmethod
    def from_device(cls, header, ch_len, enc, n_segments, dense, total, seg_crc=None):
        """The host record of an encoded set: enc = the codec.Encoded the plan filled, dense = its compacted words
        (device int32), total = how many of them are used, seg_crc = their checksums (device int32 [n_segments], for a
        revision-4 header).  The caller has synchronised."""
        return cls(header, ch_len.copy(), enc.peak.cpu().numpy(), enc.enc.cpu().numpy(), enc.skipped.cpu().numpy(),
                   enc.ch_bits.cpu().numpy().astype(np.uint64), enc.seg_words.cpu().numpy().astype(np.uint64)[:n_segments],
                   dense[:total].cpu().numpy().view(np.uint32).copy(),
                   None if seg_crc is None else seg_crc[:n_segments].cpu().numpy().view(np.uint32).copy())


# the arrays behind the header, in file order (each padded to 8 bytes); the payload is the last
ARRAYS = (("ch_len", np.uint64), ("peak", np.uint8), ("enc", np.uint8), ("skipped", np.uint8), ("ch_bits", np.uint64),
          ("seg_words", np.uint64), ("payload", np.uint32))


SEG_CRC = ("seg_crc", np.uint32)   # revision 4: between seg_words and payload (ARRAYS stays what revision 3 holds)
EXCESS = excess.NAMES              # exact=True: exc_seg, exc_pos, exc_val behind the payload


def file_arrays(hd, have, reading=False):
    """The header rule, for writing and reading alike -> (name, dtype) of the arrays a container with header hd holds, in
    file order.  have: the names present (a Compressed's arrays) or listed (the sizes of a header that was read).  ValueError
    unless revision 4 <=> seg_crc, "exact": true <=> the three lists; reading: no other "exact", both => excess_crc32."""
    crc, exc = SEG_CRC[0] in have, [name in have for name, _ in EXCESS]
    if crc != (hd.get("format_revision") == CHECKSUM_REVISION):
        raise ValueError("container revision %r %s seg_crc" % (hd.get("format_revision"), "with" if crc else "without"))
    if any(exc) != all(exc) or all(exc) != (hd.get("exact") is True) or (reading and hd.get("exact", True) is not True):
        raise ValueError("container header says exact=%r %s the excess lists" % (hd.get("exact"), "with" if any(exc) else "without"))
    if reading and all(exc) and crc and not isinstance(hd.get("excess_crc32"), int):
        raise ValueError("corrupt container: checksums without excess_crc32")
    return ARRAYS[:-1] + ((SEG_CRC,) if crc else ()) + ARRAYS[-1:] + (EXCESS if all(exc) else ())


def _file_arrays(c):
    return file_arrays(c.header, [name for name, _ in ARRAYS + (SEG_CRC,) + EXCESS if getattr(c, name, None) is not None])


def crc32_padded(parts):
    """zlib's CRC-32 over arrays as written: parts = (an array's bytes, its padding to 8 -- None: the zeros of write())."""
    crc = 0
    for raw, pad in parts:
        crc = zlib.crc32(b"\0" * (-len(raw) % 8) if pad is None else pad, zlib.crc32(raw, crc))
    return crc


def _raw(c, name, dt):
    return np.ascontiguousarray(getattr(c, name), dtype=dt).reshape(-1).view(np.uint8)   # from where it lies: no copy


def _header_blob(c):
    hdr = dict(c.header)
    arrays = _file_arrays(c)
    hdr["sizes"] = {name: int(np.asarray(getattr(c, name)).size) for name, _ in arrays}
    if SEG_CRC in arrays:
        hdr["checksum"], hdr["arrays_crc32"] = "crc32", crc32_padded((_raw(c, name, dt), None) for name, dt in arrays[:arrays.index(ARRAYS[-1])])
        if EXCESS[0] in arrays:
            hdr["excess_crc32"] = excess.crc32(c.exc_seg, c.exc_pos, c.exc_val)
    return json.dumps(hdr, sort_keys=True).encode()


def nbytes(c):
    """The number of bytes write() emits for c (archive.py puts it in front of the block)."""
    sizes = [int(np.asarray(getattr(c, name)).size) * np.dtype(dt).itemsize for name, dt in _file_arrays(c)]
    return 12 + len(_header_blob(c)) + sum(n + (-n % 8) for n in sizes)


def write(f, c):
    blob = _header_blob(c)
    f.write(MAGIC + struct.pack("<I", len(blob)) + blob)
    for name, dt in _file_arrays(c):
        raw = _raw(c, name, dt)
        f.write(raw)
        f.write(b"\0" * (-raw.size % 8))


def word_offsets(seg_words):
    """int64 [n_segments + 1]: the first stored word of every directory entry, and the total behind the last."""
    return np.concatenate([[0], np.cumsum(seg_words)]).astype(np.int64)


def seg_crc_host(c):
    """The checksums of c's segments (a `Compressed` or a `ContainerFile`) with zlib, no GPU: uint32 [n_segments],
    zlib.crc32 of each segment's stored words as little-endian bytes, 0 for a segment of 0 words."""
    words = np.asarray(c.seg_words, np.uint64)
    off = word_offsets(words)
    if off[-1] > c.payload_words:
        raise ValueError("corrupt container: the directory points past the payload")
    pay = np.ascontiguousarray(c.read_words(0, int(off[-1])), "<u4")
    return np.array([zlib.crc32(pay[off[s]:off[s + 1]].tobytes()) if words[s] else 0 for s in range(len(words))], np.uint32)


def _read_arrays(read, skip, hdr, names, crc=False, whole=False):
    """The arrays `names`, in file order, through read(n) -> bytes; skip(n) passes over padding, with crc it is read (whole:
    and must be there) -> ({name: array}, bytes taken in the file, crc32_padded of them as written or None)"""
    out, used, parts = {}, 0, []
    for name, dt in names:
        size = int(hdr["sizes"][name]) * np.dtype(dt).itemsize
        raw = read(size)
        if len(raw) != size:
            raise ValueError("truncated container (%s)" % name)
        pad = (read if crc else skip)(-size % 8)
        if whole and len(pad) != -size % 8:
            raise ValueError("truncated container (%s)" % name)
        out[name] = np.frombuffer(raw, dtype=dt).copy()
        parts.append((raw, pad))
        used += size + (-size % 8)
    return out, used, crc32_padded(parts) if crc else None


def read_head(read, skip=None):
    """Everything in front of the payload, through read(n) -> bytes: magic, header length, header, revision check and
    every array of ARRAYS but the payload.  skip(n) passes over padding (default: read it).
    -> (header, {name: array}, bytes consumed: the payload starts that far behind the magic)"""
    if read(8) != MAGIC:
        raise ValueError("not a MUAHUFF1 container")
    (n,) = struct.unpack("<I", read(4))
    hdr = json.loads(read(n).decode())
    if hdr.get("format_revision") not in READ_REVISIONS:
        raise ValueError("unsupported container revision %r" % hdr.get("format_revision"))
    names = file_arrays(hdr, hdr["sizes"] if isinstance(hdr.get("sizes"), dict) else (), reading=True)
    has = SEG_CRC in names     # arrays_crc32 covers the padding as written: read, not skipped
    arrays, size, crc = _read_arrays(read, read if skip is None else skip, hdr, names[:names.index(ARRAYS[-1])], crc=has)
    if has and (hdr.get("checksum") != "crc32" or hdr.get("arrays_crc32") != crc):
        raise ValueError("corrupt container: checksum of the arrays in front of the payload does not match")
    return hdr, arrays, 12 + n + size


def read_excess(read, hdr):
    """The three arrays behind the payload through read(n) -> bytes, excess_crc32 checked when the header has one -> {name: array}"""
    out, _size, crc = _read_arrays(read, None, hdr, EXCESS, crc=True, whole=True)
    if "excess_crc32" in hdr and hdr["excess_crc32"] != crc:
        raise ValueError("corrupt container: checksum of the excess lists does not match")
    return out


def read(f):
    hdr, arrays, _pos = read_head(f.read)
    arrays.update(_read_arrays(f.read, f.read, hdr, ARRAYS[-1:])[0])
    if hdr.get("exact"):
        arrays.update(read_excess(f.read, hdr))
        c = Compressed(hdr, **arrays)
        if len(c.exc_pos) != len(c.exc_val):
            raise ValueError("corrupt container: exc_pos and exc_val differ in length")
        check_consistent(c, arrays=False)
        excess.check_container(c)
        return c
    return Compressed(hdr, **arrays)


def save(path, c):
    with builtins.open(path, "wb") as f:
        write(f, c)


def load(path):
    with builtins.open(path, "rb") as f:
        return read(f)


def make_header(S, h, mode, window, seg_chunks, sclv, checksum=False, exact=False):
    from . import _lib
    sclv = np.asarray(sclv, dtype=np.uint8).reshape(-1, int(S))
    return {**({"exact": True} if exact else {}), "format_revision": CHECKSUM_REVISION if checksum else FORMAT_REVISION, "piece": _lib.PIECE, "lanes": _lib.LANES, "rows": _lib.ROWS,
            "S": int(S), "h": int(h), "mode": int(mode), "window": int(window), "seg_chunks": int(seg_chunks),
            "K": int(sclv.shape[0]), "sclv": [[int(v) for v in r] for r in sclv]}


# ---- GPU end-to-end ----------------------------------------------------------------------------
def attach_excess(c, exc_off, pos, val):
    """Give the `Compressed` c (header with "exact": true) its lists: (exc_off [C + 1], pos, val) is the channel-major list
    of its channels (host arrays); the segment index is made here from the directory."""
    ch, lo, _hi = Directory.of(c).bounds()
    c.exc_pos = np.ascontiguousarray(pos, np.uint32)
    c.exc_val = np.ascontiguousarray(val, np.uint8)
    c.exc_seg = excess.segment_index(exc_off, c.exc_pos, ch, lo)
    return c


def compress(cs, S, h, mode, sclv, window=None, seg_chunks=0, checksum=False, exact=False):
    """Calibrate + encode every channel of a ChannelSet on the GPU and bring the dense stream to
    the host as a `Compressed`.  seg_chunks = 0: the planner's choice; the header records it.
    checksum=True: a revision-4 container -- the CRC-32 of every segment of the compacted payload is taken on the
    device (mhi_seg_crc32) and comes to the host with the other small arrays.
    exact=True: the container also keeps what the clip at S-1 drops -- every sample above S-1 inside a channel's encoded
    window, as a sparse list made on the device (mhi_excess_count / mhi_excess_emit, one more read of a count) -- so that
    decompress() returns the counts themselves.  Skipped channels get no entries.  The stream is unchanged; `excess_bits`
    is the price."""
    import torch

    from . import WIN_AFTER_CAL, codec
    window = WIN_AFTER_CAL if window is None else window
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, h, mode, window, sclv, seg_chunks=seg_chunks)
    enc = plan.encode(cs.data)
    dense, tot = plan.compact(enc)
    crc = enqueue_seg_crc(plan, dense) if checksum else None
    torch.cuda.synchronize()
    c = Compressed.from_device(make_header(S, h, mode, window, plan.seg_chunks, sclv, checksum, exact), cs.ch_len, enc,
                               plan.n_segments, dense.payload, int(tot.item()), crc)
    plan.close()
    if exact:
        w0, w1, _head, _nseg = channel_layout(cs.ch_len, h, window)
        w1 = np.where(c.skipped != 0, w0, w1)
        exc_off, pos, val = excess.from_rows(cs.data, cs.ch_off, w0, w1, int(cs.ch_len.max()) if cs.C else 1, int(S) - 1) \
            if cs.C else (torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8))
        attach_excess(c, exc_off.cpu().numpy(), pos.cpu().numpy().view(np.uint32), val.cpu().numpy())
    return c


def enqueue_seg_crc(plan, dense, out=None):
    """mhi_seg_crc32 over every segment of a compacted stream (dense: the codec.Encoded that Plan.compact returns, with
    its device offsets and sizes), on the current stream -> int32 device tensor [n_segments] holding the uint32 values."""
    return _enqueue_crc(dense.payload, dense.seg_off, dense.seg_words, plan.n_segments, out)


def _enqueue_crc(payload, seg_off, seg_words, n, out=None, payload_words=None):
    import torch

    from . import _ingest
    crc = torch.zeros(max(n, 1), dtype=torch.int32, device=payload.device) if out is None else out
    if n:
        _ingest.seg_crc32(payload, seg_off, seg_words, n, crc=crc, payload_words=payload_words)
    return crc


def seg_crc_device(c):
    """seg_crc_host's values from the current device: c's payload uploaded whole, mhi_seg_crc32 over every segment (synchronises)."""
    import torch

    from . import codec
    n, device = len(c.seg_words), torch.device("cuda", torch.cuda.current_device())
    pay, d_off, _pk, _en = codec.upload_stream(device, c.payload, word_offsets(c.seg_words)[:-1] if n else np.zeros(1, np.int64),
                                               c.peak, c.enc)
    words = torch.from_numpy(np.ascontiguousarray(c.seg_words, np.uint64).view(np.int64)).to(device)
    return _enqueue_crc(pay, d_off, words, n, payload_words=pay.numel() - 4)[:n].cpu().numpy().view(np.uint32)


def enqueue_verify(src, pay, d_off, seg_words, segs, check, expect=None):
    """The read side of the checksums, next to an upload: with `check` and a source that carries seg_crc, mhi_seg_crc32 in
    verify form over the uploaded segments -- pay (codec.upload_stream: four words of slack behind the payload), d_off
    and seg_words indexed by segment, segs: the uint64 directory entries that were uploaded (None: all) -- against the
    stored values (expect: those in the order of seg_words when it is not the source's).  On the current stream, no
    synchronisation.  -> the call's own `bad` tensor for check_verified, or None when nothing is verified."""
    import torch

    from . import _ingest
    stored = getattr(src, "seg_crc", None) if expect is None else expect
    if not check or stored is None:
        return None
    if len(stored) != len(seg_words):
        raise ValueError("corrupt container: %d checksums for %d segments" % (len(stored), len(seg_words)))
    if len(seg_words) == 0:
        return None
    dev = pay.device
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).view(np.int64 if dt == np.uint64 else np.int32)).to(dev)  # noqa: E731
    cached = getattr(src, "_dev_dir", None) if expect is None else None     # a ContainerFile keeps its directory there
    if cached is None or cached[0].device != dev:
        cached = (up(seg_words, np.uint64), up(stored, np.uint32))
        if expect is None and hasattr(src, "_dev_dir"):
            src._dev_dir = cached
    bad = _ingest.verify_state(dev)
    _ingest.seg_crc32(pay, d_off, cached[0], len(seg_words), seg_idx=None if segs is None else up(segs, np.uint64),
                      expect=cached[1], bad=bad, payload_words=pay.numel() - 4)
    return bad


def check_verified(bad, plans=(), what="container", where="", index=None):
    """Read one call's `bad` (synchronises; None: nothing was verified) where the decode status is read: ValueError
    naming the lowest mismatching segment (index: local -> directory entry, for a re-gathered selection); the plans'
    status words are read and cleared first, so that the error leaves none behind."""
    if bad is None:
        return
    n, first = (int(v) for v in bad.tolist())
    if n:
        from . import codec
        codec.check_decoded(plans, unwinding=True)
        if index is not None and 0 <= first < len(index):
            first = int(index[first])
        raise ValueError("corrupt %s: checksum of segment %d%s does not match its payload (%d of the segments read)"
                         % (what, first, where, n))


def plan_window(hd):
    """The `window` argument a plan for this container takes: the header's window rule, plus the flag that selects
    revision 2's segment directory when a revision-2 stream is read."""
    return int(hd["window"]) | (WIN_REV2_SEGMENTS if int(hd.get("format_revision", FORMAT_REVISION)) == 2 else 0)


def channel_layout(ch_len, h, window, seg_chunks=1, revision=FORMAT_REVISION):
    """The planner's layout of each channel, by arithmetic (include/muahuff.h) -> int64 arrays (w0, w1, head, nseg): the
    encoded window [w0, w1) in channel samples by the window rule; the samples of its head segment -- from revision 3 on
    a window of at least 16 chunks that starts off a multiple of 128 samples opens with a segment up to the next one,
    else 0 --; its number of directory entries: the head, then segments of seg_chunks chunks."""
    from . import CHUNK, WIN_AFTER_CAL, WIN_FULL, WIN_REF_HALF, WIN_REF_HALF_TRUNC
    T = np.asarray(ch_len, dtype=np.int64)
    c = np.minimum(np.int64(1) << int(h), T)
    e = c + T // 2
    if window == WIN_REF_HALF:
        n = np.where(e > T, 0, e - c)
    elif window == WIN_REF_HALF_TRUNC:
        n = np.minimum(e, T) - c
    elif window == WIN_AFTER_CAL:
        n = T - c
    elif window == WIN_FULL:
        n = T
    else:
        raise ValueError("unknown window rule %r" % (window,))
    w0 = np.zeros_like(T) if window == WIN_FULL else c
    seg = int(seg_chunks) * CHUNK
    head = np.zeros_like(T) if int(revision) == 2 else np.where((n >= 16 * CHUNK) & (w0 % 128 != 0), 128 - w0 % 128, 0)
    return w0, w0 + n, head, (n - head + seg - 1) // seg + (head > 0)


def segments_per_channel(ch_len, h, window, seg_chunks, revision=FORMAT_REVISION):
    """Number of directory entries of each channel (channel_layout)."""
    return channel_layout(ch_len, h, window, seg_chunks, revision)[3]


def window_bounds(ch_len, h, window):
    """(w0, w1): the encoded window [w0, w1) of each channel, in channel samples (channel_layout)."""
    return channel_layout(ch_len, h, window)[:2]


def window_lengths(ch_len, h, window):
    """Samples in the encoded window of each channel (channel_layout)."""
    return np.subtract(*window_bounds(ch_len, h, window)[::-1])


def _header_fields(hd):
    """The range checks of validate() on a container header -> (S, K, h, window, seg_chunks, mode, sclv [K, S])."""
    from . import _lib
    try:
        S, K, h, window, seg_chunks, mode = (int(hd[k]) for k in ("S", "K", "h", "window", "seg_chunks", "mode"))
        sclv = np.ascontiguousarray(np.array(hd["sclv"], np.int64).reshape(K, S))
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("container header: %r" % (e,))
    if (hd.get("piece"), hd.get("lanes"), hd.get("rows")) != (_lib.PIECE, _lib.LANES, _lib.ROWS):
        raise ValueError("container header: chunk geometry differs from this library's")
    if not (2 <= S <= 10) or not (1 <= K <= 255) or sclv.min() < 1 or sclv.max() > 9:
        raise ValueError("container header: S / K / code lengths out of range")
    if not (0 <= h <= 30) or not (0 <= window <= 3) or not (0 <= mode <= 1) or not (1 <= seg_chunks <= 0xFFFFFFFF // (_lib.PIECE * _lib.LANES * _lib.ROWS)):
        raise ValueError("container header: h / window / mode / seg_chunks out of range")
    return S, K, h, window, seg_chunks, mode, sclv


class Directory(namedtuple("Directory", "w0 w1 head nseg first seg")):
    """A container's directory layout, built once per query from (ch_len, header) by channel_layout: int64 w0, w1, head,
    nseg per channel; first [C + 1]: each channel's first entry (its segments are consecutive); seg: samples per segment."""
    __slots__ = ()

    @classmethod
    def build(cls, ch_len, h, window, seg_chunks, revision=FORMAT_REVISION):
        from . import CHUNK
        w0, w1, head, nseg = channel_layout(ch_len, h, window, seg_chunks, revision)
        return cls(w0, w1, head, nseg, np.concatenate([[0], np.cumsum(nseg)]).astype(np.int64), int(seg_chunks) * CHUNK)

    @classmethod
    def of(cls, src):
        return cls.build(src.ch_len, *(src.header[k] for k in ("h", "window", "seg_chunks")),
                         src.header.get("format_revision", FORMAT_REVISION))

    def range(self, start, stop):
        """-> int64 (first, end): entries first[c] .. end[c] - 1 hold samples [start, stop) of channel c (equal: none)."""
        base, head, seg = self.first[:-1], self.head, self.seg
        a = np.maximum(int(start), self.w0) - self.w0       # window samples [a, b)
        b = np.minimum(int(stop), self.w1) - self.w0
        hit = a < b     # index: the segment of window sample r within its channel
        index = lambda r: np.where(head > 0, np.where(r < head, 0, 1 + (r - head) // seg), r // seg)  # noqa: E731
        return np.where(hit, base + index(np.maximum(a, 0)), base), np.where(hit, base + index(np.maximum(b - 1, 0)) + 1, base)

    def bounds(self):
        """-> int64 arrays (channel, lo, hi) of every directory entry: its channel and its samples [lo, hi)."""
        nseg, seg = self.nseg, self.seg
        ch = np.repeat(np.arange(len(nseg), dtype=np.int64), nseg)
        j = np.arange(int(self.first[-1]), dtype=np.int64) - np.repeat(self.first[:-1], nseg)   # entry within its channel
        w0r, w1r, hd = self.w0[ch], self.w1[ch], self.head[ch]
        has = hd > 0
        lo = np.where(has, np.where(j == 0, w0r, w0r + hd + (j - 1) * seg), w0r + j * seg)
        hi = np.where(has & (j == 0), w0r + hd, np.minimum(lo + seg, w1r))
        return ch, lo, hi


def check_consistent(c, arrays=True, what="container", layout=None):
    """ValueError unless the per-channel arrays agree about the channel count (with `arrays`), no channel is empty and the
    directory has the entries the header's layout (a Directory the caller has, else made here) gives.  -> entries per channel"""
    C = len(c.ch_len)
    if arrays and not (len(c.peak) == len(c.enc) == len(c.skipped) == len(c.ch_bits) == C):
        raise ValueError("%s arrays disagree about the channel count" % what)
    if C and int(np.min(c.ch_len)) == 0:
        raise ValueError("%s holds an empty channel" % what)
    nseg = (Directory.of(c) if layout is None else layout).nseg
    if int(nseg.sum()) != len(c.seg_words) or (C == 0 and c.payload_words):
        raise ValueError("%s directory does not match its header" % what)
    return nseg


def check_block(c, C, S, mode, seg_chunks, sclv, what="container"):
    """ValueError unless c (a Compressed or a ContainerFile) is a block of the stream whose two ends were built with
    these parameters: (S, mode, seg_chunks), the whole-channel window, the SCLV rows, C channels of one length."""
    from . import WIN_FULL
    hd = c.header
    got = tuple(hd.get(k) for k in ("S", "mode", "window", "seg_chunks"))
    if tuple(-1 if v is None else int(v) for v in got) != (S, mode, WIN_FULL, seg_chunks):
        raise ValueError("%s (S, mode, window, seg_chunks) = %s is not the expected %s"
                         % (what, got, (S, mode, WIN_FULL, seg_chunks)))
    if np.asarray(hd.get("sclv"), np.int64).reshape(-1).tolist() != np.asarray(sclv, np.int64).reshape(-1).tolist():
        raise ValueError("%s SCLV rows are not the expected ones" % what)
    ch_len = np.asarray(c.ch_len, np.uint64)
    if len(ch_len) != C or ch_len.size == 0 or (ch_len != ch_len[0]).any():
        raise ValueError("%s does not hold %d channels of one length" % (what, C))


def validate(c):
    """Structural check of a container before it goes to the GPU.  The header fields are range-
    checked here; the walk over every chunk header of every segment -- header sizes, sub-stream
    lengths possible for the channel's code, chunk sizes adding up exactly to the directory and the
    payload -- is mh_validate_stream (host-only C, no GPU needed).  mh_decode itself never reads
    outside the payload it is given, so this check is about detecting corruption, not about
    memory safety.  Raises ValueError."""
    from . import _lib
    hd = c.header
    S, K, h, window, seg_chunks, mode, sclv = _header_fields(hd)
    if hd.get("format_revision") not in READ_REVISIONS:
        raise ValueError("container header: unsupported revision %r" % (hd.get("format_revision"),))
    C = len(c.ch_len)
    check_consistent(c)
    if C == 0:
        return
    ch_len = np.ascontiguousarray(c.ch_len, np.uint64)
    rows = np.ascontiguousarray(sclv, np.uint8)
    pay = np.ascontiguousarray(c.payload, np.uint32)
    segw = np.ascontiguousarray(c.seg_words, np.uint64)
    peak, enc = np.ascontiguousarray(c.peak, np.uint8), np.ascontiguousarray(c.enc, np.uint8)
    rc = _lib.lib().mh_validate_stream(ch_len.ctypes.data, C, S, h, mode, plan_window(hd), rows.ctypes.data, K, seg_chunks,
                                       pay.ctypes.data if pay.size else np.zeros(1, np.uint32).ctypes.data, pay.size,
                                       segw.ctypes.data if segw.size else np.zeros(1, np.uint64).ctypes.data, segw.size,
                                       peak.ctypes.data, enc.ctypes.data)
    if rc != 0:
        raise ValueError("corrupt container: " + _lib.lib().mh_last_error().decode(errors="replace"))


def wants_excess(src, exact, what="container"):
    """The exact= rule of every reader: None -> apply the lists when the source has them, False -> never, True ->
    ValueError when it has none.  -> bool: apply them"""
    has = src.header.get("exact") is True
    if exact is True and not has:
        raise ValueError("exact=True: this %s was written without the excess lists" % what)
    return has and exact is not False


def _apply_channel_set(cs, pos, val, fe, le):
    """mhi_excess_apply onto the rows of a ChannelSet: one call when the channels are equally spaced, else one per channel
    that has entries."""
    off, ln = cs.ch_off.astype(np.int64), cs.ch_len.astype(np.int64)
    pitch = np.diff(off)
    if len(off) == 1 or (pitch == pitch[0]).all():
        excess.apply(pos, val, fe, le, 0, int(ln.max()), 1, 0, cs.data, int(pitch[0]) if len(off) > 1 else 0, 1,
                     ptr=cs.data.data_ptr() + int(off[0]))
        return
    fd, ld = excess._i64(fe, pos.device), excess._i64(le, pos.device)
    for i in np.nonzero(np.asarray(le) > np.asarray(fe))[0]:
        excess.apply(pos, val, fd[i:i + 1], ld[i:i + 1], 0, int(ln[i]), 1, 0, cs.data, 0, 1, ptr=cs.data.data_ptr() + int(off[i]))


def decompress(c, device="cuda", channels=None, check=True, exact=None):
    """Inverse of compress(): a ChannelSet whose windows hold min(x, S-1) (bytes outside the
    encoded windows are zero).  channels: optional list of channel indices -- only their segments
    are uploaded and decoded (the directory gives random access per channel); the returned set
    holds them in the order given.  check=True runs validate() first (containers from disk are
    untrusted input for a kernel that follows their headers) and, when the container carries checksums, verifies every
    uploaded segment on the device (mhi_seg_crc32): ValueError names the first that does not match.
    exact: None = add the excess lists back when the container has them (then the windows hold x itself), False = do not
    read them (min(x, S-1), what the container without the lists gives), True = ValueError when it has none.  The lists
    are range-checked on the host with `check` and applied on the decode's stream, right behind it."""
    import torch

    from . import codec
    from .container import ChannelSet
    use = wants_excess(c, exact)
    if check:
        validate(c)
        if use:
            excess.check_container(c)
    hd = c.header
    layout = Directory.of(c)
    check_consistent(c, arrays=False, layout=layout)
    seg_words, payload, peak, enc, skipped, ch_bits, ch_len = (c.seg_words, c.payload, c.peak, c.enc, c.skipped,
                                                                c.ch_bits, c.ch_len)
    stored_crc, segs = getattr(c, "seg_crc", None), None
    if channels is not None:
        sel = codec.select_channels(len(c.ch_len), channels)
        first, off = layout.first, word_offsets(c.seg_words)        # channel -> first segment -> first word
        segs = np.concatenate([np.arange(first[i], first[i + 1]) for i in sel]) if sel.size else np.zeros(0, np.int64)
        payload = (np.concatenate([c.payload[off[s]:off[s + 1]] for s in segs]) if segs.size
                   else np.zeros(0, np.uint32))
        seg_words = c.seg_words[segs]
        if stored_crc is not None and len(stored_crc) == len(c.seg_words):
            stored_crc = stored_crc[segs]
        peak, enc, skipped, ch_bits, ch_len = c.peak[sel], c.enc[sel], c.skipped[sel], c.ch_bits[sel], c.ch_len[sel]
    cs = ChannelSet.empty([int(n) for n in ch_len], device=device)
    if len(ch_len) == 0:
        return cs
    plan = codec.Plan(cs.ch_off, cs.ch_len, hd["S"], hd["h"], hd["mode"], plan_window(hd),
                      np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])
    try:
        if plan.n_segments != len(seg_words):      # not for a header that validate() accepts: the arithmetic is the planner's
            raise ValueError("container header: the planner cuts these channels into %d segments, not %d"
                             % (plan.n_segments, len(seg_words)))
        dev = cs.data.device
        seg_off = word_offsets(seg_words)[:-1] if len(seg_words) else np.zeros(1, np.int64)
        pay, d_off, d_peak, d_enc = codec.upload_stream(dev, payload, seg_off, peak, enc)
        e = codec.Encoded(pay, torch.from_numpy(seg_words.astype(np.int64)).to(dev),
                          torch.from_numpy(ch_bits.astype(np.int64)).to(dev), d_peak, d_enc,
                          torch.from_numpy(np.ascontiguousarray(skipped)).to(dev), d_off, True)
        bad = enqueue_verify(c, pay, d_off, seg_words, None, check, expect=stored_crc)
        plan.decode(e, cs.data)
        if use and len(c.exc_pos):
            ch = np.arange(len(c.ch_len)) if channels is None else sel
            seg_e = np.asarray(c.exc_seg, np.uint64).astype(np.int64)
            _apply_channel_set(cs, *excess.upload(c.exc_pos, c.exc_val, dev), seg_e[layout.first[ch]], seg_e[layout.first[ch + 1]])
        check_verified(bad, [plan], index=segs)
        codec.check_decoded([plan])
    finally:
        plan.close()
    return cs


# ---- random access in time -----------------------------------------------------------------------
class ContainerFile:
    """A container on disk with its payload left there: open() reads the magic, the header and the per-channel and
    directory arrays, and remembers where the payload starts.  Same fields as `Compressed` but `payload` (seg_crc: None without checksums);
    read_words() fetches a run of payload words (seek + readinto).  `bytes_read` counts every byte read from the file,
    so that "a range query reads only what it needs" can be checked.  Caches one decode plan of the container's layout
    (decompress_range).  offset: the byte of the file where the container starts (a block inside an archive, archive.py)."""

    def __init__(self, path, offset=0):
        self.path = str(path)
        self.offset = int(offset)
        self.bytes_read = 0
        self._plan = None
        self.seg_crc = None     # revision 4: the stored checksums
        self._dev_dir = None    # (seg_words, seg_crc) on the device once a query has verified against them
        self._f = builtins.open(self.path, "rb")
        try:
            self._f.seek(self.offset)
            self._read_head(*read_head(self._read, lambda pad: self._f.seek(pad, 1)))
        except Exception:
            self._f.close()
            raise

    def _read(self, n):
        b = self._f.read(n)
        self.bytes_read += len(b)
        return b

    def _read_head(self, header, arrays, n):
        self.header = header
        for name, a in arrays.items():
            setattr(self, name, a)
        self.payload_offset = self.offset + n           # file offset of payload word 0
        self.payload_words = int(self.header["sizes"]["payload"])
        self.head_bytes = self.bytes_read               # what open() read
        self._exc_seg = None
        if self.header.get("exact"):                    # the lists stay on disk: only where they lie is worked out
            pad8 = lambda b: b + (-b % 8)  # noqa: E731
            sizes = self.header["sizes"]
            self.excess_entries = int(sizes["exc_pos"])
            if int(sizes["exc_val"]) != self.excess_entries:
                raise ValueError("corrupt container: exc_pos and exc_val differ in length")
            self._off_exc_seg = self.payload_offset + pad8(4 * self.payload_words)
            self._off_exc_pos = self._off_exc_seg + pad8(8 * int(sizes["exc_seg"]))
            self._off_exc_val = self._off_exc_pos + pad8(4 * self.excess_entries)

    def _read_at(self, at, count, dt, name):
        out = np.empty(int(count), dtype=dt)
        if count:
            self._f.seek(at)
            got = self._f.readinto(memoryview(out).cast("B"))
            self.bytes_read += got
            if got != out.nbytes:
                raise ValueError("truncated container (%s)" % name)
        return out

    @property
    def exc_seg(self):
        """The segment index of the excess lists (read on first use, checked: monotone, within the entries)."""
        if self._exc_seg is None:
            seg = self._read_at(self._off_exc_seg, int(self.header["sizes"]["exc_seg"]), np.uint64, "exc_seg")
            excess.check_index(seg, len(self.seg_words), self.excess_entries)
            self._exc_seg = seg
        return self._exc_seg

    def read_excess(self, first, n):
        """list entries [first, first + n) -> (exc_pos uint32, exc_val uint8) (ValueError past the end of the file)"""
        return (self._read_at(self._off_exc_pos + 4 * int(first), n, np.uint32, "exc_pos"),
                self._read_at(self._off_exc_val + int(first), n, np.uint8, "exc_val"))

    def verify_excess(self):
        """Read the three arrays whole and compare them with the header's excess_crc32 (a no-op without one) and with
        the directory (excess.check_container).  ValueError."""
        if not self.header.get("exact"):
            return
        self._f.seek(self._off_exc_seg)
        arrays = read_excess(self._read, self.header)
        c = Compressed(self.header, self.ch_len, self.peak, self.enc, self.skipped, self.ch_bits, self.seg_words, None,
                       self.seg_crc, **arrays)
        excess.check_container(c)

    def read_words(self, first, n):
        """payload words [first, first + n) as uint32 (ValueError past the end of the file)"""
        return self._read_at(self.payload_offset + 4 * int(first), n, np.uint32, "payload")

    def plan(self):
        """The cached decode plan of this container's layout (created on first use, on the current device)."""
        if self._plan is None:
            self._plan = _range_plan(self)
        return self._plan

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open(path, offset=0):  # noqa: A001  (shadows the builtin in this module only: save / load use builtins.open)
    """-> ContainerFile: header and directory read, payload left on disk."""
    return ContainerFile(path, offset)


def _range_plan(c):
    from . import codec
    hd = c.header
    return codec.Plan(np.zeros(len(c.ch_len), np.uint64), c.ch_len, hd["S"], hd["h"], hd["mode"], plan_window(hd),
                      np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])


def range_segments(ch_len, h, window, seg_chunks, start, stop, revision=FORMAT_REVISION):
    """Directory.range of these channels: the directory entries (first, end) that hold samples [start, stop) of each."""
    return Directory.build(ch_len, h, window, seg_chunks, revision).range(start, stop)


def gather_range(src, start, stop, sel, layout=None):
    """The payload a range query reads: for each distinct channel of `sel`, the one contiguous run of stored words of
    its segments that overlap [start, stop) (src.read_words: slices of a `Compressed`, seek + readinto for a
    `ContainerFile`), back to back.  layout: the source's Directory when the caller has it.  -> (payload uint32, seg_off
    uint64 [n_segments]: where each of those segments starts in it, 0 for the others; seg_idx uint64: their entries)."""
    first, end = (Directory.of(src) if layout is None else layout).range(start, stop)
    seg_words = np.ascontiguousarray(src.seg_words, np.uint64)
    dense = word_offsets(seg_words)         # segment -> first word in the stored payload
    # one contiguous run of payload words per selected channel (once per channel, whatever the repeats)
    runs, seg_off, idx, base = [], np.zeros(max(len(seg_words), 1), np.uint64), [], 0
    for c in np.unique(sel):
        s0, s1 = int(first[c]), int(end[c])
        if s0 == s1:
            continue
        w0_, w1_ = int(dense[s0]), int(dense[s1])
        if w1_ > src.payload_words:
            raise ValueError("corrupt container: the directory points past the payload")
        runs.append(src.read_words(w0_, w1_ - w0_))
        seg_off[s0:s1] = base + (dense[s0:s1] - w0_)
        idx.append(np.arange(s0, s1, dtype=np.uint64))
        base += w1_ - w0_
    payload = np.ascontiguousarray(np.concatenate(runs) if runs else np.zeros(0, np.uint32), np.uint32)
    segs = np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0, np.uint64))
    return payload, seg_off, segs


ExcessLists = namedtuple("ExcessLists", "pos val first last")   # row i of a query takes entries [first[i], last[i]) of (pos, val)


def gather_excess(src, start, stop, sel, check, what="container", layout=None):
    """The list entries a range query reads: for each distinct channel of `sel`, the one slice of entries of its segments
    that overlap [start, stop) (src.read_excess), back to back, next to the payload words gather_range reads.  With check
    the index and the slices are range-checked on the host (excess.check_index / check_entries) -- they are not CRC'd:
    excess_crc32 covers the arrays whole.  -> ExcessLists (pos uint32, val uint8, first, last)."""
    layout = Directory.of(src) if layout is None else layout
    s_first, s_end = layout.range(start, stop)
    seg_e = np.asarray(src.exc_seg, np.uint64).astype(np.int64)
    n = src.excess_entries
    if check:
        excess.check_index(seg_e, len(src.seg_words), n, what)
    e0, e1 = np.minimum(seg_e[s_first], n), np.minimum(seg_e[s_end], n)
    base = np.zeros(len(src.ch_len), np.int64)
    ps, vs, counts, segs, at = [], [], [], [], 0
    for c in np.unique(sel):
        a, b = int(e0[c]), int(e1[c])
        if b <= a:
            continue
        p, v = src.read_excess(a, b - a)
        ps.append(p), vs.append(v)
        base[c] = at - a
        at += b - a
        counts.append(np.diff(seg_e[int(s_first[c]):int(s_end[c]) + 1])), segs.append(np.arange(int(s_first[c]), int(s_end[c])))
    pos = np.concatenate(ps) if ps else np.zeros(0, np.uint32)
    val = np.concatenate(vs) if vs else np.zeros(0, np.uint8)
    if check and ps:
        _ch, lo, hi = layout.bounds()
        segs = np.concatenate(segs)
        excess.check_entries(pos, val, np.concatenate(counts), lo[segs], hi[segs], int(src.header["S"]) - 1, what)
    first, last = e0[sel] + base[sel], e1[sel] + base[sel]
    return ExcessLists(pos, val, first, np.maximum(last, first))


@dataclass
class Job:
    """What one source adds to one range query, from _range_job for _enqueue: rows `sel`, local samples [a, b); payload None: empty."""
    src: object                 # the `Compressed` or `ContainerFile`
    sel: np.ndarray
    a: int
    b: int
    payload: np.ndarray = None  # gather_range: the words, where each segment starts in them, the directory entries read
    seg_off: np.ndarray = None
    segs: np.ndarray = None
    peak: np.ndarray = None
    enc: np.ndarray = None
    lists: ExcessLists = None   # gather_excess, when the lists are applied
    block: int = None           # archive.Reader.read: the block's index, and its first column of the wide result
    g0: int = 0


def _range_job(src, start, stop, channels, check, r=None, use=False, what="container"):
    """The host side of a range query of a `Compressed` / `ContainerFile` -> Job: codec.query_args, ONE Directory for what
    follows, gather_range, with check mh_validate_segments on what it read and, with use, gather_excess."""
    from . import _lib, codec
    hd = src.header
    S, K, h, window, seg_chunks, mode, sclv = _header_fields(hd)
    ch_len = np.ascontiguousarray(src.ch_len, np.uint64)
    C = len(ch_len)
    job = Job(src, codec.query_args(int(ch_len.max()) if C else 0, C, start, stop, channels, r), start, stop)
    layout = Directory.of(src)
    check_consistent(src, arrays=check, layout=layout)
    if job.sel.size == 0 or stop == start:
        return job
    job.payload, job.seg_off, job.segs = gather_range(src, start, stop, job.sel, layout)
    job.peak, job.enc = np.ascontiguousarray(src.peak, np.uint8), np.ascontiguousarray(src.enc, np.uint8)
    if check:
        rows_, seg_words, pay, seg_off, segs = (np.ascontiguousarray(sclv, np.uint8), np.ascontiguousarray(src.seg_words, np.uint64),
                                                job.payload, job.seg_off, job.segs)
        rc = _lib.lib().mh_validate_segments(ch_len.ctypes.data, C, S, h, mode, plan_window(hd), rows_.ctypes.data, K,
                                             seg_chunks, pay.ctypes.data if pay.size else None, pay.size,
                                             seg_off.ctypes.data, seg_words.ctypes.data if seg_words.size else seg_off.ctypes.data,
                                             len(seg_words), segs.ctypes.data if segs.size else None, segs.size,
                                             job.peak.ctypes.data, job.enc.ctypes.data)
        if rc != 0:
            raise ValueError("corrupt container: " + _lib.lib().mh_last_error().decode(errors="replace"))
    if use:
        job.lists = gather_excess(src, start, stop, job.sel, check, what, layout)
    return job


def _enqueue(plan, job, check, decode, r=1, lead=0):
    """The device side of one job, on the current stream, no synchronisation: codec.upload_stream, with check enqueue_verify
    next to it, decode(plan, payload, seg_off, peak, enc) -> the tensor it decoded into, the job's list added onto that behind
    the decode (bins of r samples, `lead` leading ones).  -> (that tensor, the `bad` tensor for check_verified or None)"""
    from . import codec
    up = codec.upload_stream(plan.device, job.payload, job.seg_off, job.peak, job.enc)
    bad = enqueue_verify(job.src, up[0], up[1], job.src.seg_words, job.segs, check)
    out = decode(plan, *up)
    if job.lists is not None and len(job.lists.pos):
        excess.apply(*excess.upload(job.lists.pos, job.lists.val, plan.device), job.lists.first, job.lists.last, job.a, job.b,
                     r, lead, out)
    return out, bad


def _run(job, check, decode, r=1):
    """_enqueue on the source's plan (a `ContainerFile` keeps one, a `Compressed` gets one per call), then the two statuses."""
    from . import codec
    own = not isinstance(job.src, ContainerFile)
    plan = _range_plan(job.src) if own else job.src.plan()
    try:
        out, bad = _enqueue(plan, job, check, decode, r)
        check_verified(bad, [plan])
        codec.check_decoded([plan])
    finally:
        if own:
            plan.close()
    return out


def decompress_range(src, start, stop, channels=None, device="cuda", check=True, time_major=False, exact=None):
    """Samples [start, stop) of the selected channels of a `Compressed` or a `ContainerFile` (open()), reading and
    decoding only the segments that overlap the range.  -> uint8 device tensor [n_sel, stop - start] (row i = channel
    channels[i]: min(x, S-1) inside the channel's encoded window, 0 outside it and past its length -- exactly
    decompress(src, channels).to_channels()[i][start:stop], zero-extended), or [stop - start, n_sel] with
    time_major=True.  channels: None = all, else indices (rows in that order, repeats allowed).  check=True validates the
    header fields and the segments the query reads (mh_validate_segments) before anything reaches the GPU and, when the
    source carries checksums, verifies exactly those segments on the device next to their upload; a segment whose
    checksum does not match, or a decode that had to abandon one, raises ValueError as decompress() does.
    exact (None / False / True as decompress): with the lists the rows hold x itself; only the entries of the segments
    that are read are fetched (gather_excess), range-checked on the host with `check` and added on the decode's stream."""
    import torch

    from . import codec
    start, stop = int(start), int(stop)
    job = _range_job(src, start, stop, channels, check, use=wants_excess(src, exact))
    if job.payload is None:
        z = torch.zeros((int(job.sel.size), stop - start), dtype=torch.uint8, device=device)
        return z.t().contiguous() if time_major else z
    out = _run(job, check, lambda plan, *up: plan.decode_range(*up, job.sel, start, stop))
    return codec.to_time_major(out) if time_major else out


def decompress_binned(src, r, start=0, stop=None, channels=None, saturate=True, check=True, device="cuda", exact=None):
    """Samples [start, stop) of the selected channels summed in bins of r samples (mh_decode_rebin): what
    decompress_range(src, start, stop, channels) re-binned by r gives, decoded in one pass that never stores the
    byte-per-sample rows.  -> device tensor [n_sel, ceil((stop - start) / r)], uint8 = min(sum, 255) (saturate, the form
    ChannelSet.rebin has) or int32 exact sums; the last, partial bin is kept.  stop=None: the longest channel's length.
    ValueError for a bad r, start or range, IndexError for a bad channel (codec.query_args) -- before anything reaches
    the GPU; check and the status handling as decompress_range.  exact as decompress_range: with the lists the bins
    hold the sums of x itself (uint8: min(sum, 255), which is what adding the list with saturation to the clipped,
    saturated sum gives)."""
    import torch
    r, start = int(r), int(start)
    stop = (int(np.max(src.ch_len)) if len(src.ch_len) else 0) if stop is None else int(stop)
    job = _range_job(src, start, stop, channels, check, r, wants_excess(src, exact))
    if job.payload is None:
        return torch.zeros((int(job.sel.size), (stop - start + r - 1) // r), dtype=torch.uint8 if saturate else torch.int32,
                           device=device)
    return _run(job, check, lambda plan, *up: plan.decode_rebin(*up, job.sel, start, stop, r, saturate), r)


def decompress_windows(src, triggers, pre, post, channels=None, bin=None, reduce=None, moments=1, saturate=True,  # noqa: A002
                       check=True, exact=None, device="cuda", join=None, max_bytes=None):
    """archive.Reader.read_windows over decompress_range: the samples [triggers[k] - pre, triggers[k] + post) of the selected
    channels of a `Compressed`, a `ContainerFile` or a path (opened for the call), stacked [n, n_sel, nb] in the order of
    `triggers` or, with reduce="sum", summed over them (windows.psth's result; moments=2 adds the sum of squares).  A
    window lies inside [0, the longest channel's length); a shorter channel is zero past its end, as decompress_range
    has it.  bin, saturate, join and max_bytes as read_windows; check and exact as decompress_range, once per span.
    There is no CPU path: a host array is not a source."""
    from . import codec, windows
    if isinstance(src, (str, os.PathLike)):
        with open(src) as f:
            return decompress_windows(f, triggers, pre, post, channels, bin, reduce, moments, saturate, check, exact, device,
                                      join, max_bytes)
    if not hasattr(src, "ch_len"):
        raise ValueError("decompress_windows takes a Compressed, a ContainerFile or a path: there is no CPU path")
    T = int(np.max(src.ch_len)) if len(src.ch_len) else 0
    starts, W, r, nb = windows.window_args(triggers, pre, post, bin, reduce, moments, T)
    rows = int(codec.select_channels(len(src.ch_len), channels).size)

    def read_span(a, b, view):
        view.copy_(decompress_range(src, a, b, channels, device, check, exact=exact))
    return windows.read_windows(read_span, rows, starts, W, r, nb, reduce, moments, saturate, T,
                                windows.CHUNK if join is None else join, windows.MAX_BYTES if max_bytes is None else max_bytes,
                                device)


def bins(src, start=0, stop=None, channels=None, bin=None, check=True, exact=None, device="cuda", max_bytes=None):  # noqa: A002
    """archive.Reader.bins over decompress_range / decompress_binned: the whole bins of the samples [start, stop) of the
    selected channels of a `Compressed`, a `ContainerFile` or a path as a gram.BinSource.  A path is opened here and
    stays open until the source's close() (the source is a context manager).  stop=None: the longest channel's length;
    a shorter channel is zero past its end.  Only whole bins count, and with bin > 1 the operand is the saturated uint8
    bin, as read_gram says; check and exact as decompress_range, once per batch.  There is no CPU path: a host array is
    not a source."""
    from . import codec, gram
    close = None
    if isinstance(src, (str, os.PathLike)):
        src = open(src)
        close = src.close
    try:
        if not hasattr(src, "ch_len"):
            raise ValueError("a source of bins is a Compressed, a ContainerFile or a path: there is no CPU path")
        T = int(np.max(src.ch_len)) if len(src.ch_len) else 0
        start, r, n = gram.gram_args(start, T if stop is None else stop, bin, T)
        rows = int(codec.select_channels(len(src.ch_len), channels).size)
    except BaseException:
        if close is not None:
            close()
        raise

    def read_bins(b0, nb, view):
        a, b = start + b0 * r, start + (b0 + nb) * r
        if bin is None:
            view.copy_(decompress_range(src, a, b, channels, device, check, exact=exact))
        else:
            view.copy_(decompress_binned(src, r, a, b, channels, True, check, device, exact))
    return gram.BinSource(rows, n, device, max_bytes, read_bins, close)


def decompress_gram(src, start=0, stop=None, channels=None, bin=None, check=True, exact=None, device="cuda",  # noqa: A002
                    max_bytes=None, lag=0):
    """archive.Reader.read_gram over decompress_range / decompress_binned: the Gram matrix (gram.Gram: int64 products,
    row sums, n) of the samples [start, stop) of the selected channels of a `Compressed`, a `ContainerFile` or a path
    (opened for the call).  stop=None: the longest channel's length; a shorter channel is zero past its end.  Only whole
    bins count, and with bin > 1 the operand is the saturated uint8 bin, as read_gram says; check and exact as
    decompress_range, once per batch; lag as read_gram.  There is no CPU path: a host array is not a source."""
    from . import gram
    if not isinstance(src, (str, os.PathLike)) and not hasattr(src, "ch_len"):
        raise ValueError("decompress_gram takes a Compressed, a ContainerFile or a path: there is no CPU path")
    with bins(src, start, stop, channels, bin, check, exact, device, max_bytes) as b:
        return gram.source_gram(b, lag)
