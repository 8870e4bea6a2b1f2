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
import struct
import zlib
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


def _has_excess(c):
    """Does c carry the lists?  ValueError unless the header's "exact" and the three arrays agree."""
    have = [getattr(c, name, None) is not None for name, _ in EXCESS]
    if any(have) != all(have) or all(have) != (c.header.get("exact") is True):
        raise ValueError("container header says exact=%r %s the excess lists" % (c.header.get("exact"), "with" if any(have) else "without"))
    return all(have)


def _file_arrays(c):
    """(name, dtype) of the arrays c has in a file, in file order.  ValueError unless checksums and revision, and the
    header's "exact" and the lists, agree."""
    has = getattr(c, "seg_crc", None) is not None
    if has != (c.header.get("format_revision") == CHECKSUM_REVISION):
        raise ValueError("container revision %r %s seg_crc" % (c.header.get("format_revision"), "with" if has else "without"))
    return (ARRAYS[:-1] + (SEG_CRC,) + ARRAYS[-1:] if has else ARRAYS) + (EXCESS if _has_excess(c) else ())


def _raw(c, name, dt):
    return np.ascontiguousarray(getattr(c, name), dtype=dt).reshape(-1).view(np.uint8)   # from where it lies: no copy


def _header_blob(c):
    hdr = dict(c.header)
    arrays = _file_arrays(c)
    hdr["sizes"] = {name: int(np.asarray(getattr(c, name)).size) for name, _ in arrays}
    if SEG_CRC in arrays:
        crc = 0
        for name, dt in arrays[:arrays.index(ARRAYS[-1])]:
            raw = _raw(c, name, dt)
            crc = zlib.crc32(b"\0" * (-raw.size % 8), zlib.crc32(raw, crc))
        hdr["checksum"], hdr["arrays_crc32"] = "crc32", crc
        if EXCESS[0] in arrays:
            hdr["excess_crc32"] = excess.crc32(c.exc_seg, c.exc_pos, c.exc_val)
    return json.dumps(hdr, sort_keys=True).encode()


def nbytes(c):
    """The number of bytes write() emits for c (archive.py puts it in front of the block)."""
    n = 12 + len(_header_blob(c))
    for name, dt in _file_arrays(c):
        raw = int(np.asarray(getattr(c, name)).size) * np.dtype(dt).itemsize
        n += raw + (-raw % 8)
    return n


def write(f, c):
    blob = _header_blob(c)
    f.write(MAGIC)
    f.write(struct.pack("<I", len(blob)))
    f.write(blob)
    for name, dt in _file_arrays(c):
        raw = _raw(c, name, dt)
        f.write(raw)
        f.write(b"\0" * (-raw.size % 8))


def seg_crc_host(c):
    """The checksums of c's segments (a `Compressed` or a `ContainerFile`) with zlib, no GPU: uint32 [n_segments],
    zlib.crc32 of each segment's stored words as little-endian bytes, 0 for a segment of 0 words."""
    words = np.asarray(c.seg_words, np.uint64)
    off = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
    if off[-1] > _stored_words(c):
        raise ValueError("corrupt container: the directory points past the payload")
    pay = c.read_words(0, int(off[-1])) if isinstance(c, ContainerFile) else np.ascontiguousarray(c.payload, "<u4")
    return np.array([zlib.crc32(pay[off[s]:off[s + 1]].tobytes()) if words[s] else 0 for s in range(len(words))], np.uint32)


def _read_array(read, skip, hdr, name, dt):
    """-> (the array `name` of the container, the bytes it takes in the file with its padding)"""
    size = int(hdr["sizes"][name]) * np.dtype(dt).itemsize
    raw = read(size)
    if len(raw) != size:
        raise ValueError("truncated container (%s)" % name)
    skip(-size % 8)
    return np.frombuffer(raw, dtype=dt).copy(), size + (-size % 8)


def read_head(read, skip=None):
    """Everything in front of the payload, through read(n) -> bytes: magic, header length, header, revision check and
    every array of ARRAYS but the payload.  skip(n) passes over padding (default: read it).
    -> (header, {name: array}, bytes consumed: the payload starts that far behind the magic)"""
    skip = read if skip is None else skip
    if read(8) != MAGIC:
        raise ValueError("not a MUAHUFF1 container")
    (n,) = struct.unpack("<I", read(4))
    hdr = json.loads(read(n).decode())
    if hdr.get("format_revision") not in READ_REVISIONS:
        raise ValueError("unsupported container revision %r" % hdr.get("format_revision"))
    has = isinstance(hdr.get("sizes"), dict) and SEG_CRC[0] in hdr["sizes"]
    if has != (hdr["format_revision"] == CHECKSUM_REVISION):
        raise ValueError("container revision %d %s seg_crc" % (hdr["format_revision"], "with" if has else "without"))
    listed = [name in hdr["sizes"] for name, _ in EXCESS] if isinstance(hdr.get("sizes"), dict) else [False]
    if any(listed) != all(listed) or all(listed) != (hdr.get("exact") is True) or ("exact" in hdr and hdr["exact"] is not True):
        raise ValueError("container header says exact=%r %s the excess lists" % (hdr.get("exact"), "with" if any(listed) else "without"))
    if all(listed) and has and not isinstance(hdr.get("excess_crc32"), int):
        raise ValueError("corrupt container: checksums without excess_crc32")
    arrays, pos, crc = {}, 12 + n, 0
    for name, dt in ARRAYS[:-1] + ((SEG_CRC,) if has else ()):
        if has:     # arrays_crc32 covers the padding as written: read, not skipped
            arrays[name], size = _read_array(read, lambda pad: None, hdr, name, dt)
            pad = read(size - arrays[name].nbytes)
            crc = zlib.crc32(pad, zlib.crc32(arrays[name].view(np.uint8), crc))
        else:
            arrays[name], size = _read_array(read, skip, hdr, name, dt)
        pos += size
    if has and (hdr.get("checksum") != "crc32" or hdr.get("arrays_crc32") != crc):
        raise ValueError("corrupt container: checksum of the arrays in front of the payload does not match")
    return hdr, arrays, pos


def read_excess(read, hdr):
    """The three arrays behind the payload, through read(n) -> bytes, with excess_crc32 checked when the header has one.
    -> {name: array}"""
    out, crc = {}, 0
    for name, dt in EXCESS:
        out[name], size = _read_array(read, lambda pad: None, hdr, name, dt)
        pad = read(size - out[name].nbytes)
        if len(pad) != size - out[name].nbytes:
            raise ValueError("truncated container (%s)" % name)
        crc = zlib.crc32(pad, zlib.crc32(out[name].view(np.uint8), crc))
    if "excess_crc32" in hdr and hdr["excess_crc32"] != crc:
        raise ValueError("corrupt container: checksum of the excess lists does not match")
    return out


def read(f):
    hdr, arrays, _pos = read_head(f.read)
    arrays["payload"], _size = _read_array(f.read, f.read, hdr, *ARRAYS[-1])
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
    hd = c.header
    ch, lo, _hi = excess.segment_bounds(c.ch_len, hd["h"], hd["window"], hd["seg_chunks"], hd["format_revision"])
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
    import torch

    from . import _ingest
    crc = torch.zeros(max(plan.n_segments, 1), dtype=torch.int32, device=plan.device) if out is None else out
    if plan.n_segments:
        _ingest.seg_crc32(dense.payload, dense.seg_off, dense.seg_words, plan.n_segments, crc=crc)
    return crc


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
        if expect is None and isinstance(src, ContainerFile):
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


def window_lengths(ch_len, h, window):
    """Samples in the encoded window of each channel (the rules of include/muahuff.h)."""
    w0, w1, _head, _nseg = channel_layout(ch_len, h, window)
    return w1 - w0


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


def _stored_words(src):
    return int(src.payload_words if isinstance(src, ContainerFile) else src.payload.size)


def check_consistent(c, arrays=True, what="container"):
    """ValueError unless the per-channel arrays agree about the channel count (with `arrays`), no channel is empty and
    the directory has the entries the header's layout gives these lengths.  -> directory entries per channel"""
    hd = c.header
    C = len(c.ch_len)
    if arrays and not (len(c.peak) == len(c.enc) == len(c.skipped) == len(c.ch_bits) == C):
        raise ValueError("%s arrays disagree about the channel count" % what)
    if C and int(np.min(c.ch_len)) == 0:
        raise ValueError("%s holds an empty channel" % what)
    nseg = segments_per_channel(c.ch_len, hd["h"], hd["window"], hd["seg_chunks"], hd.get("format_revision", FORMAT_REVISION))
    if int(nseg.sum()) != len(c.seg_words) or (C == 0 and _stored_words(c)):
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
    nseg_ch = check_consistent(c, arrays=False)
    seg_words, payload, peak, enc, skipped, ch_bits, ch_len = (c.seg_words, c.payload, c.peak, c.enc, c.skipped,
                                                                c.ch_bits, c.ch_len)
    stored_crc, segs = getattr(c, "seg_crc", None), None
    if channels is not None:
        sel = codec.select_channels(len(c.ch_len), channels)
        first = np.concatenate([[0], np.cumsum(nseg_ch)]).astype(np.int64)       # channel -> first segment
        off = np.concatenate([[0], np.cumsum(c.seg_words)]).astype(np.int64)    # segment -> first word
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
        seg_off = np.concatenate([[0], np.cumsum(seg_words)[:-1]]).astype(np.int64) if len(seg_words) else np.zeros(1, np.int64)
        pay, d_off, d_peak, d_enc = codec.upload_stream(dev, payload, seg_off, peak, enc)
        e = codec.Encoded(pay, torch.from_numpy(seg_words.astype(np.int64)).to(dev),
                          torch.from_numpy(ch_bits.astype(np.int64)).to(dev), d_peak, d_enc,
                          torch.from_numpy(np.ascontiguousarray(skipped)).to(dev), d_off, True)
        bad = enqueue_verify(c, pay, d_off, seg_words, None, check, expect=stored_crc)
        plan.decode(e, cs.data)
        if use and len(c.exc_pos):
            first = np.concatenate([[0], np.cumsum(nseg_ch)]).astype(np.int64)
            ch = np.arange(len(c.ch_len)) if channels is None else sel
            seg_e = np.asarray(c.exc_seg, np.uint64).astype(np.int64)
            _apply_channel_set(cs, *excess.upload(c.exc_pos, c.exc_val, dev), seg_e[first[ch]], seg_e[first[ch + 1]])
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
            self._read_head()
        except Exception:
            self._f.close()
            raise

    def _read(self, n):
        b = self._f.read(n)
        self.bytes_read += len(b)
        return b

    def _read_head(self):
        self.header, arrays, n = read_head(self._read, lambda pad: self._f.seek(pad, 1))
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
        out = np.empty(int(n), dtype=np.uint32)
        if n:
            self._f.seek(self.payload_offset + 4 * int(first))
            got = self._f.readinto(memoryview(out).cast("B"))
            self.bytes_read += got
            if got != out.nbytes:
                raise ValueError("truncated container (payload)")
        return out

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


def window_bounds(ch_len, h, window):
    """(w0, w1): the encoded window [w0, w1) of each channel, in channel samples (include/muahuff.h)."""
    return channel_layout(ch_len, h, window)[:2]


def range_segments(ch_len, h, window, seg_chunks, start, stop, revision=FORMAT_REVISION):
    """Directory entries that hold samples [start, stop) of each channel, by arithmetic on the layout: int64 arrays
    (first, end) -- channel c's overlapping segments are entries first[c] .. end[c] - 1 (first == end: none, the range
    misses the channel's window).  A channel's segments are consecutive in the directory and in the payload."""
    from . import CHUNK
    w0, w1, head, nseg = channel_layout(ch_len, h, window, seg_chunks, revision)
    base = np.cumsum(nseg) - nseg
    seg = int(seg_chunks) * CHUNK
    a = np.maximum(int(start), w0) - w0                # window samples [a, b)
    b = np.minimum(int(stop), w1) - w0
    hit = a < b

    def index(r):  # segment of window sample r within its channel
        return np.where(head > 0, np.where(r < head, 0, 1 + (r - head) // seg), r // seg)
    first = np.where(hit, base + index(np.maximum(a, 0)), base)
    end = np.where(hit, base + index(np.maximum(b - 1, 0)) + 1, base)
    return first, end


def gather_range(src, start, stop, sel):
    """The payload a range query reads: for each distinct channel of `sel`, the one contiguous run of stored words of
    its segments that overlap [start, stop) (slices of a `Compressed`, seek + readinto for a `ContainerFile`), back to
    back.  -> (payload uint32, seg_off uint64 [n_segments]: where each of those segments starts in it -- 0 for the
    others --, seg_idx uint64: their directory entries)."""
    hd = src.header
    h, window, seg_chunks = int(hd["h"]), int(hd["window"]), int(hd["seg_chunks"])
    rev = int(hd.get("format_revision", FORMAT_REVISION))
    first, end = range_segments(src.ch_len, h, window, seg_chunks, start, stop, rev)
    seg_words = np.ascontiguousarray(src.seg_words, np.uint64)
    dense = np.concatenate([[0], np.cumsum(seg_words)]).astype(np.int64)  # segment -> first word in the stored payload
    stored_words = _stored_words(src)
    # one contiguous run of payload words per selected channel (once per channel, whatever the repeats)
    runs, seg_off, idx, base = [], np.zeros(max(len(seg_words), 1), np.uint64), [], 0
    for c in np.unique(sel):
        s0, s1 = int(first[c]), int(end[c])
        if s0 == s1:
            continue
        w0_, w1_ = int(dense[s0]), int(dense[s1])
        if w1_ > stored_words:
            raise ValueError("corrupt container: the directory points past the payload")
        runs.append(src.read_words(w0_, w1_ - w0_) if isinstance(src, ContainerFile) else src.payload[w0_:w1_])
        seg_off[s0:s1] = base + (dense[s0:s1] - w0_)
        idx.append(np.arange(s0, s1, dtype=np.uint64))
        base += w1_ - w0_
    payload = np.ascontiguousarray(np.concatenate(runs) if runs else np.zeros(0, np.uint32), np.uint32)
    segs = np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0, np.uint64))
    return payload, seg_off, segs


def _range_inputs(src, start, stop, channels, check, r=None):
    """What a range query of a `Compressed` / `ContainerFile` needs on the host: argument checks (codec.query_args), the
    payload of the segments that overlap [start, stop) (gather_range) and, with check, their validation
    (mh_validate_segments).  -> (sel, payload, seg_off, segs, peak, enc); segs: the directory entries whose words
    `payload` holds; payload is None when the query is empty (no channel or no sample)."""
    from . import _lib, codec
    hd = src.header
    S, K, h, window, seg_chunks, mode, sclv = _header_fields(hd)
    ch_len = np.ascontiguousarray(src.ch_len, np.uint64)
    C = len(ch_len)
    sel = codec.query_args(int(ch_len.max()) if C else 0, C, start, stop, channels, r)
    check_consistent(src, arrays=check)
    if sel.size == 0 or stop == start:
        return sel, None, None, None, None, None
    payload, seg_off, segs = gather_range(src, start, stop, sel)
    peak, enc = np.ascontiguousarray(src.peak, np.uint8), np.ascontiguousarray(src.enc, np.uint8)
    if check:
        rows_ = np.ascontiguousarray(sclv, np.uint8)
        seg_words = np.ascontiguousarray(src.seg_words, np.uint64)
        rc = _lib.lib().mh_validate_segments(ch_len.ctypes.data, C, S, h, mode, plan_window(hd), rows_.ctypes.data, K,
                                             seg_chunks, payload.ctypes.data if payload.size else None, payload.size,
                                             seg_off.ctypes.data, seg_words.ctypes.data if seg_words.size else seg_off.ctypes.data,
                                             len(seg_words), segs.ctypes.data if segs.size else None, segs.size,
                                             peak.ctypes.data, enc.ctypes.data)
        if rc != 0:
            raise ValueError("corrupt container: " + _lib.lib().mh_last_error().decode(errors="replace"))
    return sel, payload, seg_off, segs, peak, enc


def gather_excess(src, start, stop, sel, check, what="container"):
    """The list entries a range query reads: for each distinct channel of `sel`, the one slice of entries of its segments
    that overlap [start, stop), back to back, next to the payload words gather_range reads.  With check the slices are
    range-checked on the host (excess.check_index / check_entries) -- they are not CRC'd: excess_crc32 covers the arrays
    whole.  -> (pos uint32, val uint8, first, last): row i of the query takes entries [first[i], last[i]) of (pos, val)."""
    hd = src.header
    h, window, seg_chunks = int(hd["h"]), int(hd["window"]), int(hd["seg_chunks"])
    rev = int(hd.get("format_revision", FORMAT_REVISION))
    s_first, s_end = range_segments(src.ch_len, h, window, seg_chunks, start, stop, rev)
    seg_e = np.asarray(src.exc_seg, np.uint64).astype(np.int64)
    n = int(src.excess_entries if isinstance(src, ContainerFile) else len(src.exc_pos))
    if not isinstance(src, ContainerFile) and check:
        excess.check_index(seg_e, len(src.seg_words), n, what)
    e0, e1 = np.minimum(seg_e[s_first], n), np.minimum(seg_e[s_end], n)
    base = np.zeros(len(src.ch_len), np.int64)
    ps, vs, counts, segs, at = [], [], [], [], 0
    for c in np.unique(sel):
        a, b = int(e0[c]), int(e1[c])
        if b <= a:
            continue
        p, v = src.read_excess(a, b - a) if isinstance(src, ContainerFile) else (src.exc_pos[a:b], src.exc_val[a:b])
        ps.append(p), vs.append(v)
        base[c] = at - a
        at += b - a
        counts.append(np.diff(seg_e[int(s_first[c]):int(s_end[c]) + 1])), segs.append(np.arange(int(s_first[c]), int(s_end[c])))
    pos = np.concatenate(ps) if ps else np.zeros(0, np.uint32)
    val = np.concatenate(vs) if vs else np.zeros(0, np.uint8)
    if check and ps:
        _ch, lo, hi = excess.segment_bounds(src.ch_len, h, window, seg_chunks, rev)
        segs = np.concatenate(segs)
        excess.check_entries(pos, val, np.concatenate(counts), lo[segs], hi[segs], int(hd["S"]) - 1, what)
    first, last = e0[sel] + base[sel], e1[sel] + base[sel]
    return pos, val, first, np.maximum(last, first)


def _range_decode(src, payload, seg_off, segs, peak, enc, check, run):
    """run(plan, payload, seg_off, peak, enc) with the gathered payload on the plan's device, its segments verified
    next to the upload when the source carries checksums (enqueue_verify); ValueError when one does not match or the
    decode had to abandon a segment."""
    from . import codec
    own = not isinstance(src, ContainerFile)
    plan = _range_plan(src) if own else src.plan()
    try:
        up = codec.upload_stream(plan.device, payload, seg_off, peak, enc)
        bad = enqueue_verify(src, up[0], up[1], src.seg_words, segs, check)
        out = run(plan, *up)
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
    use = wants_excess(src, exact)
    sel, payload, seg_off, segs, peak, enc = _range_inputs(src, start, stop, channels, check)
    n, rows = stop - start, int(sel.size)
    if payload is None:
        z = torch.zeros((rows, n), dtype=torch.uint8, device=device)
        return z.t().contiguous() if time_major else z
    lists = gather_excess(src, start, stop, sel, check) if use else None

    def run(plan, pay, off, pk, en):
        out = plan.decode_range(pay, off, pk, en, sel, start, stop)
        if lists is not None and len(lists[0]):
            excess.apply(*excess.upload(lists[0], lists[1], out.device), lists[2], lists[3], start, stop, 1, 0, out)
        return out
    out = _range_decode(src, payload, seg_off, segs, peak, enc, check, run)
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
    use = wants_excess(src, exact)
    sel, payload, seg_off, segs, peak, enc = _range_inputs(src, start, stop, channels, check, r)
    nb, rows = (stop - start + r - 1) // r, int(sel.size)
    if payload is None:
        return torch.zeros((rows, nb), dtype=torch.uint8 if saturate else torch.int32, device=device)
    lists = gather_excess(src, start, stop, sel, check) if use else None

    def run(plan, pay, off, pk, en):
        out = plan.decode_rebin(pay, off, pk, en, sel, start, stop, r, saturate)
        if lists is not None and len(lists[0]):
            excess.apply(*excess.upload(lists[0], lists[1], out.device), lists[2], lists[3], start, stop, r, 0, out)
        return out
    return _range_decode(src, payload, seg_off, segs, peak, enc, check, run)
