"""Recording archive: the blocks of a stream appended to ONE file, any time range read back by global time.

A recorder calibrates on its first block and then codes block after block with the stored RAM word (stream.StreamEncoder);
this module keeps those blocks in one append-only file and answers "channels 3, 17, 40 from step a to step b at bins of r"
across them.  File layout (little-endian):

    b"MUAHARC1" | u32 header_len | header (UTF-8 JSON: archive_revision, C, S, mode, seg_chunks, hist_bits, K, sclv, meta)
    block records, back to back:
        b"MUAHBLK1" | u64 record_len (prefix included) | u64 t_first | u64 Tb | the container_io.write bytes of the block
    trailer, written by close():
        b"MUAHIDX1" | u64 n | n x (u64 offset of the block's container bytes, u64 container bytes, u64 t_first, u64 Tb)
        | u64 offset of the trailer | b"MUAHEND1"

A block is a complete container (container_io.read at its offset returns it, container_io.ContainerFile(path, offset)
reads it lazily) coded with the word it carries, so a reader needs nothing but the file.  A file without a valid trailer
-- the writer crashed, or the last record is cut short -- opens by walking the record prefixes; what follows the last
complete record is ignored and `truncated` is set.  open(path, "a") cuts that tail (and an old trailer) off and goes on
appending with the word of the last complete block.

Archive revision 2 (create(..., checksum=True)) is revision 1 with "checksum": "crc32" in the header and every block a
revision-4 container: the CRC-32 of each of its segments, taken on the device as the block is coded, verified there by
read() on exactly the segments a query uploads, and by verify() over the whole file.

create(..., exact=True) puts "exact": true into the header (the revision stays what it is) and makes every block an
exact container (container_io: exc_seg / exc_pos / exc_val behind the payload, the sparse list of the counts above S-1),
so that read() returns the counts themselves.  Plain blocks and exact blocks do not mix.
"""
import builtins
import json
import os
import struct
from collections import OrderedDict, namedtuple

import numpy as np

from . import MODE_APPROX, MODE_NOSORT, WIN_FULL
from . import container_io as cio

MAGIC, BLOCK_MAGIC, INDEX_MAGIC, END_MAGIC = b"MUAHARC1", b"MUAHBLK1", b"MUAHIDX1", b"MUAHEND1"
ARCHIVE_REVISION = 1                  # written by default
CHECKSUM_REVISION = 2                 # revision 1 whose blocks are revision-4 containers (checksum=True)
PREFIX = struct.Struct("<8sQQQ")      # block magic, record_len, t_first, Tb
ENTRY = struct.Struct("<QQQQ")        # offset, nbytes, t_first, Tb
OPEN_BLOCK_FILES = 16                 # block files a reader keeps open at once (one descriptor each)

Block = namedtuple("Block", "t_first Tb offset nbytes")  # offset / nbytes: the block's container bytes in the file


def is_archive(path):
    with builtins.open(path, "rb") as f:
        return f.read(8) == MAGIC


def block_ranges(t_first, Tb, start, stop):
    """Global samples [start, stop) over blocks i = [t_first[i], t_first[i] + Tb[i]) (ascending, back to back) ->
    [(i, a, b)]: block i holds the samples as its local [a, b), a < b; blocks the range misses are not listed."""
    t_first, Tb = np.asarray(t_first, np.int64), np.asarray(Tb, np.int64)
    start, stop = int(start), int(stop)
    if stop <= start or t_first.size == 0:
        return []
    end = t_first + Tb
    i0 = int(np.searchsorted(end, start, side="right"))      # first block that ends after start
    i1 = int(np.searchsorted(t_first, stop, side="left"))    # first block that begins at or after stop
    return [(i, max(start - int(t_first[i]), 0), min(stop, int(end[i])) - int(t_first[i])) for i in range(i0, i1)]


# ---- index ---------------------------------------------------------------------------------------
def _load(f, size):
    """Header and block index of an open archive -> (header, header_bytes, blocks, end of the last complete record,
    truncated, trailer_bytes, bytes read)."""
    f.seek(0)
    head = f.read(12)
    if len(head) != 12 or head[:8] != MAGIC:
        raise ValueError("not a MUAHARC1 archive")
    (n,) = struct.unpack("<I", head[8:])
    blob = f.read(n)
    if len(blob) != n:
        raise ValueError("truncated archive header")
    hdr = json.loads(blob.decode())
    if hdr.get("archive_revision") not in (ARCHIVE_REVISION, CHECKSUM_REVISION):
        raise ValueError("unsupported archive revision %r" % (hdr.get("archive_revision"),))
    if (hdr["archive_revision"] == CHECKSUM_REVISION) != (hdr.get("checksum") == "crc32") or hdr.get("checksum", "crc32") != "crc32":
        raise ValueError("archive revision %d with checksum %r" % (hdr["archive_revision"], hdr.get("checksum")))
    data0, nread = 12 + n, 12 + n
    # the trailer, when the back pointer leads to one whose entries chain from the header to itself
    if size >= data0 + 32:
        f.seek(size - 16)
        tail = f.read(16)
        nread += len(tail)
        idx = struct.unpack("<Q", tail[:8])[0]
        if tail[8:] == END_MAGIC and data0 <= idx <= size - 32:
            f.seek(idx)
            t = f.read(size - 16 - idx)
            nread += len(t)
            if t[:8] == INDEX_MAGIC and len(t) == 16 + ENTRY.size * struct.unpack("<Q", t[8:16])[0]:
                blocks, pos, T = [], data0, 0
                for k in range((len(t) - 16) // ENTRY.size):
                    off, nb, t0, Tb = ENTRY.unpack_from(t, 16 + k * ENTRY.size)
                    if off != pos + PREFIX.size or t0 != T or Tb < 1 or nb < 12:
                        break
                    blocks.append(Block(t0, Tb, off, nb))
                    pos, T = off + nb, T + Tb
                else:
                    if pos == idx:
                        return hdr, data0, blocks, pos, False, size - idx, nread
    # no trailer: walk the record prefixes
    blocks, pos, T = [], data0, 0
    while pos + PREFIX.size + 8 <= size:
        f.seek(pos)
        p = f.read(PREFIX.size + 8)
        nread += len(p)
        magic, rec, t0, Tb = PREFIX.unpack_from(p)
        if magic != BLOCK_MAGIC or p[PREFIX.size:] != cio.MAGIC or rec < PREFIX.size + 12 or pos + rec > size or t0 != T or Tb < 1:
            break
        blocks.append(Block(t0, Tb, pos + PREFIX.size, rec - PREFIX.size))
        pos, T = pos + rec, T + Tb
    return hdr, data0, blocks, pos, True, 0, nread


def _archive_fields(hdr):
    try:
        C, S, mode, sc, h = (int(hdr[k]) for k in ("C", "S", "mode", "seg_chunks", "hist_bits"))
        rows = np.ascontiguousarray(np.array(hdr["sclv"], np.uint8).reshape(-1, S))
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("archive header: %r" % (e,))
    if C < 1:
        raise ValueError("archive header: no channels")
    return C, S, mode, sc, h, rows


# ---- reader --------------------------------------------------------------------------------------
class _BlockFile(cio.ContainerFile):
    """One block of an archive as a lazily read container; the decode plan belongs to the archive (one per block
    length), so closing the block closes its descriptor only."""

    def __init__(self, reader, offset):
        self._reader = reader
        super().__init__(reader.path, offset)

    def plan(self):
        return self._reader._plan_for(self)

    def close(self):
        self._f.close()


class Reader:
    """archive.open(path): C, S, T (total steps), meta, truncated, checksum, blocks (Block tuples), block(i), words(),
    read(), read_windows(), verify()."""

    def __init__(self, path):
        self.path = str(path)
        self._f = builtins.open(self.path, "rb")
        try:
            size = os.fstat(self._f.fileno()).st_size
            (self.header, self.header_bytes, self.blocks, self._end, self.truncated, self.trailer_bytes,
             self._own_read) = _load(self._f, size)
            self.C, self.S, self.mode, self.seg_chunks, self.hist_bits, self.sclv = _archive_fields(self.header)
        except Exception:
            self._f.close()
            raise
        self.meta = self.header.get("meta", {})
        self.checksum = self.header.get("checksum") == "crc32"
        self.exact = self.header.get("exact") is True
        self.T = int(sum(b.Tb for b in self.blocks))
        self._t_first = np.array([b.t_first for b in self.blocks], np.int64)
        self._Tb = np.array([b.Tb for b in self.blocks], np.int64)
        self._files = OrderedDict()       # block index -> _BlockFile, least recently used first
        self._retired_read = 0
        self._plans = {}

    @property
    def bytes_read(self):
        """every byte read from the file so far: header, trailer or prefixes, block heads, payload words"""
        return self._own_read + self._retired_read + sum(b.bytes_read for b in self._files.values())

    def block(self, i):
        """-> container_io.Compressed of block i, read whole"""
        b = self.blocks[i]
        self._f.seek(b.offset)
        c = cio.read(self._f)
        self._own_read += b.nbytes
        return c

    def block_file(self, i):
        """-> block i as a container_io.ContainerFile (head read, payload left in the file); cached, at most
        OPEN_BLOCK_FILES stay open"""
        bf = self._files.pop(i, None)
        if bf is None:
            bf = _BlockFile(self, self.blocks[i].offset)
            while len(self._files) >= OPEN_BLOCK_FILES:
                _k, old = self._files.popitem(last=False)
                self._retired_read += old.bytes_read
                old.close()
        self._files[i] = bf
        return bf

    def words(self):
        """-> (peak, enc): uint8 [n_blocks, C], the word each block was coded with"""
        n = len(self.blocks)
        peak, enc = np.zeros((n, self.C), np.uint8), np.zeros((n, self.C), np.uint8)
        for i in range(n):
            bf = self.block_file(i)
            peak[i], enc[i] = bf.peak, bf.enc
        return peak, enc

    def _plan_for(self, bf):
        """one decode plan per distinct block length: segment boundaries depend on the lengths and seg_chunks only"""
        key = (int(bf.ch_len[0]), int(bf.header["h"]))
        if key not in self._plans:
            self._plans[key] = cio._range_plan(bf)
        return self._plans[key]

    def _checked_block_file(self, i):
        bf = self.block_file(i)
        b = self.blocks[i]
        _check_member(bf, self.C, self.S, self.mode, self.seg_chunks, self.sclv, payload_words=bf.payload_words,
                      checksum=self.checksum, exact=self.exact)
        if int(bf.ch_len[0]) != b.Tb:
            raise ValueError("corrupt archive: block %d holds %d steps, its record says %d" % (i, int(bf.ch_len[0]), b.Tb))
        return bf

    def read(self, start, stop, channels=None, bin=None, saturate=True, time_major=False, check=True, out=None,  # noqa: A002
             exact=None):
        """Global samples [start, stop) of the selected channels -> device tensor.
        bin=None: uint8 [n_sel, stop - start], row i = min(x, S-1) of channel channels[i] (None = all; any order,
        repeats allowed), or [stop - start, n_sel] with time_major.
        bin=r (1..4096, start % r == 0): element b of a row is the sum of the global samples [start + b*r, min(start +
        b*r + r, stop)) -- uint8 = min(sum, 255) (saturate) or int32 exact sums, [n_sel, ceil((stop - start) / r)]; a
        bin that straddles a block boundary is summed over both blocks and saturated after that.
        Only the blocks that overlap the range are opened, and of those only the segments of the selected channels that
        overlap it are read.  check=True validates those segments (mh_validate_segments) before anything is launched and,
        in an archive with checksums, verifies them on the device next to each block's upload (one counter per block,
        read where the decode status is read): ValueError names the block and the segment whose checksum does not match;
        a decode that had to abandon a segment raises ValueError.  out: optional tensor of the result's shape and dtype
        with unit stride along its last axis (not with time_major); the rows are written there and nothing else is.
        exact: None = in an archive written with exact=True every block's excess list is added back onto its columns of
        the result (mhi_excess_apply behind each block's decode, on the same stream), so that x stands where min(x, S-1)
        stood -- only the entries of the segments that are read are fetched, range-checked on the host with `check` (not
        CRC'd: excess_crc32 covers a block's lists whole, verify() checks it); False = the lists are not read; True =
        ValueError in an archive without them."""
        import torch

        from . import codec
        use = cio.wants_excess(self, exact, "archive")
        start, stop, r = int(start), int(stop), None if bin is None else int(bin)
        sel = codec.query_args(self.T, self.C, start, stop, channels, r)
        n, rows = stop - start, int(sel.size)
        cols = n if r is None else (n + r - 1) // r
        dtype = torch.uint8 if r is None or saturate else torch.int32
        if out is not None:
            if time_major:
                raise ValueError("out is not taken with time_major")
            codec.check_out(out, rows, cols, dtype, "its last axis")
        # host side first: every block's words gathered and validated before anything is launched
        jobs = []
        if rows and n:
            for i, a, b in block_ranges(self._t_first, self._Tb, start, stop):
                bf = self._checked_block_file(i)
                job = cio._range_job(bf, a, b, sel, check, use=use, what="archive block %d" % i)
                job.block, job.g0 = i, int(self._t_first[i]) + a - start
                jobs.append(job)
        if not jobs:
            z = torch.zeros((rows, cols), dtype=dtype, device="cuda") if out is None else out.zero_()
            return z.t().contiguous() if time_major else z
        plans, bads = [], []
        try:
            res = self._decode(torch, jobs, rows, n, cols, r, saturate, dtype, out, plans, bads, check)
        except BaseException:
            codec.check_decoded(plans, unwinding=True)      # every plan's flag is read and cleared all the same
            raise
        for i, bad in bads:                                 # synchronises
            cio.check_verified(bad, plans, "archive", " of block %d" % i)
        codec.check_decoded(plans, "archive")
        if not time_major:
            return res
        return codec.to_time_major(res) if r is None else res.t().contiguous()

    def read_windows(self, triggers, pre, post, channels=None, bin=None, reduce=None, moments=1, saturate=True,  # noqa: A002
                     check=True, exact=None, join=None, max_bytes=None):
        """The same window around many trigger times in one call: window k is the global samples [triggers[k] - pre,
        triggers[k] + post) of the selected channels (pre, post >= 0, pre + post >= 1; triggers: host integers in any
        order, repeats allowed; ValueError names a trigger whose window is not inside [0, T)).  bin=r (1..4096) sums each
        window in bins of r samples from ITS OWN first sample -- not on read()'s global grid; the last bin may be cut.
        reduce=None -> device tensor [n, n_sel, ceil((pre + post) / r)] in the order of `triggers`: uint8 = min(sum,
        255), or int32 sums with saturate=False.  reduce="sum" -> what windows.psth returns: the int32 sum over the
        triggers [n_sel, nb], and with moments=2 (sum, sumsq) with the int64 sum of the squared per-window bin values.
        windows.plan_spans joins the windows into spans -- a gap shorter than `join` samples (default: one chunk) is
        bridged -- and every span is read ONCE with read(a, b, channels, check=check, exact=exact) into its columns of a
        scratch matrix of at most max_bytes bytes (default windows.MAX_BYTES; more spans than fit are further batches):
        blocks, checksums, exact lists and the decode status are read()'s.  One mhi_windows per batch then cuts, bins and
        stacks or sums the windows on the device.  An empty trigger list gives an empty or zero result."""
        from . import codec, windows
        starts, W, r, nb = windows.window_args(triggers, pre, post, bin, reduce, moments, self.T)
        cio.wants_excess(self, exact, "archive")
        rows = int(codec.select_channels(self.C, channels).size)
        return windows.read_windows(lambda a, b, view: self.read(a, b, channels, check=check, exact=exact, out=view), rows,
                                    starts, W, r, nb, reduce, moments, saturate, self.T,
                                    windows.CHUNK if join is None else join, windows.MAX_BYTES if max_bytes is None else max_bytes)

    def bins(self, start, stop, channels=None, bin=None, check=True, exact=None, max_bytes=None):  # noqa: A002
        """The whole bins of the global samples [start, stop) of the selected channels as a gram.BinSource: what
        read_gram, wiener.stats_from, WienerFilter.predict_from, cascade.cross_validate_from and the Kalman filter's
        file routes walk in batches of at most max_bytes bytes (default windows.MAX_BYTES) without holding the decoded
        range.  The argument rules and the operand are read_gram's: n = (stop - start) // r bins, start % r == 0, and
        with r > 1 the saturated uint8 bin.  Every batch is one read(a, b, channels, bin=, check=check, exact=exact,
        out=): blocks, checksums, exact lists and the decode status are read()'s.  Nothing is read here."""
        from . import codec, gram
        start, r, n = gram.gram_args(start, stop, bin, self.T)
        cio.wants_excess(self, exact, "archive")
        rows = int(codec.select_channels(self.C, channels).size)

        def read_bins(b0, nb, view):
            self.read(start + b0 * r, start + (b0 + nb) * r, channels, bin=bin, check=check, exact=exact, out=view)
        return gram.BinSource(rows, n, "cuda", max_bytes, read_bins)

    def read_gram(self, start, stop, channels=None, bin=None, check=True, exact=None, max_bytes=None, lag=0):  # noqa: A002
        """The spike-count Gram matrix of the global samples [start, stop) of the selected channels, without holding the
        decoded range: -> gram.Gram with gram[i, j] = sum over the bins of x_i * x_j (int64, exact), the row sums and n,
        from which Gram.cov() and Gram.corr() follow.  bin=r (1..4096, start % r == 0) takes the products of the counts
        in bins of r samples.  Only WHOLE bins count: n = (stop - start) // r, and the samples behind the last whole bin
        are left out -- unlike a read, a cut bin would bias a covariance.  With r > 1 the operand is what read(...,
        bin=r, saturate=True) returns: uint8, a bin's sum clipped at 255, the reference's own dtype for binned MUA at
        every bin period it uses.  The range is walked in batches of whole bins of at most max_bytes bytes (default
        windows.MAX_BYTES); each is decoded with read(a, b, channels, bin=, check=check, exact=exact, out=) into one
        reused scratch matrix and added by one symmetric mhi_gram: blocks, checksums, exact lists and the decode status
        are read()'s.  lag: what gram.gram takes, an int >= 0 below n or a sequence of them, with the same result in
        every field; a batch then keeps the last max(lag) bins of the one before (gram.walk)."""
        from . import gram
        return gram.source_gram(self.bins(start, stop, channels, bin, check, exact, max_bytes), lag)

    def read_events(self, start, stop, channels=None, origin=0, period=1, phase=0, check=True, aer=False,  # noqa: A002
                    ch_dtype=None, exact=None):
        """Global samples [start, stop) of the selected channels as spike events on the recording's clock: sample t of a
        channel with count k gives k events at the tick origin + t*period + phase -- read(start, stop, channels,
        check=check) followed by events.EventSet.from_counts with the origin moved to origin + start*period, expanded on
        the device (mhi_unbin_count / mhi_unbin_emit).  An archive written with exact=True gives every event that went in
        (exact as read()); any other holds min(count, S-1) per bin and gives that many.  All of a bin's events get the
        bin's start + phase.
        -> events.EventSet whose channel k is channels[k] (None = all; any order, repeats allowed).
        aer=True: read(time_major=True) and events.aer_from_counts -> (ticks int64, channels): one merged list in time
        order; the channel numbers are the archive's (mapped through `channels` when a subset was selected; within a
        tick the pairs follow the order of `channels`).  ch_dtype: torch.int32 (default) or a 16-bit type."""
        import torch

        from . import codec, events
        start, stop = int(start), int(stop)
        sel = codec.query_args(self.T, self.C, start, stop, channels, None)
        origin, period, phase = events._tick_args(origin, period, phase, max(stop, 1))
        ch_dtype = torch.int32 if ch_dtype is None else ch_dtype
        if sel.size == 0:
            raise ValueError("read_events needs at least one channel")
        if stop == start:       # an empty range: no events
            none = torch.zeros(0, dtype=torch.int64, device="cuda")
            if aer:
                return none, torch.zeros(0, dtype=ch_dtype, device="cuda")
            return events.EventSet(none, np.zeros(int(sel.size) + 1, np.uint64), check=False)
        x = self.read(start, stop, channels, time_major=aer, check=check, exact=exact)
        if not aer:
            return events.EventSet.from_counts(x, origin + start * period, period, phase)
        ticks, ch = events.aer_from_counts(x.contiguous(), origin + start * period, period, phase, ch_dtype=ch_dtype)
        if channels is not None:
            ch = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int64)).to(ch.device)[ch.long()].to(ch_dtype)
        return ticks, ch

    def _decode(self, torch, jobs, rows, n, cols, r, saturate, dtype, out, plans, bads, check):
        """Enqueue the decode of every job into its columns of the wide result (out_pitch = the wide row stride); with
        check, the verification of each block's uploaded segments next to its upload: (block, counter) pairs in `bads`."""
        from . import codec

        def launch(job, decode, lead=0):
            plan = self._plan_for(job.src)
            if plan not in plans:
                plans.append(plan)
            _target, bad = cio._enqueue(plan, job, check, decode, 1 if r is None else r, lead)   # the list: into the block's columns
            if bad is not None:
                bads.append((job.block, bad))

        if r is None:
            if out is None:     # the first block's local sample t at a byte address congruent to t mod 128
                out = codec.aligned_rows(rows, n, jobs[0].a, "cuda")
            for j in jobs:
                launch(j, lambda plan, *up: plan.decode_range(*up, j.sel, j.a, j.b, out=out[:, j.g0:j.g0 + j.b - j.a]))
            return out
        # a block whose t_first - start is a multiple of r decodes straight to sums; every bin it touches begins in it
        aligned = [(j.g0 - j.a) % r == 0 for j in jobs]   # g0 - a == t_first - start: mh_decode_rebin's local rule holds
        summed = not all(aligned)    # all aligned: no bin has samples in two blocks either, each block writes its own bins;
        # otherwise exact int32 sums: aligned blocks write theirs (in time order, so before any later block adds to their
        # last, cut bin); the others are range-decoded behind g0 % r leading zeros and summed per bin on the device
        res = torch.zeros((rows, cols), dtype=torch.int32, device="cuda") if summed else \
            torch.empty((rows, cols), dtype=dtype, device="cuda") if out is None else out
        for j, al in zip(jobs, aligned):
            if al:
                launch(j, lambda plan, *up: plan.decode_rebin(*up, j.sel, j.a, j.b, r, saturate and not summed,
                                                              out=res[:, j.g0 // r:j.g0 // r + (j.b - j.a + r - 1) // r]))
            else:
                def edge(plan, *up):
                    lead = j.g0 % r
                    k = (lead + j.b - j.a + r - 1) // r
                    tmp = torch.zeros((rows, k * r), dtype=torch.uint8, device=plan.device)
                    plan.decode_range(*up, j.sel, j.a, j.b, out=tmp[:, lead:lead + j.b - j.a])
                    res[:, j.g0 // r:j.g0 // r + k] += tmp.view(rows, k, r).sum(dim=2, dtype=torch.int32)
                    return res[:, j.g0 // r:j.g0 // r + k]
                launch(j, edge, j.g0 % r)
        if not summed:
            return res
        res = res.clamp_(max=255).to(torch.uint8) if saturate else res
        return res if out is None else out.copy_(res)

    def verify(self, device=True):
        """Every segment of every block against its stored CRC-32, one block's payload at a time -> [(block, segment)]
        of the mismatches, in order; empty when the file is clean.  device=True: the payload is uploaded and
        mhi_seg_crc32 takes the checksums; device=False: zlib on the host, no GPU.  The arrays in front of each payload
        are checked as every read of a block's head checks them (ValueError).  ValueError on an archive without
        checksums."""
        if not self.checksum:
            raise ValueError("this archive carries no checksums (create(..., checksum=True) writes them)")
        bad = []
        for i in range(len(self.blocks)):
            c = self.block(i)      # read whole: an exact block's lists against excess_crc32 and the directory (ValueError)
            _check_member(c, self.C, self.S, self.mode, self.seg_chunks, self.sclv, checksum=True, exact=self.exact)
            got = cio.seg_crc_device(c) if device else cio.seg_crc_host(c)
            bad += [(i, int(s)) for s in np.nonzero(got != np.asarray(c.seg_crc, np.uint32))[0]]
        return bad

    def close(self):
        for p in self._plans.values():
            p.close()
        self._plans = {}
        for bf in self._files.values():
            self._retired_read += bf.bytes_read
            bf.close()
        self._files = OrderedDict()
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- writer --------------------------------------------------------------------------------------
def _check_member(c, C, S, mode, seg_chunks, sclv, payload_words=None, checksum=False, exact=False):
    """ValueError unless c (a Compressed or a ContainerFile) is a block of an archive with these parameters: the check
    StreamDecoder.decode_block makes, plus the array sizes the directory arithmetic relies on.  checksum: the archive's
    blocks are revision-4 containers, each with one checksum per segment.  exact: the archive's blocks carry the excess
    lists -- plain blocks and exact blocks do not mix."""
    hd = c.header
    if (hd.get("exact") is True) != bool(exact):
        raise ValueError("a block of an archive %s the excess lists carries %s" % (("with", "none") if exact else ("without", "them")))
    cio._header_fields(hd)
    cio.check_block(c, C, S, mode, seg_chunks, sclv, what="block")
    revision = cio.CHECKSUM_REVISION if checksum else cio.FORMAT_REVISION
    if int(hd.get("format_revision", -1)) != revision:
        raise ValueError("an archive block has container format revision %d" % revision)
    if checksum != (getattr(c, "seg_crc", None) is not None) or (checksum and len(c.seg_crc) != len(c.seg_words)):
        raise ValueError("a block of an archive %s checksums carries %s" % (("with", "none") if checksum else ("without", "them")))
    cio.check_consistent(c, what="block")
    words = int(c.payload.size) if payload_words is None else int(payload_words)
    if int(np.asarray(c.seg_words, np.uint64).sum()) != words:
        raise ValueError("block directory does not match its payload")


class Writer:
    """archive.create(...) / archive.open(path, "a"): append(block), append_events(ev, origin, period, T),
    append_compressed(c), flush(), close()."""

    def __init__(self, f, path, header, blocks, word, recalibrate, pipeline):
        self._f, self.path, self.header = f, str(path), header
        self.C, self.S, self.mode, self.seg_chunks, self.hist_bits, self.sclv = _archive_fields(header)
        self.blocks = list(blocks)
        self.T = int(sum(b.Tb for b in self.blocks))
        if recalibrate is not None and int(recalibrate) < 1:
            raise ValueError("recalibrate is None or an excess of at least 1 bit")
        self.recalibrate = None if recalibrate is None else int(recalibrate)
        self.pipeline = bool(pipeline)
        self.checksum = header.get("checksum") == "crc32"
        self.exact = header.get("exact") is True
        self._word = word                  # (peak, enc) host arrays to go on with, or None: calibrate on the next block
        self._gpu = None
        self._pending = None
        self._n = 0
        self._block_header = cio.make_header(self.S, 0, self.mode, WIN_FULL, self.seg_chunks, self.sclv, self.checksum, self.exact)
        self._block_header["preset"] = True    # what StreamEncoder.encode_block writes

    # -- records
    def _write_record(self, c, Tb):
        nb = cio.nbytes(c)
        pos = self._f.tell()
        self._f.write(PREFIX.pack(BLOCK_MAGIC, PREFIX.size + nb, self.T, Tb))
        cio.write(self._f, c)
        assert self._f.tell() == pos + PREFIX.size + nb
        self.blocks.append(Block(self.T, Tb, pos + PREFIX.size, nb))
        self.T += Tb

    def append_compressed(self, c):
        """Append a block that is already encoded (StreamEncoder.encode_block, or one received over a link).  Needs no
        GPU.  ValueError when the block is not this archive's (S, mode, seg_chunks, SCLV rows, WIN_FULL, C channels of
        one length).  An archive with checksums stores the block's own seg_crc or, for a block without, takes the
        values on the host with zlib (container_io.seg_crc_host); a block with checksums does not go into an archive
        without them (ValueError)."""
        if self.checksum and getattr(c, "seg_crc", None) is None:
            hdr = dict(c.header, format_revision=cio.CHECKSUM_REVISION)
            c = cio.Compressed(hdr, c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words, c.payload, cio.seg_crc_host(c),
                               getattr(c, "exc_seg", None), getattr(c, "exc_pos", None), getattr(c, "exc_val", None))
        _check_member(c, self.C, self.S, self.mode, self.seg_chunks, self.sclv, checksum=self.checksum, exact=self.exact)
        self._drain()
        self._write_record(c, int(c.ch_len[0]))
        self._word = (np.array(c.peak, np.uint8), np.array(c.enc, np.uint8))
        if self._gpu is not None:       # later append()s go on with this block's word
            g = self._gpu
            if g["enc"][0].peak is not None:
                torch = g["torch"]
                g["enc"][0].peak.copy_(torch.from_numpy(self._word[0]))
                g["enc"][0].enc.copy_(torch.from_numpy(self._word[1]))

    # -- device side
    def _device(self):
        if self._gpu is None:
            import torch

            from .stream import StreamEncoder
            encs = [StreamEncoder(self.C, self.S, self.hist_bits, self.sclv, mode=self.mode, seg_chunks=self.seg_chunks)
                    for _ in range(2 if self.pipeline else 1)]      # two sets of slot buffers: blocks k and k + 1
            pin = lambda n, dt: torch.empty(n, dtype=dt).pin_memory()  # noqa: E731
            sets = [dict(done=None, dense=None, small={}, peak=pin(self.C, torch.uint8), enc=pin(self.C, torch.uint8),
                         tot=pin(1, torch.int64)) for _ in encs]
            self._gpu = dict(torch=torch, enc=encs, sets=sets, copy=torch.cuda.Stream(device=encs[0].device))
        return self._gpu

    def append(self, block):
        """block: [Tb, C] time-major uint8 counts, host array or device tensor; blocks may differ in length.  Enqueues
        de-interleave, preset encode (with the drift measure when recalibrate is set) and compaction on the current
        stream, then the copies of the block's sizes to pinned memory on the archive's copy stream.  pipeline=True:
        returns then, after writing the PREVIOUS block to the file while this one runs; pipeline=False: waits for this
        block and writes it.
        In an archive created with exact=True the block's excess list is made on the time-major block itself (the COLS
        form of mhi_excess_count / mhi_excess_emit: the packed intermediate has already lost the counts above S-1), and
        the list's length is read between the two passes: ONE synchronisation of the current stream per block, behind
        the block's encode.  The file is the same with pipeline on and off."""
        g = self._device()
        torch = g["torch"]
        dev = g["enc"][0].device
        t = block if isinstance(block, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(block, np.uint8))
        if t.dim() != 2 or int(t.shape[1]) != self.C or int(t.shape[0]) < 1 or t.dtype != torch.uint8:
            raise ValueError("a block is a uint8 [Tb >= 1, %d] array" % self.C)
        t = t.to(dev).contiguous()
        lists = None
        if self.exact:
            def lists():
                from . import excess
                return excess.from_time_major(t, self.S - 1)
        self._append(int(t.shape[0]), lambda se: se.calibrate(t),
                     lambda se, track: se.encode_block_device(t, track=track, checksum=self.checksum), lists)

    def append_events(self, ev, origin, period, T):
        """append() for the block of T bins that `ev` (an events.EventSet of C channels) fills from tick `origin` at
        `period` ticks per bin: binned on the GPU straight into the encoder's packed pieces
        (StreamEncoder.encode_events_device; a first block calibrates with calibrate_events), then the same pipeline.
        The archive's time axis counts bins as before: this block is its next T steps.  ValueError in an archive created
        with exact=True: the binner writes packed pieces, which have lost the counts above S-1."""
        from .stream import _no_exact_events
        _no_exact_events(self.exact)
        T = int(T)
        if ev.C != self.C or T < 1:
            raise ValueError("a block of events has %d channels and at least 1 bin" % self.C)
        self._append(T, lambda se: se.calibrate_events(ev, origin, period, T),
                     lambda se, track: se.encode_events_device(ev, origin, period, T, track=track, checksum=self.checksum))

    def append_aer(self, ticks, channels, origin, period, T):
        """append_events() for one merged, time-ordered list of (tick, channel) pairs on the device
        (events.EventSet.from_aer: partitioned by channel there).  The same file as from the host-sorted EventSet."""
        from . import events
        from .stream import _no_exact_events
        _no_exact_events(self.exact)
        self.append_events(events.EventSet.from_aer(ticks, channels, self.C), origin, period, T)

    def _append(self, Tb, calibrate, encode, lists=None):
        """The pipeline of one block: calibrate(encoder) on a first block, encode(encoder, track) -> what
        encode_block_device returns; lists() -> the block's excess list on the device (synchronises the current stream)."""
        g = self._device()
        torch = g["torch"]
        dev = g["enc"][0].device
        k = self._n % len(g["enc"])
        se, st = g["enc"][k], g["sets"][k]
        first = g["enc"][0]
        if first.peak is None:
            if self._word is None:
                calibrate(first)       # the one device-wide synchronisation of a recording
            else:
                first.peak, first.enc = torch.from_numpy(self._word[0]).to(dev), torch.from_numpy(self._word[1]).to(dev)
            for e in g["enc"][1:]:     # one word, updated in place by adopt(), for both sets
                e.peak, e.enc = first.peak, first.enc
        cur = torch.cuda.current_stream()
        if st["done"] is not None:     # the set's previous block has left its buffers
            cur.wait_event(st["done"])
        dense, _tot, slot = encode(se, self.recalibrate is not None)
        st["peak"].copy_(se.peak, non_blocking=True)    # the word this block was coded with: in stream order before adopt()
        st["enc"].copy_(se.enc, non_blocking=True)
        if self.recalibrate is not None:
            se.adopt(slot, self.recalibrate)
        coded = torch.cuda.Event()
        coded.record(cur)
        plan, e = slot["plan"], slot["enc"]
        if Tb not in st["small"]:
            st["small"][Tb] = (torch.empty(plan.n_segments, dtype=torch.int64).pin_memory(),
                               torch.empty(self.C, dtype=torch.int64).pin_memory(),
                               torch.empty(plan.n_segments, dtype=torch.int32).pin_memory() if self.checksum else None)
        segw, bits, crc = st["small"][Tb]
        sizes = torch.cuda.Event()
        with torch.cuda.stream(g["copy"]):
            g["copy"].wait_event(coded)
            st["tot"].copy_(slot["tot"], non_blocking=True)
            segw.copy_(e.seg_words[:plan.n_segments], non_blocking=True)
            bits.copy_(e.ch_bits, non_blocking=True)
            if crc is not None:        # taken behind the compaction, in front of `coded`
                crc.copy_(slot["crc"][:plan.n_segments], non_blocking=True)
            sizes.record(g["copy"])
        job = dict(st=st, Tb=Tb, dense=dense.payload, segw=segw, bits=bits, crc=crc, sizes=sizes, exc=None)
        if lists is not None:
            made = torch.cuda.Event()
            job["exc"] = lists()
            made.record(cur)
            job["made"] = made
        self._n += 1
        self._drain()                  # block k - 1 goes to the file while block k runs
        self._pending = job
        if not self.pipeline:
            self._drain()

    def _drain(self):
        """Bring the pending block's payload to the host and write its record."""
        job, self._pending = self._pending, None
        if job is None:
            return
        g = self._gpu
        torch, st = g["torch"], job["st"]
        job["sizes"].synchronize()     # this block's kernels and small copies, nothing else
        total = int(st["tot"][0])
        if st["dense"] is None or st["dense"].numel() < total:
            st["dense"] = torch.empty(total + total // 4 + 1024, dtype=torch.int32).pin_memory()
        done = torch.cuda.Event()
        with torch.cuda.stream(g["copy"]):
            st["dense"][:total].copy_(job["dense"][:total], non_blocking=True)
            done.record(g["copy"])
        done.synchronize()
        st["done"] = done
        c = cio.Compressed(self._block_header, np.full(self.C, job["Tb"], np.uint64), st["peak"].numpy(), st["enc"].numpy(),
                           np.zeros(self.C, np.uint8), job["bits"].numpy().astype(np.uint64),
                           job["segw"].numpy().astype(np.uint64), st["dense"][:total].numpy().view(np.uint32),
                           None if job["crc"] is None else job["crc"].numpy().view(np.uint32))
        if job["exc"] is not None:
            job["made"].synchronize()
            exc_off, pos, val = job["exc"]
            cio.attach_excess(c, exc_off.cpu().numpy(), pos.cpu().numpy().view(np.uint32), val.cpu().numpy())
        self._write_record(c, job["Tb"])
        self._word = (st["peak"].numpy().copy(), st["enc"].numpy().copy())

    def flush(self):
        """every appended block is in the file (not yet the trailer: close() writes it)"""
        self._drain()
        self._f.flush()

    def close(self):
        if self._f is None:
            return
        try:
            self._drain()
        finally:
            idx = self._f.tell()
            self._f.write(INDEX_MAGIC + struct.pack("<Q", len(self.blocks)))
            for b in self.blocks:
                self._f.write(ENTRY.pack(b.offset, b.nbytes, b.t_first, b.Tb))
            self._f.write(struct.pack("<Q", idx) + END_MAGIC)
            self._f.close()
            self._f = None
            if self._gpu is not None:
                for e in self._gpu["enc"]:
                    e.close()
                self._gpu = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def create(path, C, S=3, hist_bits=6, sclv_rows=None, approx=True, seg_chunks=2, recalibrate=None, pipeline=True, meta=None,
           checksum=False, exact=False):
    """Start a new archive (an existing file is replaced) -> Writer, a context manager.  checksum=True: archive
    revision 2 -- every block carries the CRC-32 of each of its segments (module docstring).  exact=True: every block
    also carries the sparse list of its counts above S-1, and read() returns the counts themselves; the header says
    "exact": true, the revision stays, and open(path, "a") goes on in the file's mode."""
    from . import sclv
    rows = np.asarray(sclv.table(S) if sclv_rows is None else sclv_rows, dtype=np.uint8).reshape(-1, int(S))
    header = {"archive_revision": ARCHIVE_REVISION, "C": int(C), "S": int(S), "mode": MODE_APPROX if approx else MODE_NOSORT,
              "seg_chunks": int(seg_chunks), "hist_bits": int(hist_bits), "K": int(rows.shape[0]),
              "sclv": [[int(v) for v in r] for r in rows], "meta": dict(meta or {})}
    if checksum:
        header.update(archive_revision=CHECKSUM_REVISION, checksum="crc32")
    if exact:
        header["exact"] = True
    cio._header_fields(cio.make_header(S, hist_bits, header["mode"], WIN_FULL, seg_chunks, rows))   # range checks
    _archive_fields(header)
    blob = json.dumps(header, sort_keys=True).encode()
    f = builtins.open(path, "wb")
    try:
        f.write(MAGIC + struct.pack("<I", len(blob)) + blob)
        return Writer(f, path, header, [], None, recalibrate, pipeline)
    except Exception:
        f.close()
        raise


def open(path, mode="r", recalibrate=None, pipeline=True):  # noqa: A001  (builtins.open is used by name in this module)
    """mode "r" -> Reader.  mode "a" -> Writer that continues the archive: an incomplete tail and the old trailer are
    cut off, the word of the last complete block is restored and appending goes on without recalibrating."""
    if mode == "r":
        return Reader(path)
    if mode != "a":
        raise ValueError("mode is 'r' or 'a'")
    f = builtins.open(path, "r+b")
    try:
        header, _n, blocks, end, _trunc, _tb, _nread = _load(f, os.fstat(f.fileno()).st_size)
        word = None
        if blocks:
            last = cio.ContainerFile(path, blocks[-1].offset)
            word = (last.peak.copy(), last.enc.copy())
            last.close()
        f.truncate(end)
        f.seek(end)
        return Writer(f, path, header, blocks, word, recalibrate, pipeline)
    except Exception:
        f.close()
        raise
