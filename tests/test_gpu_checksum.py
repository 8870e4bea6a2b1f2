"""Payload checksums on the GPU: k_seg_crc32 (mhi_seg_crc32, include/muahuff_ingest.h) against zlib on payloads that
owe nothing to the codec -- every buffer inside canaries --, its verify form on clean, altered and out-of-range
directories, and the option end to end: compress / decompress / range / re-bin, the stream's two ends, and an archive
whose read() names the block and the segment of one flipped payload bit."""
import ctypes as ct
import shutil
import zlib

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _ingest, archive
from muahuff import container_io as cio
from muahuff.container import ChannelSet
from tests import helpers
from tests.test_host_checksum import _flip_behind_a_chunk_header

pytestmark = pytest.mark.gpu
CH = muahuff.CHUNK
GUARD = 1024                    # canary words on either side of every buffer
CAN32, CAN64 = 0x5A5AC3C3, 0x5A5AC3C3A5A53C3C
NONE = (1 << 64) - 1            # bad[1] while no segment has mismatched
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 259, 64 * 4 * 3 + 7, 9300)      # words
CAP_WAVES = 4 * 2048            # csrc/mh_crc.hpp: kCrcWaves segments per workgroup, at most kCrcMaxGroups workgroups


@pytest.fixture(scope="module")
def mh():
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    return _ingest.lib()


def _framed(values, dtype, canary):
    """values inside GUARD canary entries on either side -> (whole device tensor, view of the values)"""
    values = np.ascontiguousarray(values, dtype)
    whole = np.full(values.size + 2 * GUARD, canary, dtype)
    whole[GUARD:GUARD + values.size] = values
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[np.dtype(dtype)]
    t = torch.from_numpy(whole.view(signed)).cuda()
    return t, t[GUARD:GUARD + values.size]


class Case:
    """A directory over random words: segments of `sizes` words back to back behind `lead` words, so that a segment
    starts at any word offset; payload (one word off a 16-byte boundary), offsets, sizes, crc and bad each sit inside
    canaries."""

    def __init__(self, sizes, lead=0, seed=0):
        rng = np.random.RandomState(seed)
        self.words = np.array(sizes, np.uint64)
        self.off = (np.uint64(lead) + np.cumsum(self.words) - self.words).astype(np.uint64)
        self.total = int(self.off[-1] + self.words[-1])
        self.host = rng.randint(0, 1 << 32, size=self.total, dtype=np.uint64).astype(np.uint32)
        self.n = len(sizes)
        self.want = np.array([zlib.crc32(self.host[int(o):int(o + w)].tobytes()) if w else 0
                              for o, w in zip(self.off, self.words)], np.uint32)
        self.load()

    def load(self):
        whole = np.full(self.total + 2 * GUARD + 1, CAN32, np.uint32)
        whole[GUARD + 1:GUARD + 1 + self.total] = self.host
        self.frame_host = whole
        self.frame = torch.from_numpy(whole.view(np.int32)).cuda()
        self.payload = self.frame[GUARD + 1:GUARD + 1 + self.total]
        assert self.payload.data_ptr() % 16 == 4
        self.f_off, self.d_off = _framed(self.off, np.uint64, CAN64)
        self.f_words, self.d_words = _framed(self.words, np.uint64, CAN64)
        self.f_crc, self.d_crc = _framed(np.full(self.n, CAN32), np.uint32, CAN32)
        self.f_bad, self.d_bad = _framed([0, NONE], np.uint64, CAN64)
        self.f_expect, self.d_expect = _framed(self.want, np.uint32, CAN32)

    def call(self, mh, idx=None, crc=True, expect=False, stream=None, payload_words=None):
        self.d_idx = None if idx is None else torch.from_numpy(np.array(idx, np.uint64).view(np.int64)).cuda()
        p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = mh.mhi_seg_crc32(p(self.payload), self.total if payload_words is None else payload_words, p(self.d_off),
                              p(self.d_words), self.n, None if idx is None else p(self.d_idx), 0 if idx is None else len(idx),
                              p(self.d_crc) if crc else None, p(self.d_expect) if expect else None,
                              p(self.d_bad) if expect else None, ct.c_void_p(st))
        assert rc == 0, mh.mhi_last_error().decode()

    def crc(self):
        return self.d_crc.cpu().numpy().view(np.uint32)

    def bad(self):
        return [int(v) for v in self.d_bad.cpu().numpy().view(np.uint64)]

    def check_frames(self, crc_written=None):
        """the canaries, the payload and the directory are what they were; crc entries outside crc_written too"""
        torch.cuda.synchronize()
        assert np.array_equal(self.frame.cpu().numpy().view(np.uint32), self.frame_host)
        for f, can in ((self.f_off, CAN64), (self.f_words, CAN64), (self.f_bad, CAN64), (self.f_crc, CAN32), (self.f_expect, CAN32)):
            a = f.cpu().numpy().view(np.uint64 if can == CAN64 else np.uint32)
            assert (a[:GUARD] == can).all() and (a[-GUARD:] == can).all()
        if crc_written is not None:
            rest = np.setdiff1d(np.arange(self.n), np.array(crc_written, np.int64))
            assert (self.crc()[rest] == CAN32).all()


LAYOUTS = [(SIZES, 0), (SIZES[::-1], 1), (SIZES[3:] + SIZES[:3], 2), (SIZES + SIZES, 3)]


@pytest.mark.parametrize("k", range(len(LAYOUTS)))
def test_every_segment_against_zlib(mh, k):
    sizes, lead = LAYOUTS[k]
    c = Case(sizes, lead, seed=k)
    c.call(mh)
    torch.cuda.synchronize()
    assert np.array_equal(c.crc(), c.want), np.nonzero(c.crc() != c.want)[0]
    assert (c.want[c.words == 0] == 0).all()
    c.check_frames()


def test_the_layouts_start_segments_at_every_word_offset_and_off_the_rows():
    starts, rows = set(), set()
    for sizes, lead in LAYOUTS:
        c = Case(sizes, lead)
        nz = c.words > 0
        starts |= {int(o) % 4 for o in c.off[nz]}
        rows |= {int(o) % 256 != 0 for o in c.off[nz]}
        assert set(SIZES) <= set(sizes)
    assert starts == {0, 1, 2, 3} and True in rows


def test_a_permuted_subset_on_a_side_stream_writes_the_listed_segments_only(mh):
    c = Case(SIZES + SIZES[::-1], 1, seed=7)
    idx = [20, 3, 10, 0, 9, 21, 12, 10]         # any order, a repeat
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c.call(mh, idx=idx, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(c.crc()[idx], c.want[idx])
    c.check_frames(crc_written=idx)


def test_two_calls_in_a_row_and_a_graph_replay(mh):
    a, b = Case(SIZES, 2, seed=11), Case(SIZES[::-1], 3, seed=12)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a.call(mh, stream=side.cuda_stream)
        b.call(mh, stream=side.cuda_stream)
        a.call(mh, expect=True, stream=side.cuda_stream)        # the verify form behind the compute form, one counter
        side.synchronize()
    assert np.array_equal(a.crc(), a.want) and np.array_equal(b.crc(), b.want) and a.bad() == [0, NONE]
    # captured once, replayed on changed words: nothing but launches on the stream
    other = np.random.RandomState(13).randint(0, 1 << 32, size=a.total, dtype=np.uint64).astype(np.uint32)
    want2 = np.array([zlib.crc32(other[int(o):int(o + w)].tobytes()) if w else 0 for o, w in zip(a.off, a.words)], np.uint32)
    pin = torch.from_numpy(other.view(np.int32)).pin_memory()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        a.call(mh, stream=side.cuda_stream)
    with torch.cuda.stream(side):
        a.payload.copy_(pin, non_blocking=True)
        a.d_crc.fill_(0)
        g.replay()
        side.synchronize()
    assert np.array_equal(a.crc(), want2)
    a.frame_host[GUARD + 1:GUARD + 1 + a.total] = other
    a.check_frames()
    b.check_frames()


def test_more_segments_than_the_capped_grid_holds(mh):
    """the grid is min(ceil(n / 4), 2048) workgroups of 4 waves: a longer list is walked in strides of 4 * gridDim.x"""
    n = 3 * CAP_WAVES + 5
    assert n > CAP_WAVES
    sizes = [(0, 1, 2, 3, 5, 17, 300)[i % 7] for i in range(n)]
    c = Case(sizes, 1, seed=3)
    c.call(mh)
    torch.cuda.synchronize()
    assert np.array_equal(c.crc(), c.want)
    idx = np.random.RandomState(4).permutation(n)[:CAP_WAVES + 9]
    c.d_crc.fill_(0)
    c.call(mh, idx=idx, crc=False, expect=True)
    assert c.bad() == [0, NONE] and (c.crc() == 0).all()
    c.check_frames()


# ---- the verify form -----------------------------------------------------------------------------------
def test_verify_counts_altered_segments_and_names_the_lowest(mh):
    c = Case(SIZES + SIZES, 1, seed=21)
    c.call(mh, crc=False, expect=True)
    assert c.bad() == [0, NONE]
    hit = [13, 6, 20]                            # 6: 256 words, 13: 3 words, 20: 64 * 4 * 3 + 7
    assert all(c.words[s] > 0 for s in hit)
    for s, where in zip(hit, (0, 255, 500)):     # first word, last word, the middle of a row
        c.payload[int(c.off[s]) + where] ^= 1 << (s % 32)
    c.call(mh, crc=False, expect=True)
    assert c.bad() == [len(hit), min(hit)]
    c.call(mh, idx=[1, 20, 2, 13], crc=False, expect=True)       # the counter accumulates; the minimum stays
    assert c.bad() == [len(hit) + 2, min(hit)]
    c.frame_host = c.frame.cpu().numpy().view(np.uint32).copy()
    c.check_frames(crc_written=[])


def test_out_of_range_values_are_counted_and_never_followed(mh):
    """valid buffers, out-of-range VALUES: a segment that ends behind the payload, one whose end wraps 64 bits, a size
    beyond the payload, and list entries beyond the directory"""
    c = Case(SIZES, 1, seed=22)
    off, words = c.off.copy(), c.words.copy()
    off[4] = np.uint64(c.total - 2)              # 5 words from there: 3 too many
    off[6] = np.uint64((1 << 64) - 2)            # + 256 wraps to 254
    words[8] = np.uint64(1 << 40)
    off[9] = np.uint64(c.total)                  # 0 words AT the end would be fine; this one has 775
    c.d_off.copy_(torch.from_numpy(off.view(np.int64)))
    c.d_words.copy_(torch.from_numpy(words.view(np.int64)))
    outside = [4, 6, 8, 9]
    c.call(mh, expect=True)
    want = c.want.copy()
    want[outside] = 0                            # written as 0
    assert np.array_equal(c.crc(), want)
    assert c.bad() == [len(outside), min(outside)]
    c.d_bad.copy_(torch.from_numpy(np.array([0, NONE], np.uint64).view(np.int64)))
    c.d_crc.fill_(0x11111111)
    c.call(mh, idx=[c.n, 2, 1 << 63, 4, (1 << 64) - 1], expect=True)         # three entries beyond the directory
    assert c.bad() == [4, 4]
    got = c.crc()
    assert got[2] == c.want[2] and got[4] == 0 and (np.delete(got, [2, 4]) == 0x11111111).all()
    # a payload_words below the buffer: the segments behind it are not read
    c2 = Case(SIZES, 0, seed=23)
    cut = int(c2.off[-1]) + 10
    c2.call(mh, expect=True, payload_words=cut)
    assert c2.bad() == [1, c2.n - 1] and c2.crc()[-1] == 0 and np.array_equal(c2.crc()[:-1], c2.want[:-1])
    c.check_frames()
    c2.check_frames()


# ---- end to end ------------------------------------------------------------------------------------------
LENS = (40000, CH * 17 + 5, 9, 70001, 3000)
_SETS = {}


@pytest.fixture(scope="module")
def sets(mh):
    """S -> (channels, plain container, checksummed container); compressed once"""
    def get(S):
        if S not in _SETS:
            rng = np.random.RandomState(S)
            chans = [np.minimum(rng.poisson(0.4 + 0.6 * i, size=T), 255).astype(np.uint8) for i, T in enumerate(LENS)]
            cs = ChannelSet.from_channels(chans)
            tab = helpers.sclv_tables()[S]
            plain = cio.compress(cs, S, 6, muahuff.MODE_APPROX, tab, seg_chunks=2)
            summed = cio.compress(cs, S, 6, muahuff.MODE_APPROX, tab, seg_chunks=2, checksum=True)
            _SETS[S] = (chans, plain, summed)
        return _SETS[S]
    return get


@pytest.mark.parametrize("S", [3, 8])
def test_compress_with_checksums(sets, S, tmp_path):
    chans, plain, k = sets(S)
    assert plain.seg_crc is None and plain.header["format_revision"] == 3
    assert k.header["format_revision"] == 4 and k.seg_crc.dtype == np.uint32 and len(k.seg_crc) == len(k.seg_words)
    assert np.array_equal(k.payload, plain.payload) and np.array_equal(k.seg_words, plain.seg_words)
    assert np.array_equal(k.seg_crc, cio.seg_crc_host(k))
    assert len(set(int(o) % 4 for o in np.cumsum(k.seg_words))) > 1      # compacted segments start off 16-byte boundaries
    fn = str(tmp_path / "k.muahuff")
    cio.save(fn, k)
    a = cio.decompress(plain).to_channels()
    for src in (k, cio.load(fn)):
        b = cio.decompress(src).to_channels()
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    sub = cio.decompress(k, channels=[3, 1]).to_channels()
    assert np.array_equal(sub[0], a[3]) and np.array_equal(sub[1], a[1])
    with cio.open(fn) as cf:
        for start, stop, ch in ((0, 70001, None), (33000, 66000, [3, 0, 1]), (CH * 2 - 1, CH * 2 + 1, [1]), (100, 100, None)):
            want = cio.decompress_range(plain, start, stop, ch).cpu().numpy()
            assert np.array_equal(cio.decompress_range(k, start, stop, ch).cpu().numpy(), want)
            assert np.array_equal(cio.decompress_range(cf, start, stop, ch).cpu().numpy(), want)
        for r, start, stop, ch in ((7, 0, None, None), (100, 32800, 65000, [1, 3]), (4096, 0, 70001, [4, 0])):
            want = cio.decompress_binned(plain, r, start, stop, ch).cpu().numpy()
            assert np.array_equal(cio.decompress_binned(k, r, start, stop, ch).cpu().numpy(), want)
            assert np.array_equal(cio.decompress_binned(cf, r, start, stop, ch).cpu().numpy(), want)
    api = muahuff.compress(chans, S=S, hist_bits=6, checksum=True)
    assert api.header["format_revision"] == 4 and np.array_equal(api.seg_crc, cio.seg_crc_host(api))


def test_a_flipped_bit_in_a_container_is_named(sets):
    _chans, _plain, k = sets(3)
    off = np.concatenate([[0], np.cumsum(k.seg_words)]).astype(int)
    nseg = cio.check_consistent(k)
    ch = 3                                                  # 70001 samples behind 64 of calibration: no head segment
    seg = int(np.sum(nseg[:ch])) + 1                        # its second segment: window samples 32768 .. 65535
    t0 = 64 + 2 * CH
    assert nseg[ch] == 3 and k.header["window"] == muahuff.WIN_AFTER_CAL and k.header["seg_chunks"] == 2
    w0 = int(k.payload[off[seg]])
    word = off[seg] + ((16 + 64 * ((w0 >> 12) & 15) + 31) >> 5) + 3
    bad = cio.Compressed(k.header, k.ch_len, k.peak, k.enc, k.skipped, k.ch_bits, k.seg_words, k.payload.copy(), k.seg_crc)
    bad.payload[word] ^= 1 << 9
    for call in (lambda **kw: cio.decompress(bad, **kw), lambda **kw: cio.decompress(bad, channels=[ch], **kw),
                 lambda **kw: cio.decompress_range(bad, int(t0) + 10, int(t0) + 20, [ch], **kw),
                 lambda **kw: cio.decompress_binned(bad, 5, 0, None, [ch, 0], **kw)):
        with pytest.raises(ValueError, match="corrupt container: checksum of segment %d " % seg):
            call()
        call(check=False)
    cio.decompress_range(bad, 0, 70001, [c for c in range(len(LENS)) if c != ch])   # a query that does not read it


def test_stream_blocks_with_checksums(mh):
    from muahuff.stream import StreamDecoder, StreamEncoder
    C, S, Tb = 6, 3, 2 * CH + 77
    tab = helpers.sclv_tables()[S]
    rng = np.random.RandomState(9)
    x = np.minimum(rng.poisson(0.7, size=(Tb, C)), 255).astype(np.uint8)
    se = StreamEncoder(C, S, 6, tab)
    se.calibrate(x)
    plain, k = se.encode_block(x), se.encode_block(x, checksum=True)
    assert plain.seg_crc is None and k.header["format_revision"] == 4
    assert np.array_equal(k.payload, plain.payload) and np.array_equal(k.seg_crc, cio.seg_crc_host(k))
    sd = StreamDecoder(C, S, tab)
    want = np.minimum(x, S - 1)
    assert np.array_equal(sd.decode_block(k), want) and np.array_equal(StreamEncoder.decode_block(k), want)
    k.payload[40] ^= 4                          # behind the first chunk header (25 words at the most) of segment 0
    assert k.seg_words[0] > 41
    with pytest.raises(ValueError, match="checksum of segment 0 "):
        sd.decode_block(k)
    assert sd.decode_block(k, check=False).shape == want.shape
    se.close()
    sd.close()


ATB = (40000, 20001, 50000)
AC = 8


@pytest.fixture(scope="module")
def arcs(mh, tmp_path_factory):
    """paths of (checksummed + pipelined, checksummed + plain writer, no checksums) archives of the same three blocks"""
    d = tmp_path_factory.mktemp("sum")
    rng = np.random.RandomState(77)
    blocks = [np.minimum(rng.poisson(0.2 + 0.3 * np.arange(AC), size=(Tb, AC)), 255).astype(np.uint8) for Tb in ATB]
    out = []
    for name, kw in (("pipe", dict(checksum=True, pipeline=True)), ("plain", dict(checksum=True, pipeline=False)),
                     ("none", dict())):
        fn = str(d / (name + ".mua"))
        with archive.create(fn, AC, S=3, hist_bits=6, seg_chunks=2, **kw) as w:
            for k, x in enumerate(blocks):
                w.append(torch.from_numpy(x).cuda() if k % 2 else x)
        out.append(fn)
    return out, blocks


def test_archive_with_checksums(arcs, tmp_path):
    (pipe, plain, none), blocks = arcs
    assert open(pipe, "rb").read() == open(plain, "rb").read()
    with archive.open(pipe) as r, archive.open(none) as r0:
        assert r.checksum and not r0.checksum and r.header["archive_revision"] == 2
        for i in range(len(ATB)):
            b, b0 = r.block(i), r0.block(i)
            assert b.header["format_revision"] == 4 and np.array_equal(b.payload, b0.payload)
            assert np.array_equal(b.seg_crc, cio.seg_crc_host(b))
        assert r.verify() == [] and r.verify(device=False) == []
        want = np.minimum(np.concatenate(blocks), 2).T
        for a, b, ch, rr in ((39000, 41000, None, None), (0, sum(ATB), [5, 0], None), (39990, 60020, [3], 10)):
            got = r.read(a, b, ch, bin=rr).cpu().numpy()
            assert np.array_equal(got, r0.read(a, b, ch, bin=rr).cpu().numpy())
            if rr is None:
                assert np.array_equal(got, want[:, a:b] if ch is None else want[ch][:, a:b])
    # one payload bit of channel 3's second segment of block 0 (steps 32768 .. 39999), flipped in the file
    fn = str(tmp_path / "flipped.mua")
    shutil.copy(pipe, fn)
    block, seg = 0, 2 * 3 + 1
    with archive.open(pipe) as r:
        assert len(r.block_file(block).seg_words) == 2 * AC
        _flip_behind_a_chunk_header(fn, r, block, seg)
    with archive.open(fn) as r:
        with pytest.raises(ValueError, match="corrupt archive: checksum of segment %d of block %d " % (seg, block)):
            r.read(39000, 41000)
        assert r.read(39000, 41000, check=False).shape == (AC, 2000)
        assert r.read(39000, 41000, [0, 1, 2, 4]).shape == (4, 2000)       # the same range without the channel
        assert r.read(0, 30000).shape == (AC, 30000)                       # the channel without the segment
        assert r.read(40000, 60001).shape == (AC, 20001)                   # the next block
        assert r.verify() == [(block, seg)] == r.verify(device=False)


def test_append_compressed_and_reopening_keep_the_checksums(arcs, tmp_path):
    (pipe, _plain, none), blocks = arcs
    fn = str(tmp_path / "more.mua")
    shutil.copy(pipe, fn)
    with archive.open(none) as r0:
        extra = r0.block(1)                     # a block without checksums: the values come from zlib
    with archive.open(fn, "a") as w:
        assert w.checksum
        w.append_compressed(extra)
        w.append(blocks[2])
    with archive.open(fn) as r:
        assert len(r.blocks) == 5 and all(r.block(i).header["format_revision"] == 4 for i in range(5))
        assert r.verify() == []
        assert np.array_equal(r.read(sum(ATB), sum(ATB) + ATB[1]).cpu().numpy(), np.minimum(blocks[1], 2).T)
