"""exact=True end to end on the GPU, against the ORIGINAL counts: compress / StreamEncoder.encode_block / archive.create
with exact=True keep what the codec's clip at S-1 drops as a sparse list, and every reader adds it back --
decompress, decompress_range, decompress_binned, muahuff.decompress(path), Reader.read in its three branches,
read_events.  exact=False returns min(x, S-1), which is what the plain file gives.

The yardstick is NumPy on x itself.  Every case asserts that its input really has entries; the container's longest
channel has several entries in one tile, one channel of every input has none, and one has bins whose exact sum is
above 255."""
import importlib
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [9, 3000, 20000, 50000, 17 * 16384 + 5]
RATES = [2.0, 0.3, 0.8, 8.0, 1.5]          # channel 1 is clipped below to <= 1: no entry; channel 3: bins of 50 above 255
H = 6


@pytest.fixture(scope="module")
def mh():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()
    import muahuff
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    assert muahuff.CHUNK == 16384
    return muahuff


def rebin(x, r, saturate):
    """x: [rows, n] int64 -> sums of r, the last bin partial"""
    n = x.shape[1]
    k = -(-n // r)
    z = np.zeros((x.shape[0], k * r), np.int64)
    z[:, :n] = x
    s = z.reshape(x.shape[0], k, r).sum(2)
    return np.minimum(s, 255).astype(np.uint8) if saturate else s.astype(np.int32)


# ---- container -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chans():
    rng = np.random.RandomState(7)
    x = [np.minimum(rng.poisson(rate, n), 255).astype(np.uint8) for n, rate in zip(LENS, RATES)]
    x[1] = np.minimum(x[1], 1)
    x[4][[64, 65, 16383, 16384, 2 * 16384 - 1, 2 * 16384, LENS[4] - 1]] = 255        # window, tile and segment edges
    x[4][0] = 255                                                                    # inside WIN_FULL only
    return x


def windowed(mh, chans, window, clip=None):
    """[C, Tmax] int64: x inside each channel's encoded window (clipped at `clip`), 0 outside and past its length"""
    from muahuff import container_io as cio
    w0, w1 = cio.window_bounds(np.array(LENS, np.uint64), H, window)
    out = np.zeros((len(chans), max(LENS)), np.int64)
    for i, x in enumerate(chans):
        v = x.astype(np.int64) if clip is None else np.minimum(x.astype(np.int64), clip)
        out[i, w0[i]:w1[i]] = v[w0[i]:w1[i]]
    return out


@pytest.fixture(scope="module", params=[(3, "after_cal"), (3, "full"), (5, "after_cal"), (5, "full")], ids=lambda p: "S%d-%s" % p)
def packed(request, mh, chans, tmp_path_factory):
    """(S, window, exact container, plain container, path of the exact file, path of the plain file)"""
    from muahuff import container_io as cio
    from muahuff.container import ChannelSet
    S, wname = request.param
    window = mh.WIN_AFTER_CAL if wname == "after_cal" else mh.WIN_FULL
    cs = ChannelSet.from_channels(chans)
    rows = mh.sclv.table(S)
    e = cio.compress(cs, S, H, mh.MODE_APPROX, rows, window=window, seg_chunks=2, exact=True)
    p = cio.compress(cs, S, H, mh.MODE_APPROX, rows, window=window, seg_chunks=2)
    d = tmp_path_factory.mktemp("exact")
    cio.save(d / "e.mh", e)
    cio.save(d / "p.mh", p)
    return S, window, e, p, str(d / "e.mh"), str(d / "p.mh")


def test_container_round_trip(mh, chans, packed):
    from muahuff import container_io as cio
    S, window, e, p, epath, ppath = packed
    want, clipped = windowed(mh, chans, window), windowed(mh, chans, window, S - 1)
    n = len(e.exc_pos)
    assert n == int((want > S - 1).sum()) > 0 and e.excess_bits == 40 * n + 64 * (len(e.seg_words) + 1) and p.excess_bits == 0
    seg = e.exc_seg.astype(np.int64)
    first = np.concatenate([[0], np.cumsum(cio.check_consistent(e, arrays=False))])
    per_ch = np.diff(seg[first])
    assert per_ch[1] == 0 and per_ch[4] > 17 * 3                              # a channel with none; several per tile
    assert np.bincount(e.exc_pos[seg[first[4]]:seg[first[5]]] // 16384, minlength=17)[:17].min() > 3
    # the stream is the plain container's, byte for byte
    for name, _dt in cio.ARRAYS:
        assert np.array_equal(getattr(e, name), getattr(p, name)), name
    eb, pb = e.tobytes(), p.tobytes()
    ebody, pbody = (blob[12 + struct.unpack("<I", blob[8:12])[0]:] for blob in (eb, pb))
    tail = sum(a.nbytes + (-a.nbytes % 8) for a in (e.exc_seg, e.exc_pos, e.exc_val))
    assert ebody[:len(pbody)] == pbody and len(ebody) == len(pbody) + tail

    def rows_of(cs):
        out = np.zeros((len(LENS), max(LENS)), np.int64)
        for i, r in enumerate(cs.to_channels()):
            out[i, :len(r)] = r
        return out
    assert np.array_equal(rows_of(cio.decompress(e)), want)
    assert np.array_equal(rows_of(cio.decompress(cio.load(epath), exact=True)), want)
    assert np.array_equal(rows_of(cio.decompress(e, exact=False)), clipped)
    assert np.array_equal(rows_of(cio.decompress(cio.load(ppath))), clipped)
    with pytest.raises(ValueError, match="exact=True"):
        cio.decompress(p, exact=True)
    got = cio.decompress(e, channels=[4, 1, 4, 3]).to_channels()             # repeated and re-ordered
    for r, i in zip(got, [4, 1, 4, 3]):
        assert np.array_equal(r, want[i, :LENS[i]])
    for r, i in zip(mh.decompress(epath, channels=[3, 0]), [3, 0]):
        assert np.array_equal(r, want[i, :LENS[i]])
    for r, i in zip(mh.decompress(epath, channels=[3, 0], exact=False), [3, 0]):
        assert np.array_equal(r, clipped[i, :LENS[i]])


RANGES = [(0, max(LENS)), (5 * 16384 + 11, 9 * 16384 + 400), (100, 2900), (2 * 16384 - 1, 2 * 16384 + 1), (60, 70)]
SEL = [4, 2, 4, 0, 3, 1]


def test_container_range_and_binned(mh, chans, packed):
    from muahuff import container_io as cio
    S, window, e, p, epath, ppath = packed
    want, clipped = windowed(mh, chans, window), windowed(mh, chans, window, S - 1)
    with cio.open(epath) as f, cio.open(ppath) as pf:
        for src in (e, f):
            for a, b in RANGES:
                got = cio.decompress_range(src, a, b, channels=SEL).cpu().numpy()
                assert np.array_equal(got, want[SEL, a:b]), (a, b)
                assert (want[SEL, a:b] > S - 1).any() or b - a <= 10
                got = cio.decompress_range(src, a, b, channels=SEL, exact=False).cpu().numpy()
                assert np.array_equal(got, clipped[SEL, a:b])
            a, b = RANGES[1]
            tm = cio.decompress_range(src, a, b, channels=SEL, time_major=True).cpu().numpy()
            assert np.array_equal(tm, want[SEL, a:b].T)
            for r, a, b in ((50, 0, max(LENS)), (50, 81950, 9 * 16384 + 421), (7, 32760, 2 * 16384 + 30), (4096, 0, 70000)):
                assert a % r == 0
                for sat in (True, False):
                    got = cio.decompress_binned(src, r, a, b, channels=SEL, saturate=sat).cpu().numpy()
                    ref = rebin(want[SEL, a:b], r, sat)
                    assert got.dtype == ref.dtype and np.array_equal(got, ref), (r, a, b, sat)
                    got = cio.decompress_binned(src, r, a, b, channels=SEL, saturate=sat, exact=False).cpu().numpy()
                    assert np.array_equal(got, rebin(clipped[SEL, a:b], r, sat))
            assert rebin(want[[3], :50000], 50, False).max() > 255             # a bin whose exact sum exceeds a byte
        assert np.array_equal(cio.decompress_range(pf, 100, 2900).cpu().numpy(), clipped[:, 100:2900])
        with pytest.raises(ValueError, match="exact=True"):
            cio.decompress_range(pf, 100, 2900, exact=True)
        with pytest.raises(ValueError, match="exact=True"):
            cio.decompress_binned(pf, 50, exact=True)
    rows = mh.decompress(epath, channels=[3, 4], start=100, stop=40000, bin=50)
    assert np.array_equal(np.stack(rows), rebin(want[[3, 4], 100:40000], 50, True))


# ---- stream block --------------------------------------------------------------------------------------------------
C, BLOCKS = 70, (20000, 16384, 5000)


@pytest.fixture(scope="module")
def recording():
    """[T, C] time-major counts: rates 0.05 .. 6, channel 3 never above 2 (no entry), channel 9 at rate 9"""
    rng = np.random.RandomState(17)
    T = sum(BLOCKS) + 5000
    rates = np.linspace(0.05, 6.0, C)
    rates[9] = 9.0
    x = np.minimum(rng.poisson(rates, (T, C)), 255).astype(np.uint8)
    x[:, 3] = np.minimum(x[:, 3], 2)
    x[[0, 19999, 20000, 36383, 36384, 41383], 5] = 255           # first and last step of every block
    return x


def test_stream_block(mh, recording):
    from muahuff.stream import StreamEncoder
    se = StreamEncoder(C, 3, H, mh.sclv.table(3))
    x = recording[:20000]
    se.calibrate(x)
    e, p = se.encode_block(x, exact=True), se.encode_block(x)
    assert len(e.exc_pos) == int((x > 2).sum()) > 0 and e.header["exact"] is True and "exact" not in p.header
    assert np.array_equal(e.payload, p.payload) and np.array_equal(e.seg_words, p.seg_words)
    assert np.array_equal(StreamEncoder.decode_block(e), x)
    assert np.array_equal(StreamEncoder.decode_block(p), np.minimum(x, 2))
    from muahuff import events
    ev = events.EventSet(torch.zeros(0, dtype=torch.int64, device="cuda"), np.zeros(C + 1, np.uint64), check=False)
    with pytest.raises(ValueError, match="exact=True"):
        se.encode_events(ev, 0, 1, 100, exact=True)
    with pytest.raises(ValueError, match="exact=True"):
        se.encode_events_device(ev, 0, 1, 100, exact=True)
    se.close()


# ---- archive -------------------------------------------------------------------------------------------------------
def _write(mh, path, x, blocks, **kw):
    from muahuff import archive
    with archive.create(path, C, S=3, hist_bits=H, **kw) as w:
        t = 0
        for n in blocks:
            w.append(x[t:t + n])
            t += n
    return t


@pytest.fixture(scope="module")
def files(mh, recording, tmp_path_factory):
    d = tmp_path_factory.mktemp("arch")
    paths = {k: str(d / (k + ".mha")) for k in ("exact", "serial", "plain", "crc")}
    _write(mh, paths["exact"], recording, BLOCKS, exact=True, pipeline=True)
    _write(mh, paths["serial"], recording, BLOCKS, exact=True, pipeline=False)
    _write(mh, paths["plain"], recording, BLOCKS)
    _write(mh, paths["crc"], recording, BLOCKS, exact=True, checksum=True)
    return paths


def test_archive_files(mh, recording, files):
    from muahuff import archive
    assert open(files["exact"], "rb").read() == open(files["serial"], "rb").read()        # pipeline on and off
    with archive.open(files["exact"]) as a, archive.open(files["plain"]) as p, archive.open(files["crc"]) as c:
        assert a.exact and not p.exact and c.exact and c.checksum
        assert (a.header["archive_revision"], c.header["archive_revision"], p.header["archive_revision"]) == (1, 2, 1)
        assert a.header["exact"] is True and "exact" not in p.header
        t = 0
        for i, n in enumerate(BLOCKS):
            blk = a.block(i)
            assert len(blk.exc_pos) == int((recording[t:t + n] > 2).sum()) > 0 and blk.header["format_revision"] == 3
            assert np.array_equal(blk.payload, p.block(i).payload)
            assert "excess_crc32" in c.block(i).header and c.block(i).header["format_revision"] == 4
            t += n
        assert c.verify() == [] and c.verify(device=False) == []


QUERIES = [(0, sum(BLOCKS), None), (19000, 37000, [5, 0, 69, 5, 3, 9]), (19999, 20001, [5, 9]), (36000, 41384, None)]


@pytest.mark.parametrize("which", ["exact", "crc"])
def test_archive_read(mh, recording, files, which):
    from muahuff import archive
    T = sum(BLOCKS)
    x = recording[:T].T.astype(np.int64)                         # [C, T]
    clipped = np.minimum(x, 2)
    with archive.open(files[which]) as a:
        for s0, s1, ch in QUERIES:
            rows = slice(None) if ch is None else ch
            assert (x[rows, s0:s1] > 2).any()
            assert np.array_equal(a.read(s0, s1, channels=ch).cpu().numpy(), x[rows, s0:s1]), (s0, s1)
            assert np.array_equal(a.read(s0, s1, channels=ch, exact=False).cpu().numpy(), clipped[rows, s0:s1])
            assert np.array_equal(a.read(s0, s1, channels=ch, time_major=True).cpu().numpy(), x[rows, s0:s1].T)
        # bin = 16: every block starts on the grid; bin = 50: block 2 (t_first 36384) is off it; 4096: bins across blocks
        for r in (16, 50, 4096):
            assert all(t % 16 == 0 for t in (20000, 36384)) and 36384 % 50 != 0
            for s0, s1, ch in ((0, T, None), (r * (19000 // r), 37003, [9, 5, 9, 3]), (r * 4, 36400, [9])):
                rows = slice(None) if ch is None else ch
                for sat in (True, False):
                    got = a.read(s0, s1, channels=ch, bin=r, saturate=sat).cpu().numpy()
                    ref = rebin(x[rows, s0:s1], r, sat)
                    assert got.dtype == ref.dtype and np.array_equal(got, ref), (r, s0, s1, sat)
                    got = a.read(s0, s1, channels=ch, bin=r, saturate=sat, exact=False).cpu().numpy()
                    assert np.array_equal(got, rebin(clipped[rows, s0:s1], r, sat))
                got = a.read(s0, s1, channels=ch, bin=r, time_major=True).cpu().numpy()
                assert np.array_equal(got, rebin(x[rows, s0:s1], r, True).T)
        assert rebin(x[[9]], 50, False).max() > 255 and not (x[3] > 2).any()
        ev = a.read_events(0, T)
        assert int(ev.ticks.numel()) == int(x.sum()) > int(clipped.sum())
        assert int(a.read_events(0, T, exact=False).ticks.numel()) == int(clipped.sum())
        ticks, chn = a.read_events(19990, 20010, channels=[9, 5], aer=True)
        assert int(ticks.numel()) == int(x[[9, 5], 19990:20010].sum())
    out = mh.decompress(files[which], channels=[9], start=19000, stop=37000)
    assert np.array_equal(out[0], x[9, 19000:37000])


def test_archive_append_and_refusals(mh, recording, files, tmp_path):
    import shutil

    from muahuff import archive, events
    T = sum(BLOCKS)
    path = str(tmp_path / "more.mha")
    shutil.copy(files["exact"], path)
    with archive.open(path, "a") as w:
        assert w.exact
        w.append(recording[T:T + 5000])
        ev = events.EventSet(torch.zeros(0, dtype=torch.int64, device="cuda"), np.zeros(C + 1, np.uint64), check=False)
        with pytest.raises(ValueError, match="exact=True"):
            w.append_events(ev, 0, 1, 100)
        with pytest.raises(ValueError, match="exact=True"):
            w.append_aer(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 0, 1, 100)
        with archive.open(files["plain"]) as p:
            with pytest.raises(ValueError, match="excess lists"):
                w.append_compressed(p.block(0))                  # plain blocks and exact blocks do not mix
    with archive.open(path) as a:
        assert a.T == T + 5000 and len(a.blocks) == 4
        got = a.read(T - 100, T + 5000).cpu().numpy()
        assert np.array_equal(got, recording[T - 100:T + 5000].T) and (got > 2).any()
    with archive.open(files["plain"]) as p:
        with pytest.raises(ValueError, match="exact=True"):
            p.read(0, 100, exact=True)
        with pytest.raises(ValueError, match="exact=True"):
            p.read_events(0, 100, exact=True)
        assert np.array_equal(p.read(0, 100).cpu().numpy(), np.minimum(recording[:100].T, 2))
    plain = str(tmp_path / "plain.mha")
    shutil.copy(files["plain"], plain)
    with archive.open(plain, "a") as w, archive.open(files["exact"]) as a:
        assert not w.exact
        with pytest.raises(ValueError, match="excess lists"):
            w.append_compressed(a.block(0))
