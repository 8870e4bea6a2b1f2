"""archive.Reader.read_windows and container_io.decompress_windows on the GPU: trial-aligned windows of a stored
recording against a NumPy cut of the original -- clipped at S-1 for a plain file, the counts themselves for an exact
one -- across block boundaries, with shared segments, unsorted and repeated triggers; every span is read once
(bytes_read), a corrupt segment raises what read() raises, and a ragged container gives the zero-extended rows."""
import shutil

import numpy as np
import pytest
import torch

import muahuff
from muahuff import archive, windows
from muahuff import container_io as cio
from tests.test_host_checksum import _flip_behind_a_chunk_header

pytestmark = pytest.mark.gpu

C, S, TB = 40, 3, [20000, 33000, 16384, 5000]
T = sum(TB)
PRE, POST = 30, 70
# windows that straddle each block boundary, that share a segment, unsorted, repeated, the first and the last possible
TRIGGERS = np.array([20000, 53010, 69384 + 20, 19990, 60000, 60050, 60010, 30, 53010, T - 70, 41000, 20000, 7000, 7100])


@pytest.fixture(scope="module")
def arcs(tmp_path_factory):
    d = tmp_path_factory.mktemp("win")
    rng = np.random.RandomState(12)
    rec = np.minimum(rng.poisson(0.3 + 0.05 * np.arange(C), size=(T, C)), 255).astype(np.uint8)
    rec[rng.rand(T, C) < 0.001] = 255
    files = {}
    for name, kw in (("plain", {}), ("exact", dict(exact=True)), ("crc", dict(checksum=True))):
        fn = str(d / (name + ".mua"))
        with archive.create(fn, C, S=S, hist_bits=6, seg_chunks=2, **kw) as w:
            t = 0
            for Tb in TB:
                w.append(rec[t:t + Tb])
                t += Tb
        files[name] = fn
    assert (rec > 2).sum() > 1000
    return files, np.ascontiguousarray(rec.T)


def _cut(x, triggers, pre, post, r):
    """int64 [n, rows, nb] from the [rows, T] recording"""
    W = pre + post
    nb = -(-W // r)
    g = x[:, (np.asarray(triggers, np.int64) - pre)[:, None] + np.arange(W)].astype(np.int64)
    g = np.concatenate([g, np.zeros(g.shape[:2] + (nb * r - W,), np.int64)], axis=2)
    return g.reshape(g.shape[0], g.shape[1], nb, r).sum(axis=3).transpose(1, 0, 2)


@pytest.mark.parametrize("bin_", [None, 1, 7, 50])
@pytest.mark.parametrize("channels", [None, [7, 0, 7]])
@pytest.mark.parametrize("kind", ["plain", "exact", "crc"])
def test_read_windows_against_the_recording(arcs, kind, channels, bin_):
    files, rec = arcs
    x = rec if channels is None else rec[channels]
    r = bin_ or 1
    clipped, true = _cut(np.minimum(x, S - 1), TRIGGERS, PRE, POST, r), _cut(x, TRIGGERS, PRE, POST, r)
    want = true if kind == "exact" else clipped
    with archive.open(files[kind]) as rd:
        got = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), np.minimum(want, 255))
        got = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_, saturate=False)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        s, q = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_, reduce="sum", moments=2)
        assert s.dtype == torch.int32 and q.dtype == torch.int64
        assert np.array_equal(s.cpu().numpy(), want.sum(axis=0)) and np.array_equal(q.cpu().numpy(), (want ** 2).sum(axis=0))
        s1 = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_, reduce="sum")
        assert np.array_equal(s1.cpu().numpy(), want.sum(axis=0))
        # several batches: a scratch of three windows' width at a time, the sums accumulate across them
        small = 3 * (PRE + POST) * x.shape[0]
        plan = windows.plan_spans(TRIGGERS - PRE, PRE + POST, T, budget=3 * (PRE + POST))
        assert len(plan.batches) > 3
        got = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_, saturate=False, max_bytes=small)
        assert np.array_equal(got.cpu().numpy(), want)
        s, q = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_, reduce="sum", moments=2, max_bytes=small, join=0)
        assert np.array_equal(s.cpu().numpy(), want.sum(axis=0)) and np.array_equal(q.cpu().numpy(), (want ** 2).sum(axis=0))
        if kind == "exact":
            got = rd.read_windows(TRIGGERS, PRE, POST, channels, bin=bin_, saturate=False, exact=False)
            assert np.array_equal(got.cpu().numpy(), clipped) and not np.array_equal(clipped, true)
        else:
            with pytest.raises(ValueError, match="exact=True"):
                rd.read_windows(TRIGGERS, PRE, POST, channels, exact=True)


def test_empty_lists_and_other_widths(arcs):
    files, rec = arcs
    with archive.open(files["plain"]) as rd:
        assert tuple(rd.read_windows([], 5, 5, bin=3).shape) == (0, C, 4)
        s, q = rd.read_windows([], 5, 5, [1, 2], reduce="sum", moments=2)
        assert tuple(s.shape) == tuple(q.shape) == (2, 10) and not s.any() and not q.any()
        assert tuple(rd.read_windows([100], 5, 5, channels=[]).shape) == (1, 0, 10)
        for pre, post in ((0, 1), (1, 0), (0, 40000), (25000, 25000)):      # one sample; windows wider than a block
            trig = [pre, T - post, 30000] if pre + post < 1000 else [30000]
            got = rd.read_windows(trig, pre, post, [3, 39], saturate=False)
            assert np.array_equal(got.cpu().numpy(), _cut(np.minimum(rec[[3, 39]], 2), trig, pre, post, 1))
        with pytest.raises(ValueError, match="wider than the budget"):
            rd.read_windows([30000], 100, 100, max_bytes=199 * C)


def test_every_span_is_read_once(arcs):
    files, rec = arcs
    trig = 21000 + 40 * np.random.RandomState(1).permutation(50)             # 50 windows inside one span
    a, b = int(trig.min()) - PRE, int(trig.max()) + POST
    plan = windows.plan_spans(trig - PRE, PRE + POST, T)
    assert len(plan.batches) == 1 and plan.batches[0].spans.tolist() == [[a, b]]
    with archive.open(files["plain"]) as one, archive.open(files["plain"]) as span, archive.open(files["plain"]) as loop:
        got = one.read_windows(trig, PRE, POST)
        span.read(a, b)
        for t in trig:
            loop.read(int(t) - PRE, int(t) + POST)
        assert one.bytes_read == span.bytes_read < loop.bytes_read
        assert np.array_equal(got.cpu().numpy(), _cut(np.minimum(rec, 2), trig, PRE, POST, 1))


def test_a_corrupt_segment_raises_what_read_raises(arcs, tmp_path):
    files, _rec = arcs
    fn = str(tmp_path / "flipped.mua")
    shutil.copy(files["crc"], fn)
    block, seg = 1, 2 * 3                  # channel 3's first segment of block 1: its steps 0 .. 32767
    with archive.open(files["crc"]) as rd:
        assert len(rd.block_file(block).seg_words) == 2 * C
        _flip_behind_a_chunk_header(fn, rd, block, seg)
    t = 20000 + 5000
    with archive.open(fn) as rd:
        with pytest.raises(ValueError) as by_read:
            rd.read(t - PRE, t + POST)
        with pytest.raises(ValueError) as by_windows:
            rd.read_windows([100, t], PRE, POST)
        assert str(by_read.value) == str(by_windows.value)
        assert "corrupt archive: checksum of segment %d of block %d " % (seg, block) in str(by_windows.value)
        assert tuple(rd.read_windows([100, t], PRE, POST, check=False).shape) == (2, C, PRE + POST)
        assert tuple(rd.read_windows([100, t], PRE, POST, channels=[0, 1]).shape) == (2, 2, PRE + POST)


@pytest.mark.parametrize("exact", [False, True])
def test_decompress_windows_on_a_ragged_container(exact, tmp_path):
    rng = np.random.RandomState(8)
    lens = [50000, 20000, 3 * muahuff.CHUNK + 5, 900]
    chans = [np.minimum(rng.poisson(0.6, n), 255).astype(np.uint8) for n in lens]
    c = muahuff.compress(chans, S=3, hist_bits=6, exact=exact)
    Tmax = max(lens)
    trig = np.array([19990, 49000, 100, 850, 19990, 3 * muahuff.CHUNK, 33000])     # past the ends of channels 1, 3 and 2
    path = str(tmp_path / "c.mh")
    cio.save(path, c)
    whole = cio.decompress_range(c, 0, Tmax).cpu().numpy()                  # zero-extended rows
    if exact:
        assert whole.max() > 2
    for channels in (None, [3, 1, 1]):
        x = whole if channels is None else whole[channels]
        for r in (None, 7):
            want = _cut(x, trig, PRE, POST, r or 1)
            with cio.open(path) as f:
                for src in (c, f, path):
                    got = cio.decompress_windows(src, trig, PRE, POST, channels, bin=r, saturate=False)
                    assert np.array_equal(got.cpu().numpy(), want)
                    s, q = cio.decompress_windows(src, trig, PRE, POST, channels, bin=r, reduce="sum", moments=2,
                                                  max_bytes=250 * x.shape[0])
                    assert np.array_equal(s.cpu().numpy(), want.sum(axis=0)) and np.array_equal(q.cpu().numpy(), (want ** 2).sum(axis=0))
    assert not whole[1, 20000:].any() and not whole[3, 900:].any() and whole[1, 19000:20000].any()
    with pytest.raises(ValueError, match="trigger %d:" % (Tmax - POST + 1)):
        cio.decompress_windows(c, [Tmax - POST + 1], PRE, POST)
