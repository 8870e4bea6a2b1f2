"""The recording archive without a GPU (archive.py): blocks encoded by the CPU oracle go in through append_compressed;
the index (trailer or prefix scan), the stored blocks and words, truncated files and appending to them, foreign blocks,
the global-range -> (block, local range) arithmetic and the argument errors of read()."""
import io
import os
import shutil

import numpy as np
import pytest

import muahuff
from muahuff import archive
from muahuff import container_io as cio
from tests import helpers, standins

CH = muahuff.CHUNK
C, S, SC = 5, 5, 1
LENS = (CH + 1, 40, 3 * CH + 7, 2 * CH, 100)
FIELDS = ("ch_len", "peak", "enc", "skipped", "ch_bits", "seg_words", "payload")


def _block(Tb, n_ch=C, S_=S, sc=SC, seed=0, window=3, tab=None, h=6):
    """one block from oracle.c.encode, as _container of tests/test_gpu_decode_rebin.py builds its container"""
    import oracle
    OC = oracle.c
    rng = np.random.RandomState(seed)
    tab = helpers.sclv_tables()[S_] if tab is None else tab
    chans = [np.minimum(rng.poisson(0.3 + 0.5 * ((i + seed) % 4), size=Tb), 255).astype(np.uint8) for i in range(n_ch)]
    data, off, ln = OC.flatten(chans)
    e = OC.encode(data, off, ln, OC.Params(S_, h, 1, window, tab, seg_chunks=sc))
    dense = standins.dense_words(e["payload"], e["seg"]["off"], e["seg_words"])
    return cio.Compressed(cio.make_header(S_, h, 1, window, sc, tab), np.full(n_ch, Tb, np.uint64), e["peak"].astype(np.uint8),
                          e["enc"].astype(np.uint8), np.zeros(n_ch, np.uint8), e["ch_bits"].astype(np.uint64),
                          e["seg_words"].astype(np.uint64), dense)


@pytest.fixture(scope="module")
def blocks():
    return [_block(Tb, seed=k) for k, Tb in enumerate(LENS)]


@pytest.fixture(scope="module")
def arc(blocks, tmp_path_factory):
    """(path of a closed five-block archive, its bytes); never written to again"""
    fn = str(tmp_path_factory.mktemp("arc") / "rec.mua")
    with archive.create(fn, C, S=S, sclv_rows=helpers.sclv_tables()[S], seg_chunks=SC, meta={"subject": "m1", "bp_ms": 1}) as w:
        for c in blocks:
            w.append_compressed(c)
        assert w.T == sum(LENS) and len(w.blocks) == len(LENS)
    with open(fn, "rb") as f:
        return fn, f.read()


def _same(a, b):
    strip = lambda h: {k: v for k, v in h.items() if k != "sizes"}  # noqa: E731  (read() keeps the array sizes write() added)
    assert strip(a.header) == strip(b.header)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f


def _check_index(a, blocks, n):
    assert len(a.blocks) == n and a.T == sum(LENS[:n])
    assert [b.Tb for b in a.blocks] == list(LENS[:n])
    assert [b.t_first for b in a.blocks] == [sum(LENS[:k]) for k in range(n)]
    peak, enc = a.words()
    assert peak.shape == enc.shape == (n, C) and peak.dtype == enc.dtype == np.uint8
    for k in range(n):
        _same(a.block(k), blocks[k])
        assert np.array_equal(peak[k], blocks[k].peak) and np.array_equal(enc[k], blocks[k].enc)


def test_reopen_gives_back_what_was_appended(arc, blocks):
    fn, raw = arc
    assert archive.is_archive(fn) and muahuff.archive is archive
    with archive.open(fn) as a:
        assert (a.C, a.S, a.truncated) == (C, S, False) and a.meta == {"subject": "m1", "bp_ms": 1}
        _check_index(a, blocks, len(LENS))
        for b, c in zip(a.blocks, blocks):
            assert raw[b.offset:b.offset + b.nbytes] == c.tobytes() and b.nbytes == cio.nbytes(c)
            with open(fn, "rb") as f:       # container_io.read positioned at the recorded offset
                f.seek(b.offset)
                _same(cio.read(f), c)
            with cio.ContainerFile(fn, offset=b.offset) as cf:      # and the lazy form
                assert cf.payload_words == c.payload.size and cf.header == cio.read(io.BytesIO(c.tobytes())).header
                assert np.array_equal(cf.seg_words, c.seg_words) and np.array_equal(cf.peak, c.peak)
                n = min(7, c.payload.size)
                assert np.array_equal(cf.read_words(c.payload.size - n, n), c.payload[c.payload.size - n:])
        # records are back to back behind the header, the trailer follows the last one
        pos = a.header_bytes
        for b in a.blocks:
            assert b.offset == pos + 32
            pos = b.offset + b.nbytes
        assert pos + a.trailer_bytes == len(raw)


def test_without_the_trailer_the_scan_finds_the_same_index(arc, blocks, tmp_path):
    fn, raw = arc
    with archive.open(fn) as a:
        want, end = list(a.blocks), a.blocks[-1].offset + a.blocks[-1].nbytes
    cut = str(tmp_path / "cut.mua")
    for tail in (b"", raw[end:end + 9], raw[end:-1]):   # no trailer, a trailer cut short
        with open(cut, "wb") as f:
            f.write(raw[:end] + tail)
        with archive.open(cut) as a:
            assert a.truncated and a.blocks == want
            _check_index(a, blocks, len(LENS))


def test_truncated_files_open_and_can_be_continued(arc, blocks, tmp_path):
    fn, raw = arc
    with archive.open(fn) as a:
        last = a.blocks[-1]
        want = list(a.blocks[:-1])
    rec = last.offset - 32
    cuts = [rec + 1, rec + 8, rec + 31, rec + 32, last.offset + 5, last.offset + 13, last.offset + last.nbytes // 2,
            last.offset + last.nbytes - 1]
    cut = str(tmp_path / "cut.mua")
    for at in cuts:
        with open(cut, "wb") as f:
            f.write(raw[:at])
        with archive.open(cut) as a:
            assert a.truncated and a.blocks == want, at
            _check_index(a, blocks, len(LENS) - 1)
        with archive.open(cut, "a") as w:
            assert w.T == sum(LENS[:-1]) and np.array_equal(w._word[0], blocks[-2].peak)
            w.append_compressed(blocks[-1])
        with open(cut, "rb") as f:
            assert f.read() == raw, at      # the old blocks byte for byte, and the file a closed archive again
    # appending to a closed archive replaces its trailer
    shutil.copy(fn, cut)
    extra = _block(777, seed=9)
    with archive.open(cut, "a") as w:
        w.append_compressed(extra)
    with open(cut, "rb") as f:
        now = f.read()
    end = last.offset + last.nbytes
    assert now[:end] == raw[:end]
    with archive.open(cut) as a:
        assert not a.truncated and a.T == sum(LENS) + 777 and a.blocks[:-1] == want + [last]
        _same(a.block(len(LENS)), extra)
    # an empty archive (header only, with or without a trailer) opens too
    with archive.create(cut, C, S=S, seg_chunks=SC):
        pass
    with archive.open(cut) as a:
        assert a.T == 0 and a.blocks == [] and not a.truncated
    with open(cut, "r+b") as f:
        f.truncate(os.path.getsize(cut) - 32)
    with archive.open(cut) as a:
        assert a.T == 0 and a.truncated
    with open(cut, "wb") as f:
        f.write(b"MUAHUFF1" + raw[8:])
    with pytest.raises(ValueError):
        archive.open(cut)


def test_a_foreign_block_is_refused(tmp_path):
    fn = str(tmp_path / "f.mua")
    tab = helpers.sclv_tables()[S]
    other = tab.copy()[::-1]
    assert other.tolist() != tab.tolist()
    foreign = dict(S=_block(50, S_=3), seg_chunks=_block(50, sc=2), sclv=_block(50, tab=other), window=_block(200, window=2),
                   channels=_block(50, n_ch=C + 1))
    ragged = _block(50)
    ragged.ch_len = ragged.ch_len.copy()
    ragged.ch_len[1] = 49
    with archive.create(fn, C, S=S, sclv_rows=tab, seg_chunks=SC) as w:
        for name, c in list(foreign.items()) + [("ragged", ragged)]:
            with pytest.raises(ValueError):
                w.append_compressed(c)
        good = _block(50)
        w.append_compressed(good)
    with archive.open(fn) as a:
        assert a.T == 50 and len(a.blocks) == 1
        _same(a.block(0), good)
    with pytest.raises(ValueError):
        archive.create(fn, C, S=S, seg_chunks=SC, recalibrate=0)


def test_block_ranges_match_brute_force():
    lens = np.array([5, 1, 9, 3, 7])
    t_first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    T = int(lens.sum())
    owner = np.repeat(np.arange(len(lens)), lens)
    local = np.concatenate([np.arange(n) for n in lens])
    edges = sorted({p for b in np.concatenate([[0], np.cumsum(lens)]) for p in (b - 1, b, b + 1) if 0 <= p <= T})
    assert len(edges) > 12
    for start in edges:
        for stop in edges:
            if stop < start:
                continue
            got = archive.block_ranges(t_first, lens, start, stop)
            want = []
            for i in np.unique(owner[start:stop]):
                t = local[start:stop][owner[start:stop] == i]
                want.append((int(i), int(t[0]), int(t[-1]) + 1))
            assert got == want, (start, stop)
    assert archive.block_ranges([], [], 0, 0) == []


def test_read_checks_its_arguments_before_any_device_work(arc):
    fn, _raw = arc
    with archive.open(fn) as a:
        for bad in (dict(start=5, stop=4), dict(start=0, stop=a.T + 1), dict(start=-1, stop=3), dict(start=0, stop=9, bin=0),
                    dict(start=0, stop=9, bin=4097), dict(start=7, stop=90, bin=5)):
            with pytest.raises(ValueError):
                a.read(**bad)
        with pytest.raises(IndexError):
            a.read(0, 10, channels=[C])
        before = a.bytes_read
        with pytest.raises(IndexError):
            a.read(0, 10, channels=[-1])
        assert a.bytes_read == before
