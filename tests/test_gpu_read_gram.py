"""archive.Reader.read_gram and container_io.decompress_gram on the GPU: the Gram matrix of a stored recording, walked in
batches, against NumPy's int64 product of what read() returns for the same whole bins -- ranges that start and stop
inside blocks and cross their boundaries, bins of 1, 5 and 50 samples, a channel subset, a plain and an exact archive,
at least three batches against one, the tail behind the last whole bin left out, and only the range's bytes read."""
import os

import numpy as np
import pytest
import torch

import muahuff
from muahuff import archive, gram
from muahuff import container_io as cio

pytestmark = pytest.mark.gpu

C, S = 24, 3
TB = [2 * muahuff.CHUNK + 700, 20000, 3 * muahuff.CHUNK + 5]       # three blocks of unequal length, a few chunks each
T = sum(TB)
B1, B2 = TB[0], TB[0] + TB[1]
# inside the first block; from inside the first across the second into the third; the whole recording
RANGES = [(100, 30000), (B1 - 5000, B2 + 7003), (0, T)]
SUBSET = [7, 0, 23, 7]


@pytest.fixture(scope="module")
def arcs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gram")
    rng = np.random.RandomState(21)
    rec = np.minimum(rng.poisson(0.3 + 0.05 * np.arange(C), size=(T, C)), 255).astype(np.uint8)
    rec[rng.rand(T, C) < 0.001] = 255
    files = {}
    for name, kw in (("plain", {}), ("exact", dict(exact=True))):
        fn = str(d / (name + ".mua"))
        with archive.create(fn, C, S=S, hist_bits=6, seg_chunks=2, **kw) as w:
            t = 0
            for Tb in TB:
                w.append(rec[t:t + Tb])
                t += Tb
        files[name] = fn
    return files


def _ref(x):
    x = x.astype(np.int64)
    return x @ x.T, x.sum(1)


def _check(res, want, n):
    assert isinstance(res, gram.Gram) and res.n == n and res.symmetric
    assert res.gram.dtype == torch.int64 and res.sum_a.dtype == torch.int64
    assert np.array_equal(res.gram.cpu().numpy(), want[0])
    assert np.array_equal(res.sum_a.cpu().numpy(), want[1]) and np.array_equal(res.sum_b.cpu().numpy(), want[1])


@pytest.mark.parametrize("bin_", [None, 5, 50])
@pytest.mark.parametrize("channels", [None, SUBSET])
@pytest.mark.parametrize("kind", ["plain", "exact"])
def test_read_gram_against_the_product_of_what_read_returns(arcs, kind, channels, bin_):
    r = bin_ or 1
    rows = C if channels is None else len(channels)
    with archive.open(arcs[kind]) as rd:
        assert rd.T == T
        for start, stop in RANGES:
            start -= start % r
            n = (stop - start) // r
            x = rd.read(start, start + n * r, channels, bin=bin_).cpu().numpy()
            assert x.dtype == np.uint8 and x.shape == (rows, n)
            want = _ref(x)
            one = rd.read_gram(start, stop, channels, bin=bin_)
            _check(one, want, n)
            # at least three batches: a scratch of a third of the bins, less a few
            small = rows * (n // 3 - 11)
            assert len(gram.batches(n, rows, small)) >= 3
            many = rd.read_gram(start, stop, channels, bin=bin_, max_bytes=small)
            _check(many, want, n)
            assert torch.equal(many.gram, one.gram)
        if kind == "exact":
            clipped = rd.read_gram(100, 30000, channels, exact=False)
            x = rd.read(100, 30000, channels, exact=False).cpu().numpy()
            _check(clipped, _ref(x), 29900)
            assert x.max() == S - 1
        else:
            with pytest.raises(ValueError, match="exact=True"):
                rd.read_gram(100, 30000, exact=True)


def test_the_tail_behind_the_last_whole_bin_is_left_out(arcs):
    with archive.open(arcs["plain"]) as rd:
        a = rd.read_gram(1000, 1000 + 50 * 100 + 49, bin=50)
        b = rd.read_gram(1000, 1000 + 50 * 100, bin=50)
        c = rd.read_gram(1000, 1000 + 50 * 101, bin=50)
        assert a.n == b.n == 100 and c.n == 101
        assert torch.equal(a.gram, b.gram) and torch.equal(a.sum_a, b.sum_a) and not torch.equal(a.gram, c.gram)
        # two disjoint ranges add up to the range over both
        both = rd.read_gram(1000, 1000 + 50 * 100, bin=50) + rd.read_gram(1000 + 50 * 100, 1000 + 50 * 101, bin=50)
        assert both.n == 101 and torch.equal(both.gram, c.gram) and torch.equal(both.sum_a, c.sum_a)
        empty = rd.read_gram(1000, 1049, bin=50)
        assert empty.n == 0 and not empty.gram.any() and tuple(empty.gram.shape) == (C, C)
        for kw in (dict(start=1001, stop=5000, bin=50), dict(start=0, stop=T + 1), dict(start=0, stop=100, bin=0)):
            with pytest.raises(ValueError):
                rd.read_gram(kw["start"], kw["stop"], bin=kw.get("bin"))
        with pytest.raises(IndexError):
            rd.read_gram(0, 100, channels=[C])


def test_a_short_range_reads_less_than_the_file(arcs):
    with archive.open(arcs["plain"]) as rd:
        before = rd.bytes_read
        rd.read_gram(B1 + 100, B1 + 3000, channels=[1, 2])
        assert 0 < rd.bytes_read - before and rd.bytes_read < os.path.getsize(arcs["plain"])


@pytest.mark.parametrize("exact", [False, True])
def test_decompress_gram_on_one_container(exact, tmp_path):
    rng = np.random.RandomState(8)
    lens = [50000, 20000, 3 * muahuff.CHUNK + 5, 900]
    chans = [np.minimum(rng.poisson(0.6, n), 255).astype(np.uint8) for n in lens]
    c = muahuff.compress(chans, S=3, hist_bits=6, exact=exact)
    Tmax = max(lens)
    path = str(tmp_path / "c.mh")
    cio.save(path, c)
    with cio.open(path) as f:
        for src in (c, f, path):
            for channels in (None, [3, 1, 1]):
                for r, start, stop in ((None, 0, None), (None, 19001, 49999), (5, 19000, 49999), (50, 0, None)):
                    a, b = start, Tmax if stop is None else stop
                    n = (b - a) // (r or 1)
                    if r is None:
                        x = cio.decompress_range(c, a, a + n, channels).cpu().numpy()
                    else:
                        x = cio.decompress_binned(c, r, a, a + n * r, channels).cpu().numpy()
                    want = _ref(x)
                    _check(cio.decompress_gram(src, start, stop, channels, bin=r), want, n)
                    small = x.shape[0] * (n // 3 - 7)
                    _check(cio.decompress_gram(src, start, stop, channels, bin=r, max_bytes=small), want, n)
