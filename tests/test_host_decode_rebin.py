"""Fused decode + re-bin, the parts that need no GPU: the exported symbol, the argument checks of the Python layers
(before any device is touched), the oracle expectation the GPU tests compare with, and the untouched bin=None path."""
import ctypes as ct

import numpy as np
import pytest

import muahuff
from muahuff import _lib, container_io as cio
from tests.test_host_range_decode import _oracle_container

CH = muahuff.CHUNK
LENS = [3 * CH + 77, 50000, 5]


def test_the_library_exports_mh_decode_rebin():
    so = ct.CDLL(_lib.SO)
    assert hasattr(so, "mh_decode_rebin")
    assert _lib.lib().mh_decode_rebin.argtypes and len(_lib.lib().mh_decode_rebin.argtypes) == 15
    assert _lib.lib().mh_version() == 103


def test_bad_arguments_are_rejected_before_any_device_work():
    c, _ = _oracle_container(LENS, 3, 6, 2, 2)
    T = max(LENS)
    for kw in (dict(r=5, start=3), dict(r=0), dict(r=4097), dict(r=-1), dict(r=5, start=10, stop=5),
               dict(r=5, start=0, stop=T + 1), dict(r=5, start=-5, stop=10)):
        with pytest.raises(ValueError):
            cio.decompress_binned(c, **kw)
    for ch in ([3], [-1], [0, 99]):
        with pytest.raises(IndexError):
            cio.decompress_binned(c, 5, channels=ch)
    with pytest.raises(ValueError):
        muahuff.decompress(c, start=3, stop=100, bin=5)
    with pytest.raises(ValueError):
        muahuff.decompress(c, bin=5000)


def test_the_oracle_expectation_is_a_reduceat_of_the_oracle_decode():
    """the yardstick of tests/test_gpu_decode_rebin.py restated in NumPy: reduceat over the zero-extended slice"""
    import oracle
    from tests.test_gpu_decode_rebin import _container, _want
    c, full = _container(LENS, 5, 6, 2, 2, seed=2)
    for (a, b, r) in ((0, max(LENS), 50), (100, 40001, 100), (CH, CH + 7, 7), (0, 4097, 4096), (20, 21, 1)):
        for saturate in (True, False):
            want = _want(full, [1, 0, 2], a, b, r, saturate)
            for i, ch in enumerate((1, 0, 2)):
                y = np.zeros(b - a, np.uint32)
                y[:len(full[ch][a:b])] = full[ch][a:b]
                s = np.add.reduceat(y, np.arange(0, b - a, r))
                assert np.array_equal(want[i], np.minimum(s, 255) if saturate else s), (a, b, r, ch)
    assert max(x.max() for x in full) == 4  # S = 5: clipped at S - 1


def test_bin_none_takes_the_old_path(monkeypatch):
    """decompress(..., bin=None) never reaches the new layers"""
    def boom(*a, **k):
        raise AssertionError("bin=None called the binned path")
    monkeypatch.setattr(cio, "decompress_binned", boom)
    seen = []
    monkeypatch.setattr(cio, "decompress_range", lambda *a, **k: seen.append((a[1:], k)) or _FakeRows())
    c, _ = _oracle_container(LENS, 3, 6, 2, 2)
    out = muahuff.decompress(c, channels=[1], start=4, stop=9)
    assert seen == [((4, 9), {"channels": [1]})] and len(out) == 1
    import inspect
    assert inspect.signature(muahuff.decompress).parameters["bin"].default is None


class _FakeRows:
    def cpu(self):
        return self

    def numpy(self):
        return np.zeros((1, 5), np.uint8)
