"""The walk over a stored stream (csrc/mh_validate.hpp: what mh_validate_stream and mh_validate_segments run behind
their NULL checks) as a host program under AddressSanitizer + UBSan, on streams made by the CPU oracle.  This is the
code that parses untrusted file bytes, so planner_check --validate holds every payload in a heap block of exactly its
words: a read of one word behind it ends the program.  Every case must leave the program with exit status 0, and its
codes AND messages must be the ones the built library gives through ctypes for the same arguments.  Runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from muahuff import _lib
from tests import helpers, standins
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

OC = oracle.c
LENS = [70001, 16384, 5, 40000, 16385 + 64, 100]
# (S, h, window, seg_chunks, lens): the three design points of test_validate_stream_accepts_oracle_streams_and_names_corruption,
# and one whose first channel has a head segment (a window of at least 16 chunks that starts at sample 2^6)
POINTS = [(3, 6, 2, 2, LENS), (5, 4, 0, 1, LENS), (10, 3, 3, 3, LENS), (3, 6, 2, 2, [16 * 16384 + 64 + 777, 16384, 5, 100])]
U64 = 2 ** 64


class Case:
    """the arguments of one stream walk and of the segment walks that go with it"""

    def __init__(self, name, lens, payload, seg_words, peak, enc, want=None, text=None):
        self.name, self.lens, self.want, self.text = name, list(lens), want, text
        self.payload = np.ascontiguousarray(payload, np.uint32)
        self.seg_words = np.ascontiguousarray(seg_words, np.uint64)
        self.peak, self.enc = np.ascontiguousarray(peak, np.uint8), np.ascontiguousarray(enc, np.uint8)
        # (null payload, seg_idx, seg_off, expected code or None): every segment at its dense offset, always
        dense_off = np.cumsum(self.seg_words, dtype=np.uint64) - self.seg_words
        self.walks = [(False, np.arange(self.seg_words.size, dtype=np.uint64), dense_off, want)]


def _stream(S, h, window, sc, lens):
    rng = np.random.RandomState(3)
    tab = helpers.sclv_tables()[S]
    chans = [np.minimum(rng.poisson(0.7, size=T), 255).astype(np.uint8) for T in lens]
    data, off, ln = OC.flatten(chans)
    e = OC.encode(data, off, ln, OC.Params(S, h, 1, window, tab, seg_chunks=sc))
    return tab, e, standins.dense_words(e["payload"], e["seg"]["off"], e["seg_words"])


def _cases(S, lens, e, dense):
    sw, pk, en = e["seg_words"].astype(np.uint64), e["peak"], e["enc"]
    nseg, ST, ARG = sw.size, _lib.ERR_STREAM, _lib.ERR_ARG
    cases = [Case("as made", lens, dense, sw, pk, en, 0)]
    base = cases[0]
    off = base.walks[0][2]
    some = np.unique(np.array([0, nseg // 2, nseg - 1], np.uint64))
    far, wrap, past = off.copy(), off.copy(), some.copy()
    far[some[-1]] = U64 - 1
    wrap[some[-1]] = U64 - int(sw[some[-1]])            # seg_off + seg_words == 2^64
    past[-1] = nseg
    base.walks += [(False, some, off, 0), (False, some[::-1], off, 0),
                   (False, some, far, ST), (False, some, wrap, ST), (False, past, off, ARG),
                   (True, np.zeros(0, np.uint64), off, 0)]
    # the damage test_validate_stream_accepts_oracle_streams_and_names_corruption applies
    bad = dense.copy()
    bad[0] ^= 0x3000
    cases.append(Case("field width of the first chunk header", lens, bad, sw, pk, en, ST))
    bad = dense.copy()
    bad[0] = (bad[0] & ~np.uint32(0xFFF)) | np.uint32(0xFFF)
    cases.append(Case("impossible minimum length", lens, bad, sw, pk, en, ST, "impossible"))
    cases.append(Case("cut by one word", lens, dense[:-1], sw, pk, en, ST, "ends at word"))
    more = sw.copy()
    more[0] += 1
    cases.append(Case("seg_words[0] + 1", lens, dense, more, pk, en, ST))
    cases.append(Case("a directory entry short", lens, dense, sw[:-1], pk, en, ST, "directory has"))
    high = pk.copy()
    high[0] = S
    cases.append(Case("peak = S", lens, dense, sw, high, en, ST, "peak"))
    cases.append(Case("another last channel", lens[:-1] + [101], dense, sw, pk, en))
    # further
    bad = dense.copy()
    bad[0] = 0xFFFFFFFF
    cases.append(Case("all-ones first header word", lens, bad, sw, pk, en, ST, "field width 15 above 12"))
    assert int(e["seg"]["n"][-1]) <= 16384 and int(sw[-1]) < 25     # the last chunk starts the last segment, which is short
    bad = dense.copy()
    last = dense.size - int(sw[-1])
    bad[last] = (bad[last] & ~np.uint32(0xF000)) | np.uint32(12 << 12)
    cases.append(Case("field width 12 in the last chunk", lens, bad, sw, pk, en, ST, "runs past the segment"))
    cases.append(Case("all-zero payload", lens, np.zeros_like(dense), sw, pk, en, ST, "impossible"))
    cases.append(Case("cut to no words", lens, dense[:0], sw, pk, en, ST, "segment 0 ends at word"))
    return cases


def _text(S, h, window, sc, tab, cases, tmp_path):
    out = []
    for i, c in enumerate(cases):
        fn = tmp_path / ("payload%d.u32" % i)
        c.payload.astype("<u4").tofile(str(fn))
        out.append("%d %d %d 1 %d %d %d  %s  %s" % (len(c.lens), S, h, window, len(tab), sc, " ".join(map(str, c.lens)),
                                                    " ".join(str(int(v)) for v in tab.ravel())))
        out.append("%d %s" % (c.seg_words.size, " ".join(map(str, c.seg_words))))
        out.append(" ".join(map(str, c.peak)) + "  " + " ".join(map(str, c.enc)))
        out.append("%d @%s" % (c.payload.size, fn))
        out.append(str(len(c.walks)))
        for null, idx, off, _ in c.walks:
            out.append("%d %d %s  %s" % (null, idx.size, " ".join(map(str, idx)), " ".join(str(int(o)) for o in off[:c.seg_words.size])))
    return "\n".join(out) + "\n"


def _library(S, h, window, sc, tab, c):
    """[(code, message)] of mh_validate_stream and of mh_validate_segments per walk, from the built library"""
    L = _lib.lib()
    ch_len = np.array(c.lens, np.uint64)
    pad = c.payload if c.payload.size else np.zeros(1, np.uint32)
    head = (ch_len.ctypes.data, len(ch_len), S, h, 1, window, tab.ctypes.data, len(tab), sc)
    rc = L.mh_validate_stream(*head, pad.ctypes.data, c.payload.size, c.seg_words.ctypes.data, c.seg_words.size,
                              c.peak.ctypes.data, c.enc.ctypes.data)
    got = [(rc, L.mh_last_error().decode() if rc else "")]
    for null, idx, off, _ in c.walks:
        off = np.ascontiguousarray(off[:c.seg_words.size], np.uint64)
        idx = np.ascontiguousarray(idx, np.uint64)
        rc = L.mh_validate_segments(*head, None if null else pad.ctypes.data, c.payload.size, off.ctypes.data,
                                    c.seg_words.ctypes.data, c.seg_words.size, None if null else idx.ctypes.data, idx.size,
                                    c.peak.ctypes.data, c.enc.ctypes.data)
        got.append((rc, L.mh_last_error().decode() if rc else ""))
    return got


@pytest.mark.parametrize("point", range(len(POINTS)))
def test_stream_walks_under_sanitizers_agree_with_the_library(exe, tmp_path, point):  # noqa: F811
    S, h, window, sc, lens = POINTS[point]
    tab, e, dense = _stream(S, h, window, sc, lens)
    tab = np.ascontiguousarray(tab, np.uint8)
    if point == 3:      # the head segment: samples up to the next multiple of 128, a directory entry of its own
        assert int(e["seg"]["first"][0]) == 0 and int(e["seg"]["n"][0]) == 64 and int(e["seg"]["first"][1]) == 64
    cases = _cases(S, lens, e, dense)
    r = subprocess.run([exe, "--validate"], input=_text(S, h, window, sc, tab, cases, tmp_path), capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]          # no sanitizer report on any case
    lines = iter(r.stdout.splitlines())
    for c in cases:
        want = _library(S, h, window, sc, tab, c)
        for k, (rc_lib, msg_lib) in enumerate(want):
            tag, rc, msg = (next(lines) + " ").split(" ", 2)
            assert tag == ("G" if k else "S"), (c.name, k)
            assert (int(rc), msg.strip()) == (rc_lib, msg_lib), (c.name, k)
            expect = c.walks[k - 1][3] if k else c.want
            if expect is not None:
                assert int(rc) == expect, (c.name, k, msg)
            if k == 0 and c.text:
                assert c.text in msg, (c.name, msg)
    assert next(lines, None) is None
