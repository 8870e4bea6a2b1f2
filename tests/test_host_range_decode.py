"""Random access in time without a GPU: the C ABI of mh_decode_range / mh_validate_segments, the segment-selection
arithmetic of container_io.range_segments against the planner's directory, argument errors before any device work,
ContainerFile's reads, and the pin of the range decoder's kernel instances in the shipped code object."""
import os
import re

import numpy as np
import pytest

import muahuff
from muahuff import _lib
from muahuff import container_io as cio
from tests import helpers, standins
from tests.test_host import _plan_query
from tests.test_host_kernel_cells import code_object_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = muahuff.CHUNK


def test_header_declares_the_range_calls_with_the_binding_prototypes():
    hdr = open(os.path.join(ROOT, "include", "muahuff.h")).read()
    ctype = {"mh_plan*": "p", "constuint32_t*": "p", "constuint64_t*": "p", "constuint8_t*": "p", "uint8_t*": "p",
             "void*": "p", "uint64_t": "u64", "uint32_t": "u32"}
    py = {_lib.ct.c_void_p: "p", _lib.ct.c_uint64: "u64", _lib.ct.c_uint32: "u32"}
    for name in ("mh_decode_range", "mh_validate_segments"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\);" % name, hdr)
        assert m, name
        kinds = [ctype[re.match(r"(.*?[\s*])\w+$", re.sub(r"\s+", " ", a.strip())).group(1).replace(" ", "")]
                 for a in m.group(1).split(",")]
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is _lib.ct.c_int and [py[a] for a in argtypes] == kinds, name
    # built on the host and uploaded: not in the list of calls that can be captured into a graph
    conv = hdr[:hdr.index("#ifndef MUAHUFF_H")]
    assert "mh_decode_range" not in conv[conv.index("`stream`"):conv.index("hipGraph")]
    assert int(re.search(r"#define\s+MH_VERSION\s+(\d+)", hdr).group(1)) == 103


def test_shipped_range_kernels(tmp_path):
    assert code_object_symbols(tmp_path, r"k_decode_range|k_range_fill") == {
        "void mh::k_decode_range<4, 4, 17, 1, false>(mh::RangeArgs)",
        "void mh::k_decode_range<2, 2, 25, 2, false>(mh::RangeArgs)",
        "void mh::k_decode_range<2, 2, 32, 0, false>(mh::RangeArgs)",
        "void mh::k_decode_range<2, 2, 31, 2, true>(mh::RangeArgs)",
        "mh::k_range_fill(unsigned char*, mh::RangeFill const*)",  # (no template: c++filt prints no return type)
    }


def _expected_runs(seg, lens, h, window, start, stop):
    """(first, end) per channel from the planner's directory: segments whose window samples meet [start, stop)."""
    w0, w1 = cio.window_bounds(lens, h, window)
    first, end = [], []
    for c in range(len(lens)):
        ids = np.nonzero(seg["ch"] == c)[0]
        a, b = max(start, int(w0[c])) - int(w0[c]), min(stop, int(w1[c])) - int(w0[c])
        hit = [int(s) for s in ids if a < b and int(seg["first"][s]) < b and int(seg["first"][s] + seg["n"][s]) > a]
        base = int(ids[0]) if ids.size else int(np.sum(seg["ch"] < c))
        if hit:
            assert hit == list(range(hit[0], hit[-1] + 1))   # one contiguous run
            first.append(hit[0])
            end.append(hit[-1] + 1)
        else:
            first.append(base)
            end.append(base)
    return np.array(first), np.array(end)


def _boundaries(lens, h, window, sc):
    """range ends on piece, row, chunk, segment and window boundaries of these channels (and one past them)"""
    w0, w1 = cio.window_bounds(lens, h, window)
    pts = {0, 1, max(lens)}
    for c in range(len(lens)):
        for base in (int(w0[c]), int(w0[c]) + (128 - int(w0[c]) % 128) % 128):
            for step in (16, 1024, CH, sc * CH):
                for k in (0, 1, 2, 3):
                    pts.update(p for p in (base + k * step - 1, base + k * step, base + k * step + 1) if 0 <= p <= max(lens))
        pts.update((int(w1[c]) - 1, int(w1[c]), lens[c]))
    return sorted(p for p in pts if 0 <= p <= max(lens))


@pytest.mark.parametrize("rev", [2, 3])
@pytest.mark.parametrize("window", [0, 1, 2, 3])
def test_range_segments_follow_the_planner_directory(rev, window):
    rng = np.random.RandomState(10 * rev + window)
    tab = helpers.sclv_tables()[3]
    heads = 0
    for h, sc, lens in ((2, 1, [16 * CH + 1000, 50000, 20 * CH + 3, 5]), (3, 2, [40 * CH + 7, 16 * CH, 3, 70001]),
                        (6, 3, [33 * CH + 100, 64, 65, 16 * CH + 64 + 5])):
        wflag = window | (_lib.WIN_REV2_SEGMENTS if rev == 2 else 0)
        rc, info, seg = _plan_query(lens, 3, h, 1, wflag, tab, sc)
        assert rc == 0
        # the one layout function against the planner: entries per channel, the head segment, the window they tile
        w0, w1, head, nseg = cio.channel_layout(lens, h, window, sc, rev)
        assert np.array_equal(nseg, np.bincount(seg["ch"], minlength=len(lens))) and int(nseg.sum()) == info.n_segments
        for c in range(len(lens)):
            ids = np.nonzero(seg["ch"] == c)[0]
            assert int(seg["n"][ids].sum()) == int(w1[c] - w0[c])
            assert np.array_equal(seg["first"][ids], np.cumsum(seg["n"][ids]) - seg["n"][ids])    # back to back from w0
            if head[c]:
                assert rev == 3 and int(seg["n"][ids[0]]) == int(head[c]) and (int(w0[c]) + int(head[c])) % 128 == 0
            elif ids.size:
                assert int(seg["n"][ids[0]]) == min(sc * CH, int(w1[c] - w0[c]))
        heads += int((head > 0).sum())
        # and its thin callers give the same
        assert all(np.array_equal(x, y) for x, y in zip(cio.window_bounds(lens, h, window), (w0, w1)))
        assert np.array_equal(cio.window_lengths(lens, h, window), w1 - w0)
        assert np.array_equal(cio.segments_per_channel(lens, h, window, sc, rev), nseg)
        pts = _boundaries(lens, h, window, sc)
        pairs = [(a, b) for a in pts[::3] for b in pts[::5] if a <= b] + [(0, max(lens))]
        pairs += [tuple(sorted(rng.randint(0, max(lens) + 1, size=2))) for _ in range(30)]
        for a, b in pairs:
            got = cio.range_segments(lens, h, window, sc, a, b, rev)
            want = _expected_runs(seg, lens, h, window, a, b)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (h, sc, a, b)
    assert (heads > 0) == (rev == 3 and window != 3)        # the layouts do have head segments where the format has them


def _oracle_container(lens, S, h, window, sc, rev=3, seed=0):
    import oracle
    OC = oracle.c
    rng = np.random.RandomState(seed)
    tab = helpers.sclv_tables()[S]
    chans = [np.minimum(rng.poisson(0.8, size=T), 255).astype(np.uint8) for T in lens]
    data, off, ln = OC.flatten(chans)
    wflag = window | (OC.WIN_REV2_SEGMENTS if rev == 2 else 0)
    e = OC.encode(data, off, ln, OC.Params(S, h, 1, wflag, tab, seg_chunks=sc))
    dense = standins.dense_words(e["payload"], e["seg"]["off"], e["seg_words"])
    hdr = cio.make_header(S, h, 1, window, sc, tab)
    hdr["format_revision"] = rev
    C = len(lens)
    c = cio.Compressed(hdr, np.array(lens, np.uint64), e["peak"].astype(np.uint8), e["enc"].astype(np.uint8),
                       np.zeros(C, np.uint8), np.zeros(C, np.uint64), e["seg_words"].astype(np.uint64), dense)
    return c, chans


def _validate_segments(c, payload, seg_off, segs):
    hd = c.header
    S, K = hd["S"], hd["K"]
    tab = np.ascontiguousarray(np.array(hd["sclv"], np.uint8))
    ch_len = np.ascontiguousarray(c.ch_len, np.uint64)
    sw = np.ascontiguousarray(c.seg_words, np.uint64)
    pay = np.ascontiguousarray(payload, np.uint32)
    segs = np.ascontiguousarray(segs, np.uint64)
    seg_off = np.ascontiguousarray(seg_off, np.uint64)
    return _lib.lib().mh_validate_segments(ch_len.ctypes.data, len(ch_len), S, hd["h"], hd["mode"], cio.plan_window(hd),
                                           tab.ctypes.data, K, hd["seg_chunks"], pay.ctypes.data, pay.size,
                                           seg_off.ctypes.data, sw.ctypes.data, sw.size, segs.ctypes.data, segs.size,
                                           np.ascontiguousarray(c.peak).ctypes.data, np.ascontiguousarray(c.enc).ctypes.data)


@pytest.mark.parametrize("rev", [2, 3])
def test_validate_segments_checks_exactly_the_listed_segments(rev):
    lens = [20 * CH + 3, 50000, 16 * CH + 1000, 70001]
    c, _ = _oracle_container(lens, 3, 6, 2, 2, rev)
    start, stop = 5 * CH + 11, 9 * CH + 400
    sel = np.array([2, 0])
    pay, seg_off, segs = cio.gather_range(c, start, stop, sel)
    assert segs.size and _validate_segments(c, pay, seg_off, segs) == 0
    # the whole stream segment by segment, in the stored layout, validates as mh_validate_stream does
    dense_off = np.concatenate([[0], np.cumsum(c.seg_words)[:-1]]).astype(np.uint64)
    assert _validate_segments(c, c.payload, dense_off, np.arange(len(c.seg_words))) == 0
    # corruption in a listed segment is named
    bad = pay.copy()
    s = int(segs[1])
    bad[int(seg_off[s])] ^= 0x3000                                  # field width of its first chunk header
    assert _validate_segments(c, bad, seg_off, segs) == _lib.ERR_STREAM
    assert ("segment %d" % s).encode() in _lib.lib().mh_last_error()
    short = pay[:-1]                                                # truncated
    assert _validate_segments(c, short, seg_off, segs) == _lib.ERR_STREAM
    # corruption outside the listed segments is not looked at
    full = c.payload.copy()
    other = [s_ for s_ in range(len(c.seg_words)) if s_ not in set(int(x) for x in segs)]
    for s_ in other:
        full[int(dense_off[s_])] ^= 0x3000
    assert _validate_segments(c, full, dense_off, segs) == 0
    assert _validate_segments(c, full, dense_off, np.arange(len(c.seg_words))) == _lib.ERR_STREAM
    # a bad (peak, enc) word of a channel whose segments are read
    pk = c.peak.copy()
    pk[2] = 3
    c2 = cio.Compressed(c.header, c.ch_len, pk, c.enc, c.skipped, c.ch_bits, c.seg_words, c.payload)
    assert _validate_segments(c2, pay, seg_off, segs) == _lib.ERR_STREAM and b"peak" in _lib.lib().mh_last_error()


def test_container_file_reads_only_what_a_query_needs(tmp_path):
    lens = [20 * CH + 3, 50000, 16 * CH + 1000, 70001, 33 * CH]
    c, _ = _oracle_container(lens, 3, 6, 2, 2, 3, seed=4)
    fn = str(tmp_path / "c.muahuff")
    cio.save(fn, c)
    hdr_len = int.from_bytes(open(fn, "rb").read(12)[8:12], "little")
    C, nseg = len(lens), len(c.seg_words)
    arrays = 8 * C + 3 * C + 8 * C + 8 * nseg
    with cio.open(fn) as f:
        assert f.bytes_read == f.head_bytes == 12 + hdr_len + arrays
        for name in ("ch_len", "peak", "enc", "skipped", "ch_bits", "seg_words"):
            assert np.array_equal(getattr(f, name), getattr(c, name)), name
        assert f.header["sizes"]["payload"] == c.payload.size == f.payload_words
        assert os.path.getsize(fn) > f.bytes_read + 4 * c.payload.size - 8
        for (start, stop, sel) in ((3 * CH + 5, 3 * CH + 1005, [4, 0, 0]), (0, max(lens), [1]), (10, 20, [3, 2]),
                                   (17 * CH, 17 * CH + 1, [0, 1, 2, 3, 4])):
            before = f.bytes_read
            pay, seg_off, segs = cio.gather_range(f, start, stop, np.array(sel))
            first, end = cio.range_segments(lens, 6, 2, 2, start, stop)
            want = sum(int(np.sum(c.seg_words[first[ch]:end[ch]])) for ch in set(sel))
            assert f.bytes_read - before == 4 * want == 4 * pay.size
            mem = cio.gather_range(c, start, stop, np.array(sel))
            assert np.array_equal(mem[0], pay) and np.array_equal(mem[1], seg_off) and np.array_equal(mem[2], segs)
            assert _validate_segments(c, pay, seg_off, segs) == 0


def test_range_argument_errors_come_before_any_device_work(tmp_path):
    """decompress_range checks the range and the channel list before it creates a plan (here there is no GPU: a plan
    would fail with MuaHuffError), and the api call does the same for a path."""
    lens = [20000, 50000, 3000]
    c, _ = _oracle_container(lens, 3, 6, 2, 1)
    fn = str(tmp_path / "c.muahuff")
    cio.save(fn, c)
    for src in (c, cio.open(fn)):
        with pytest.raises(ValueError):
            cio.decompress_range(src, 10, 5)
        with pytest.raises(ValueError):
            cio.decompress_range(src, 0, 50001)
        with pytest.raises(ValueError):
            cio.decompress_range(src, -1, 5)
        with pytest.raises(IndexError):
            cio.decompress_range(src, 0, 10, channels=[0, 3])
        with pytest.raises(IndexError):
            cio.decompress_range(src, 0, 10, channels=[-1])
    with pytest.raises(ValueError):
        muahuff.decompress(fn, start=7, stop=3)
    with pytest.raises(IndexError):
        muahuff.decompress(c, channels=[5], start=0, stop=3)
    # the C entry point rejects a NULL plan with a code and a message
    assert _lib.lib().mh_decode_range(None, None, 0, None, None, 0, 0, 0, None, None, None, 0, None) == _lib.ERR_ARG
    assert b"mh_decode_range" in _lib.lib().mh_last_error()


QUERY_OK = [  # (max_len, C, start, stop, channels, r) -> sel
    ((50000, 3, 0, 50000, None, None), [0, 1, 2]),
    ((50000, 3, 7, 7, None, None), [0, 1, 2]),                 # an empty range is a range
    ((50000, 3, 0, 10, [2, 0, 0], None), [2, 0, 0]),           # order and repeats are kept
    ((50000, 3, 0, 10, [], None), []),
    ((50000, 3, 0, 10, np.array([[1], [2]]), None), [1, 2]),   # any shape, flattened
    ((0, 0, 0, 0, None, None), []),                            # no channels at all
    ((50000, 3, 0, 9, None, 1), [0, 1, 2]),
    ((50000, 3, 4096, 50000, [1], 4096), [1]),
    ((50000, 3, 10, 90, None, 5), [0, 1, 2]),
    ((50000, 3, 0, 90, [], 7), []),
]
QUERY_BAD = [  # the cases of test_range_argument_errors_... here and test_read_checks_its_arguments_... of the archive
    ((50000, 3, 10, 5, None, None), ValueError), ((50000, 3, 0, 50001, None, None), ValueError),
    ((50000, 3, -1, 5, None, None), ValueError), ((50000, 3, 0, 10, [0, 3], None), IndexError),
    ((50000, 3, 0, 10, [-1], None), IndexError), ((50000, 3, 7, 3, None, None), ValueError),
    ((50000, 3, 0, 3, [5], None), IndexError),
    ((900, 5, 5, 4, None, None), ValueError), ((900, 5, 0, 901, None, None), ValueError), ((900, 5, -1, 3, None, None), ValueError),
    ((900, 5, 0, 9, None, 0), ValueError), ((900, 5, 0, 9, None, 4097), ValueError), ((900, 5, 7, 90, None, 5), ValueError),
    ((900, 5, 0, 10, [5], None), IndexError), ((900, 5, 0, 10, [-1], None), IndexError),
    # each rule of r on its own, and a bad argument next to a bad channel
    ((900, 5, 0, 9, None, -1), ValueError), ((900, 5, 1, 9, None, 2), ValueError), ((900, 5, 0, 9, [5], 0), ValueError),
    ((900, 5, 10, 5, [9], None), ValueError), ((0, 0, 0, 1, None, None), ValueError), ((0, 0, 0, 0, [0], None), IndexError),
]


def test_query_args_table():
    from muahuff import codec
    for args, want in QUERY_OK:
        sel = codec.query_args(*args)
        assert sel.dtype == np.int64 and sel.ndim == 1 and sel.tolist() == want, args
    for args, exc in QUERY_BAD:
        with pytest.raises(exc):
            codec.query_args(*args)


def test_head_parser_reads_what_container_file_reads(tmp_path):
    import io
    c, _ = _oracle_container([20000, 50000, 3000, 17 * CH + 5, 9], 3, 6, 2, 1)
    raw = c.tobytes()
    hdr, arrays, used = cio.read_head(io.BytesIO(raw).read)
    names = [name for name, _dt in cio.ARRAYS]
    assert names[-1] == "payload" and list(arrays) == names[:-1]
    assert used == len(raw) - 4 * c.payload.size - (-4 * c.payload.size % 8)
    for offset in (0, 32):
        fn = str(tmp_path / ("c%d.muahuff" % offset))
        with open(fn, "wb") as f:
            f.write(b"\xee" * offset + raw)
        with cio.ContainerFile(fn, offset) as cf:
            assert cf.header == hdr and cf.payload_offset == offset + used and cf.payload_words == c.payload.size
            for name in names[:-1]:
                a = arrays[name]
                assert a.dtype == getattr(c, name).dtype and np.array_equal(a, getattr(c, name)), name
                assert np.array_equal(getattr(cf, name), a), name
            # padding is passed over, not read: ContainerFile counts fewer bytes than the parser consumed
            pads = sum(-a.nbytes % 8 for a in arrays.values())
            assert cf.head_bytes == cf.bytes_read == used - pads and pads > 0
            assert np.array_equal(cf.read_words(0, c.payload.size), c.payload)
    # read() is the same parse followed by the payload
    back = cio.read(io.BytesIO(raw))
    assert back.header == hdr and np.array_equal(back.payload, c.payload)
    # a cut inside each array is named
    pos = 12 + int.from_bytes(raw[8:12], "little")
    for name, dt in cio.ARRAYS:
        size = int(hdr["sizes"][name]) * np.dtype(dt).itemsize
        assert size > 0
        for cut in (pos, pos + size // 2, pos + size - 1):
            src = io.BytesIO(raw[:cut])
            with pytest.raises(ValueError) as e:
                cio.read(src) if name == "payload" else cio.read_head(src.read)
            assert str(e.value) == "truncated container (%s)" % name, (name, cut)
        pos += size + (-size % 8)
    assert pos == len(raw)
