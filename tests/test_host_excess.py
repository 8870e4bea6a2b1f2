"""Exact counts without a GPU (mhi_excess_scratch_bytes / _count / _emit / _apply, include/muahuff_ingest.h; the
container's exc_seg / exc_pos / exc_val): the ABI's three descriptions agree, every argument error comes back before a
pointer is used, the scratch size is host arithmetic and equals what tests/excess_layout_check.cpp --
csrc/mh_excess_layout.hpp built alone under AddressSanitizer + UBSan -- prints, and the container format round-trips,
leaves a plain container and the bytes ch_len .. payload alone, and refuses damaged lists.  The lists are made in NumPy
on a container from the oracle."""
import ctypes as ct
import importlib
import io
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import muahuff
from muahuff import _ingest, _lib, excess
from muahuff import container_io as cio
from tests.test_host_range_decode import _oracle_container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "excess_layout_check.cpp")
FIELDS = ("tile", "tile_t", "strip", "channels", "length", "per_channel", "pieces", "groups", "strips", "off_sum", "off_base",
          "off_partial", "bytes", "waves", "grid", "grid_scan")
ROWS, COLS = 0, 1
CH = muahuff.CHUNK
NAMES = ("mhi_excess_scratch_bytes", "mhi_excess_count", "mhi_excess_emit", "mhi_excess_apply")


@pytest.fixture(scope="module", autouse=True)
def built():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()


# ---- header, map, prototypes ---------------------------------------------------------------------------------------
def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_ingest.h")).read()
    declared = set(re.findall(r"\b(mhi_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ingest.PROTOTYPES) and set(NAMES) <= declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _ingest.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[-1].startswith("mhi_")}
    assert exported == declared
    assert "mhi_*" in open(os.path.join(CSRC, "exports_ingest.map")).read()
    assert "#define MHI_EXCESS_ROWS 0u" in hdr and "#define MHI_EXCESS_COLS 1u" in hdr
    assert (_ingest.EXCESS_ROWS, _ingest.EXCESS_COLS) == (ROWS, COLS)
    # the argument counts of the header are those of the ctypes prototypes
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
        assert len(args.split(",")) == len(_ingest.PROTOTYPES[name][1]), name
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_excess.hpp", "csrc/mh_excess_layout.hpp"} <= set(build.INGEST_HEADERS)


# ---- scratch bytes and the layout ----------------------------------------------------------------------------------
def scratch_bytes(form, rows, cols):
    b = ct.c_uint64(0)
    rc = _ingest.lib().mhi_excess_scratch_bytes(form, rows, cols, ct.byref(b))
    return rc, b.value


def test_scratch_bytes_is_nonzero_and_monotone():
    for form in (ROWS, COLS):
        prev_r = 0
        for rows in (1, 2, 3, 511, 512, 513, 1024, 4097, 40000, 10 ** 6):
            prev_c = 0
            for cols in (1, 3, 255, 256, 257, 1024, 16383, 16384, 16385, 10 ** 6):
                rc, b = scratch_bytes(form, rows, cols)
                assert rc == _lib.MH_OK and b > 0 and b % 16 == 0 and b >= prev_c, (form, rows, cols)
                prev_c = b
            assert prev_c >= prev_r
            prev_r = prev_c
        for cols in (1, 257, 16385):
            sizes = [scratch_bytes(form, rows, cols)[1] for rows in (1, 2, 511, 512, 513, 1025, 10 ** 6)]
            assert sizes == sorted(sizes) and sizes[0] > 0
    assert _ingest.excess_scratch_bytes(ROWS, 3, 100) == scratch_bytes(ROWS, 3, 100)[1]


def test_scratch_bytes_argument_errors():
    L = _ingest.lib()
    assert L.mhi_excess_scratch_bytes(ROWS, 3, 100, None) == _lib.ERR_ARG
    for form, rows, cols in ((2, 3, 100), (7, 3, 100), (ROWS, 0, 100), (ROWS, 3, 0), (COLS, 0, 5), (COLS, 5, 0),
                             (ROWS, 3, 1 << 32), (COLS, 3, 1 << 32), (COLS, 1 << 32, 3), (ROWS, 1 << 32, 16385),
                             (COLS, (1 << 32) - 1, 1 << 20)):
        rc, _ = scratch_bytes(form, rows, cols)
        assert rc == _lib.ERR_ARG and "mhi_excess_scratch_bytes" in L.mhi_last_error().decode(), (form, rows, cols)
    assert scratch_bytes(ROWS, 1 << 13, (1 << 32) - 1)[0] == _lib.MH_OK      # the longest channel that is taken
    assert scratch_bytes(COLS, (1 << 32) - 1, 511)[0] == _lib.MH_OK


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("excess") / "excess_layout_check_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, SRC, "-o", out])
    return out


def _run(exe_path, text):
    r = subprocess.run([exe_path], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_scratch_bytes_is_the_layout_program_under_the_sanitizers(exe):
    around = lambda x: [x - 1, x, x + 1]     # noqa: E731
    grid = []
    for cols in [1, 15, 16, 17] + around(16384) + around(2 * 16384) + [10 ** 7, (1 << 32) - 1]:
        for rows in (1, 3, 1023, 1024, 1025):
            grid.append((ROWS, rows, cols))
    for T in [1, 255] + around(512) + around(1024) + [4097, 40000, 10 ** 6, (1 << 32) - 1]:
        for C in [1, 3, 64, 130] + around(256) + around(512) + [1024]:
            grid.append((COLS, T, C))
    lines = _run(exe, "".join("%d %d %d\n" % t for t in grid))
    assert len(lines) == len(grid) > 150
    for (form, rows, cols), ln in zip(grid, lines):
        rc, b = scratch_bytes(form, rows, cols)
        if ln.startswith("error"):
            assert rc == _lib.ERR_ARG, (form, rows, cols)
            continue
        lay = dict(zip(FIELDS, (int(v) for v in ln.split())))
        assert rc == _lib.MH_OK and b == lay["bytes"] > 0, (form, rows, cols, b, lay)
        assert (lay["tile"], lay["tile_t"], lay["strip"]) == (16384, 512, 256)
        want = rows * -(-cols // 16384) if form == ROWS else cols * -(-rows // 512)
        assert lay["pieces"] == want and lay["groups"] == -(-want // 1024)
    bad = _run(exe, "2 5 5\n0 0 5\n1 5 0\n0 5 4294967296\n1 4294967296 5\n8589934592 5 5\n")
    assert bad == ["error -1"] * 6
    assert _run(exe, "apply 0 100 7 3\napply 5 5 1 0\napply 0 4294967296 4294967296 4294967295\napply 10 4106 4096 0\n") == \
        ["15", "0", "2", "1"]


def test_the_grids_are_the_rule_restated(exe):
    """count / emit: workgroups of 4 waves -- a wave per piece in the ROWS form, a wave per (strip of 256 channels, time
    tile) in the COLS form; the scan's two group kernels: a workgroup per 1024 pieces.  None is capped -- the layout
    refuses more than 2^32 - 1 pieces"""
    grid = [(ROWS, rows, cols) for cols in (1, 16384, 16385, 10 ** 7, (1 << 32) - 1) for rows in (1, 3, 4, 5, 1023, 1025)]
    grid += [(COLS, T, C) for T in (1, 512, 513, 4097, 10 ** 6, (1 << 32) - 1) for C in (1, 255, 256, 257, 1023, 1025)]
    grid += [(ROWS, (1 << 32) - 1, 16384), (COLS, (1 << 32) - 1, 511)]
    lines = _run(exe, "".join("%d %d %d\n" % t for t in grid))
    assert sum(ln.startswith("error") for ln in lines) == 2        # 2^32 - 1 time steps of 1023 and of 1025 channels
    for (form, rows, cols), ln in zip(grid, lines):
        if ln.startswith("error"):
            continue
        lay = dict(zip(FIELDS, (int(v) for v in ln.split())))
        pieces = rows * -(-cols // 16384) if form == ROWS else cols * -(-rows // 512)
        waves = 0 if form == ROWS else -(-cols // 256) * -(-rows // 512)
        assert lay["waves"] == waves and lay["grid_scan"] == -(-pieces // 1024), (form, rows, cols, lay)
        assert lay["grid"] == -(-(pieces if form == ROWS else waves) // 4), (form, rows, cols, lay)


def test_the_check_program_and_the_library_give_the_same_codes_and_messages(exe):
    """every row of tests/test_host_ingest_messages.py for the four entry points -- 2^32, 2^63 and 2^64 - 1 among the
    values -- through mh_excess_layout.hpp's checks under the sanitizers"""
    from tests import test_host_ingest_messages as pinned
    refused, accepted = pinned.check_program_agrees(exe, *NAMES)
    assert refused >= 2 * len(SHARED_BAD) + len(APPLY_BAD) + 11 and accepted >= 10
    # what the apply check hands the launch: the elements of a row and its runs of 32
    assert _run(exe, "check apply 4 1 8 1 1 2 0 50 5 0 1 8 16 4\ncheck apply 4 1 8 1 1 2 10 4106 1 0 1 8 16 4\n"
                     "check apply 4 1 0 1 1 2 0 50 5 0 1 8 16 4\n") == ["ok 10 1", "ok 4096 128", "ok 0 0"]


# ---- argument errors -----------------------------------------------------------------------------------------------
def _buffers(rows, cols):
    need = scratch_bytes(ROWS, rows, cols)[1]
    keep = dict(inp=np.zeros(rows * cols + 64, np.uint8), row_off=np.zeros(rows + 2, np.uint64), lo=np.zeros(rows + 2, np.uint64),
                hi=np.zeros(rows + 2, np.uint64), exc_off=np.zeros(max(rows, cols) + 3, np.uint64), total=np.zeros(2, np.uint64),
                pos=np.zeros(64, np.uint32), val=np.zeros(64, np.uint8), over=np.zeros(2, np.uint64),
                first=np.zeros(8, np.uint64), last=np.zeros(8, np.uint64), out=np.zeros(64, np.uint32),
                scratch=np.zeros(need // 8 + 4, np.uint64))
    ptr = {k: ct.c_void_p(v.ctypes.data + (-v.ctypes.data) % 16) for k, v in keep.items()}
    return keep, ptr


def _gen(which, form=ROWS, rows=3, cols=100, threshold=2, short=0, misalign=0, tables="fits", **null):
    """mhi_excess_count / _emit with host stand-ins for the device buffers: an argument error must come back before any
    of them is used as a device pointer.  null: name=None for a NULL pointer."""
    keep, ptr = _buffers(3, 100)
    need = scratch_bytes(form, rows, cols)[1] if form in (ROWS, COLS) and scratch_bytes(form, rows, cols)[0] == 0 else 1 << 20
    if tables == "fits" and form == COLS:
        ptr["row_off"] = ptr["lo"] = ptr["hi"] = None
    for k in null:
        ptr[k] = None
    L = _ingest.lib()
    sc = ct.c_void_p(ptr["scratch"].value + misalign) if ptr["scratch"] else None
    if which == "count":
        rc = L.mhi_excess_count(form, ptr["inp"], ptr["row_off"], ptr["lo"], ptr["hi"], rows, cols, threshold, ptr["exc_off"],
                                ptr["total"], sc, need - short, None)
    else:
        rc = L.mhi_excess_emit(form, ptr["inp"], ptr["row_off"], ptr["lo"], ptr["hi"], rows, cols, threshold, ptr["pos"],
                               ptr["val"], 8, ptr["over"], sc, need - short, None)
    del keep
    return rc, L.mhi_last_error().decode()


SHARED_BAD = [dict(inp=None), dict(row_off=None), dict(scratch=None), dict(form=2), dict(form=7),
              dict(form=COLS, tables="given"), dict(form=COLS, tables="given", lo=None, hi=None),
              dict(form=COLS, tables="given", row_off=None, hi=None), dict(threshold=0), dict(threshold=255),
              dict(threshold=256), dict(form=COLS, threshold=0), dict(rows=0), dict(cols=0), dict(cols=1 << 32),
              dict(cols=(1 << 32) + 5), dict(form=COLS, cols=1 << 32), dict(form=COLS, rows=1 << 32),
              dict(rows=1 << 32, cols=16385), dict(short=1), dict(form=COLS, short=16), dict(misalign=8)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items())   # noqa: E731


@pytest.mark.parametrize("bad", SHARED_BAD + [dict(exc_off=None), dict(total=None), dict(form=COLS, total=None)], ids=_ids)
def test_count_argument_errors_come_before_any_device_work(bad):
    rc, msg = _gen("count", **bad)
    assert rc == _lib.ERR_ARG, (rc, msg)
    assert "mhi_excess_count" in msg, msg


@pytest.mark.parametrize("bad", SHARED_BAD + [dict(pos=None), dict(val=None), dict(over=None), dict(form=COLS, over=None)], ids=_ids)
def test_emit_argument_errors_come_before_any_device_work(bad):
    rc, msg = _gen("emit", **bad)
    assert rc == _lib.ERR_ARG, (rc, msg)
    assert "mhi_excess_emit" in msg, msg


APPLY_BAD = [dict(pos=None), dict(val=None), dict(first=None), dict(last=None), dict(out=None), dict(out_bits=0),
             dict(out_bits=16), dict(out_bits=64), dict(r=0), dict(r=(1 << 32) + 1), dict(lead=1 << 32), dict(start=9, stop=8),
             dict(stop=(1 << 32) + 1), dict(out_bits=32, row_stride=6), dict(out_bits=32, col_stride=1),
             dict(out_bits=32, out_shift=2), dict(pos_shift=1)]


@pytest.mark.parametrize("bad", APPLY_BAD, ids=_ids)
def test_apply_argument_errors_come_before_any_device_work(bad):
    keep, ptr = _buffers(3, 100)
    a = dict(start=0, stop=50, r=5, lead=0, out_bits=8, row_stride=16, col_stride=4, out_shift=0, pos_shift=0)
    for k, v in bad.items():
        if k in a:
            a[k] = v
        else:
            ptr[k] = None
    L = _ingest.lib()
    out = ct.c_void_p(ptr["out"].value + a["out_shift"]) if ptr["out"] else None
    pos = ct.c_void_p(ptr["pos"].value + a["pos_shift"]) if ptr["pos"] else None
    rc = L.mhi_excess_apply(pos, ptr["val"], 8, ptr["first"], ptr["last"], 2, a["start"], a["stop"], a["r"], a["lead"], out,
                            a["out_bits"], a["row_stride"], a["col_stride"], None)
    msg = L.mhi_last_error().decode()
    assert rc == _lib.ERR_ARG and "mhi_excess_apply" in msg, (rc, msg)


def test_apply_of_nothing_enqueues_nothing():
    """n_rows == 0, n_entries == 0 and start == stop return MH_OK with host stand-ins: no launch is tried"""
    keep, ptr = _buffers(3, 100)
    L = _ingest.lib()
    f = lambda n_entries, n_rows, start, stop: L.mhi_excess_apply(ptr["pos"], ptr["val"], n_entries, ptr["first"], ptr["last"],   # noqa: E731
                                                                 n_rows, start, stop, 1, 0, ptr["out"], 8, 16, 1, None)
    assert f(0, 2, 0, 50) == f(8, 0, 0, 50) == f(8, 2, 7, 7) == _lib.MH_OK


# ---- the container -------------------------------------------------------------------------------------------------
LENS = [20000, 50000, 3000, 17 * CH + 5, 9]


def _lists(c, chans):
    """(exc_off, pos, val) of the channels' encoded windows in NumPy -- the oracle's container holds min(x, S-1) of
    `chans`, whatever they are, so the test is free to say what the original counts were: chans with 255s planted"""
    hd = c.header
    thr = hd["S"] - 1
    w0, w1 = cio.window_bounds(c.ch_len, hd["h"], hd["window"])
    pos, val, off = [], [], [0]
    for x, a, b in zip(chans, w0, w1):
        p = np.nonzero(x[a:b].astype(np.int64) > thr)[0] + a
        pos.append(p), val.append(x[p].astype(np.int64) - thr)
        off.append(off[-1] + len(p))
    return np.array(off), np.concatenate(pos).astype(np.uint32), np.concatenate(val).astype(np.uint8)


@pytest.fixture(scope="module")
def trio():
    """(plain container, the same with lists, its original channels): five channels, S = 3, window after calibration,
    two chunks per segment"""
    c, chans = _oracle_container(LENS, 3, 6, 2, 2)
    rng = np.random.RandomState(11)
    orig = []
    for x in chans:
        x = x.copy()
        hot = x >= 2
        x[hot] = np.minimum(2 + rng.poisson(0.7, int(hot.sum())), 255)   # min(orig, 2) == the encoded channel
        orig.append(x)
    orig[1][[64, 2 * CH + 63, 2 * CH + 64, 49999]] = 255                  # first / last sample of window, segment
    e = cio.Compressed(dict(c.header, exact=True), c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words, c.payload)
    cio.attach_excess(e, *_lists(c, orig))
    return c, e, orig


def _with_crc(c):
    out = cio.Compressed(dict(c.header, format_revision=4), c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words,
                         c.payload, cio.seg_crc_host(c), c.exc_seg, c.exc_pos, c.exc_val)
    return out


def test_lists_are_indexed_by_segment(trio):
    c, e, orig = trio
    n = len(e.exc_pos)
    assert n > 50 and e.excess_bits == 40 * n + 64 * (len(c.seg_words) + 1) and c.excess_bits == 0
    ch, lo, hi = excess.segment_bounds(c.ch_len, 6, 2, 2, 3)
    seg = e.exc_seg.astype(np.int64)
    assert len(seg) == len(c.seg_words) + 1 and seg[0] == 0 and seg[-1] == n
    total = 0
    for s in range(len(c.seg_words)):
        x = orig[ch[s]][lo[s]:hi[s]].astype(np.int64)
        want = np.nonzero(x > 2)[0] + lo[s]
        assert np.array_equal(e.exc_pos[seg[s]:seg[s + 1]], want)
        assert np.array_equal(e.exc_val[seg[s]:seg[s + 1]], x[want - lo[s]] - 2)
        total += len(want)
    assert total == n
    excess.check_container(e)


def test_round_trip_through_bytes_and_file(trio, tmp_path):
    c, e, _ = trio
    for src in (e, _with_crc(e)):
        blob = src.tobytes()
        assert len(blob) == cio.nbytes(src)
        back = cio.read(io.BytesIO(blob))
        assert back.header["exact"] is True
        for name in ("exc_seg", "exc_pos", "exc_val", "payload", "seg_words", "ch_len"):
            assert np.array_equal(getattr(back, name), getattr(src, name)), name
        assert (back.exc_seg.dtype, back.exc_pos.dtype, back.exc_val.dtype) == (np.uint64, np.uint32, np.uint8)
        assert back.tobytes() == blob
        path = tmp_path / "e.mh"
        cio.save(path, src)
        with cio.open(path) as f:
            assert f.bytes_read == f.head_bytes < len(blob) - src.payload.nbytes     # the lists stay on disk
            assert np.array_equal(f.exc_seg, src.exc_seg)
            p, v = f.read_excess(3, 20)
            assert np.array_equal(p, src.exc_pos[3:23]) and np.array_equal(v, src.exc_val[3:23])
            f.verify_excess()
        assert np.array_equal(cio.load(path).exc_pos, src.exc_pos)
    hdr = json.loads(_with_crc(e).tobytes()[12:12 + struct.unpack("<I", _with_crc(e).tobytes()[8:12])[0]])
    assert hdr["excess_crc32"] == excess.crc32(e.exc_seg, e.exc_pos, e.exc_val) and hdr["format_revision"] == 4
    assert cio.READ_REVISIONS == (2, 3, 4) and e.header["format_revision"] == 3


def _split(blob):
    n = struct.unpack("<I", blob[8:12])[0]
    return json.loads(blob[12:12 + n]), blob[12 + n:]


def test_plain_container_is_unchanged_and_the_stream_bytes_are_shared(trio):
    c, e, _ = trio
    hdr, body = _split(c.tobytes())
    assert "exact" not in hdr and "excess_crc32" not in hdr and set(hdr["sizes"]) == {n for n, _ in cio.ARRAYS}
    # what revision 3 has always written: the header of make_header + sizes, the arrays of ARRAYS, nothing else
    want = dict(cio.make_header(3, 6, 1, 2, 2, np.array(hdr["sclv"], np.uint8)), sizes=hdr["sizes"])
    assert hdr == want
    pad8 = lambda b: b + (-b % 8)  # noqa: E731
    assert len(body) == sum(pad8(hdr["sizes"][n] * np.dtype(dt).itemsize) for n, dt in cio.ARRAYS)
    ehdr, ebody = _split(e.tobytes())
    assert ehdr["exact"] is True and {k: v for k, v in ehdr.items() if k not in ("exact", "sizes")} == \
        {k: v for k, v in hdr.items() if k != "sizes"}
    assert ebody[:len(body)] == body                      # ch_len .. payload, byte for byte
    assert len(ebody) == len(body) + sum(pad8(ehdr["sizes"][n] * np.dtype(dt).itemsize) for n, dt in cio.EXCESS)
    pc, pe = _with_crc(c), _with_crc(e)
    (h4, b4), (e4, eb4) = _split(pc.tobytes()), _split(pe.tobytes())
    assert eb4[:len(b4)] == b4 and h4["arrays_crc32"] == e4["arrays_crc32"] and "excess_crc32" not in h4


def _damaged(e, **over):
    d = cio.Compressed(e.header, e.ch_len, e.peak, e.enc, e.skipped, e.ch_bits, e.seg_words, e.payload, e.seg_crc,
                       e.exc_seg.copy(), e.exc_pos.copy(), e.exc_val.copy())
    for k, f in over.items():
        setattr(d, k, f(getattr(d, k)))
    return d


def _swap(a, i, j):
    a[[i, j]] = a[[j, i]]
    return a


def _set(i, v):
    def f(a):
        a[i] = v
        return a
    return f


def test_damaged_lists_are_refused(trio, tmp_path):
    c, e, orig = trio
    seg = e.exc_seg.astype(np.int64)
    s = int(np.nonzero(np.diff(seg) >= 2)[0][0])           # a segment with two entries or more
    k = int(np.nonzero(np.diff(seg) >= 1)[0][-1])          # the last one with any
    _ch, lo, hi = excess.segment_bounds(c.ch_len, 6, 2, 2, 3)
    cases = {
        "non-monotone exc_seg": _damaged(e, exc_seg=lambda a: _swap(a, s, s + 1)),
        "index past n": _damaged(e, exc_seg=_set(-1, len(e.exc_pos) + 1)),
        "index past n inside": _damaged(e, exc_seg=_set(k + 1, len(e.exc_pos) + 7)),
        "first index not 0": _damaged(e, exc_seg=_set(0, 1)),
        "short exc_seg": _damaged(e, exc_seg=lambda a: a[:-1]),
        "position outside its segment": _damaged(e, exc_pos=_set(seg[s], int(hi[s]))),
        "position in front of its segment": _damaged(e, exc_pos=_set(seg[k], int(lo[k]) - 1)),
        "positions that do not ascend": _damaged(e, exc_pos=lambda a: _swap(a, seg[s], seg[s] + 1)),
        "value 0": _damaged(e, exc_val=_set(5, 0)),
        "value past 255": _damaged(e, exc_val=_set(5, 254)),
        "lists of different lengths": _damaged(e, exc_val=lambda a: a[:-1]),
    }
    for what, d in cases.items():
        with pytest.raises(ValueError):
            excess.check_container(d)
        with pytest.raises(ValueError):
            cio.read(io.BytesIO(d.tobytes()))
        path = tmp_path / "d.mh"
        cio.save(path, d)
        with pytest.raises(ValueError):                   # ContainerFile: at open, at the index or at the whole check
            with cio.open(path) as f:
                f.verify_excess()
    # the range query's own check: only the slices it reads
    bad = cases["position outside its segment"]
    ch = int(_ch[s])
    with pytest.raises(ValueError, match="outside its segment"):
        cio.gather_excess(bad, int(lo[s]), int(hi[s]), np.array([ch]), True)
    other = [i for i in range(len(LENS)) if i != ch]
    pos, val, first, last = cio.gather_excess(bad, 0, max(LENS), np.array(other), True)     # not read: not checked
    assert len(pos) == int(sum(np.sum(orig[i][64:].astype(int) > 2) for i in other)) and (last >= first).all()
    with pytest.raises(ValueError, match="monotone"):
        cio.gather_excess(cases["non-monotone exc_seg"], 0, 100, np.array([0]), True)


def test_cut_file_and_wrong_crc_are_refused(trio, tmp_path):
    c, e, _ = trio
    blob = e.tobytes()
    for cut in (1, 8, len(e.exc_val) + 9, len(e.exc_val) + 4 * len(e.exc_pos) + 30):
        with pytest.raises(ValueError, match="truncated"):
            cio.read(io.BytesIO(blob[:-cut]))
    path = tmp_path / "cut.mh"
    path.write_bytes(blob[:-(len(e.exc_val) + 16)])
    with cio.open(path) as f:
        with pytest.raises(ValueError, match="truncated"):
            f.read_excess(len(e.exc_pos) - 4, 4)
        with pytest.raises(ValueError, match="truncated"):
            f.verify_excess()
    crc = _with_crc(e)
    blob = bytearray(crc.tobytes())
    blob[-9] ^= 0x01                                      # one bit of exc_val
    with pytest.raises(ValueError):
        cio.read(io.BytesIO(bytes(blob)))
    # a flip the range checks cannot see (a legal value becomes another legal value) is what excess_crc32 is for
    d = _damaged(crc, exc_val=_set(5, int(crc.exc_val[5]) % 200 + 1))
    excess.check_container(d)
    hdr, body = _split(crc.tobytes())
    good = crc.tobytes()
    forged = good[:len(good) - len(body)] + _split(d.tobytes())[1]
    assert _split(forged)[0]["excess_crc32"] == hdr["excess_crc32"]
    with pytest.raises(ValueError, match="checksum of the excess lists"):
        cio.read(io.BytesIO(forged))
    path = tmp_path / "forged.mh"
    path.write_bytes(forged)
    with pytest.raises(ValueError, match="checksum of the excess lists"):
        cio.load(path)
    with cio.open(path) as f:
        with pytest.raises(ValueError, match="checksum of the excess lists"):
            f.verify_excess()


def _reheader(blob, edit):
    hdr, body = _split(blob)
    edit(hdr)
    h = json.dumps(hdr, sort_keys=True).encode()
    return cio.MAGIC + struct.pack("<I", len(h)) + h + body


def test_header_and_arrays_must_agree(trio, tmp_path):
    c, e, _ = trio
    with pytest.raises(ValueError, match="exact"):        # the writer
        cio.Compressed(dict(c.header, exact=True), c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words, c.payload).tobytes()
    with pytest.raises(ValueError, match="exact"):
        cio.Compressed(c.header, c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words, c.payload, None,
                       e.exc_seg, e.exc_pos, e.exc_val).tobytes()
    blobs = {
        "exact without the arrays": _reheader(c.tobytes(), lambda h: h.update(exact=True)),
        "the arrays without exact": _reheader(e.tobytes(), lambda h: h.pop("exact")),
        "exact: false with the arrays": _reheader(e.tobytes(), lambda h: h.update(exact=False)),
        "one array missing": _reheader(e.tobytes(), lambda h: h["sizes"].pop("exc_val")),
        "checksums without excess_crc32": _reheader(_with_crc(e).tobytes(), lambda h: h.pop("excess_crc32")),
    }
    for what, blob in blobs.items():
        with pytest.raises(ValueError):
            cio.read(io.BytesIO(blob))
        path = tmp_path / "h.mh"
        path.write_bytes(blob)
        with pytest.raises(ValueError):
            cio.open(path)


def test_exact_argument_rule(trio):
    c, e, _ = trio
    assert cio.wants_excess(e, None) and cio.wants_excess(e, True) and not cio.wants_excess(e, False)
    assert not cio.wants_excess(c, None) and not cio.wants_excess(c, False)
    with pytest.raises(ValueError, match="exact=True"):
        cio.wants_excess(c, True)


# ---- one source interface ------------------------------------------------------------------------------------------
PARITY_LENS = [9, 5000, 16 * CH + 1000, 5 * CH + 7]    # no window at all, below a chunk, just over 16 chunks: a head segment, three segments
PARITY_QUERIES = [  # (start, stop, channels, r)
    (100, 100, None, None),                             # an empty range
    (70, 71, [1], None),                                # one sample
    (CH + 5, CH + 900, [2, 3], None),                   # inside one segment
    (100, 300, [2], None),                              # across the end of the head segment
    (2 * CH, 2 * CH + 200, [3, 2], None),               # across a segment boundary of channel 3
    (0, max(PARITY_LENS), None, None),                  # every channel whole
    (3 * CH, 4 * CH + 1, [3, 0, 3, 2, 2], None),        # repeated and unordered
    (4096, 2 * CH + 77, [2, 1], 16),                    # a binned query
]


@pytest.mark.parametrize("rev,crc,exact", [(2, False, False), (2, False, True), (3, False, False), (3, False, True),
                                           (3, True, False), (3, True, True)])
def test_a_compressed_and_its_file_gather_the_same_job(rev, crc, exact, tmp_path):
    """The gather stage sees a `Compressed` and a `ContainerFile` through one interface (payload_words, excess_entries,
    read_words, read_excess): the Job of a query is the same field by field from either, and the file is read for exactly
    that -- four bytes per payload word, five per list entry, exc_seg once.  (Checksums make a container revision 4, which
    is revision 3's layout: there is no revision-2 container with them.)"""
    import dataclasses
    c, chans = _oracle_container(PARITY_LENS, 3, 6, 2, 2, rev, seed=7)
    if exact:
        orig = [np.where(x >= 2, np.minimum(x.astype(np.int64) + (np.arange(len(x)) % 3), 255), x).astype(np.uint8) for x in chans]
        c.header = dict(c.header, exact=True)
        cio.attach_excess(c, *_lists(c, orig))
        assert len(c.exc_pos) > 100
    if crc:
        c = _with_crc(c)
    layout = cio.Directory.of(c)
    assert (layout.head > 0).tolist() == [False, False, rev == 3, False] and layout.nseg.tolist() == [0, 1, 9 + (rev == 3), 3]
    path = tmp_path / "p.mh"
    cio.save(path, c)
    with cio.open(path) as f:
        assert f.payload_words == c.payload_words == c.payload.size and f.bytes_read == f.head_bytes
        assert np.array_equal(f.read_words(3, 40), c.read_words(3, 40)) and np.shares_memory(c.read_words(3, 40), c.payload)
        if exact:
            assert f.excess_entries == c.excess_entries == len(c.exc_pos)
            assert all(np.array_equal(x, y) for x, y in zip(f.read_excess(5, 9), c.read_excess(5, 9)))
            assert np.shares_memory(c.read_excess(5, 9)[0], c.exc_pos) and np.shares_memory(c.read_excess(5, 9)[1], c.exc_val)
        index_read = False
        for start, stop, channels, r in PARITY_QUERIES:
            for check in (True, False):
                mem = cio._range_job(c, start, stop, channels, check, r, use=exact)
                before = f.bytes_read
                got = cio._range_job(f, start, stop, channels, check, r, use=exact)
                want = 0 if mem.payload is None else 4 * mem.payload.size
                if mem.lists is not None:
                    want += 5 * len(mem.lists.pos) + (0 if index_read else 8 * len(c.exc_seg))
                    index_read = True
                assert f.bytes_read - before == want, (start, stop, channels, check)
                assert mem.src is c and got.src is f and (mem.payload is None) == (stop == start)
                for field in dataclasses.fields(cio.Job):
                    a, b = getattr(mem, field.name), getattr(got, field.name)
                    if field.name == "src":
                        continue
                    if field.name == "lists":
                        assert (a is None) == (b is None) == (not exact or mem.payload is None)
                        a, b = a or (), b or ()
                        assert len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))
                    elif isinstance(a, np.ndarray):
                        assert a.dtype == b.dtype and np.array_equal(a, b), field.name
                    else:
                        assert a == b, field.name
        assert index_read == exact
