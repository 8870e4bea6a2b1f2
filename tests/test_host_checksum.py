"""Payload checksums without a GPU: the CRC-32 arithmetic of k_seg_crc32 (csrc/mh_crc_tables.hpp built alone under
AddressSanitizer + UBSan, tests/crc_check.cpp) against zlib, the argument errors of mhi_seg_crc32 on host stand-ins --
with the text the same program prints from csrc/mh_ingest_check.hpp, for mhi_bin_events too, which shares that header --
container revision 4 and archive revision 2 on oracle-made blocks with zlib's values (container_io.seg_crc_host), and
the point of it all: one flipped payload bit that the structural walks accept and the checksum names."""
import ctypes as ct
import io
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import muahuff
from muahuff import _ingest, _lib, archive
from muahuff import container_io as cio
from tests import helpers
from tests.test_host_archive import _block
from tests.test_host_range_decode import _oracle_container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "crc_check.cpp")
EXE = os.path.join(ROOT, "tests", "crc_check_asan")
CH = muahuff.CHUNK


# ---- the arithmetic ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mh_crc_tables.hpp", "mh_ingest_check.hpp", "mh_launch.hpp", "mh_msg.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                               "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE])
    return EXE


# whole words: 0, below / at / above one piece, around one row (64 pieces of 16 bytes), three rows with a cut head
# piece (3 * 1024 - 1000 + 4 = 2076 bytes: 519 words, 519 % 4 == 3), and the largest segment there is (two chunks at 9
# bits per sample: 36 864 bytes)
LENGTHS = (0, 4, 12, 16, 20, 1020, 1024, 1028, 64 * 16 - 4, 64 * 16 + 4, 2076, 36864)


def test_reference_and_wave_form_agree_with_zlib(exe):
    rng = np.random.RandomState(5)
    msgs = [rng.randint(0, 256, n).astype(np.uint8).tobytes() for n in LENGTHS]
    msgs += [b"\xff" * 1028, b"\0" * 2076, b"123456789"]
    assert 2076 % 16 and -(-2076 // 1024) == 3
    r = subprocess.run([exe], input="".join(m.hex() + "\n" for m in msgs), capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(msgs)
    for m, ln in zip(msgs, lines):
        ref, wave = ln.split()
        want = 0 if len(m) == 0 else zlib.crc32(m)      # zlib.crc32(b"") == 0 as well: a segment of 0 words has CRC 0
        assert want == zlib.crc32(m)
        assert int(ref, 16) == want, (len(m), ln)
        if len(m) % 4 == 0:
            assert int(wave, 16) == want, (len(m), ln)
        else:
            assert wave == "-"
    assert lines[-1].split()[0] == "cbf43926"


# ---- the ABI ------------------------------------------------------------------------------------------
def _call(**null):
    """mhi_seg_crc32 on host stand-ins with the named arguments NULL -> (rc, message); never reaches a launch"""
    pay, off, words = np.zeros(8, np.uint32), np.zeros(2, np.uint64), np.full(2, 4, np.uint64)
    crc, expect, bad = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    a = dict(payload=pay.ctypes.data, seg_off=off.ctypes.data, seg_words=words.ctypes.data, crc=crc.ctypes.data,
             expect=expect.ctypes.data, bad=bad.ctypes.data)
    a.update({k: None for k in null})
    L = _ingest.lib()
    rc = L.mhi_seg_crc32(a["payload"], 8, a["seg_off"], a["seg_words"], 2, None, 0, a["crc"], a["expect"], a["bad"], None)
    return rc, L.mhi_last_error().decode()


@pytest.mark.parametrize("null", [("payload",), ("seg_off",), ("seg_words",), ("crc", "expect"), ("crc", "expect", "bad"),
                                  ("bad",), ("crc", "bad")], ids="+".join)
def test_argument_errors_come_before_any_device_work(null):
    rc, msg = _call(**dict.fromkeys(null))
    assert rc == _lib.ERR_ARG, (rc, msg)
    assert "mhi_seg_crc32" in msg, msg


def test_misaligned_payload_is_refused():
    pay = np.zeros(16, np.uint8)
    z = np.zeros(2, np.uint64)
    L = _ingest.lib()
    assert L.mhi_seg_crc32(pay.ctypes.data + 1, 2, z.ctypes.data, z.ctypes.data, 1, None, 0, z.ctypes.data, None, None,
                           None) == _lib.ERR_ARG
    assert "aligned" in L.mhi_last_error().decode()
    assert L.mhi_version() == 103


def test_the_check_program_and_the_library_give_the_same_codes_and_messages(exe):
    """every row of tests/test_host_ingest_messages.py for mhi_seg_crc32 and mhi_bin_events through
    csrc/mh_ingest_check.hpp under the sanitizers; the binner's out_off entries sit in a heap block of exactly C entries"""
    from tests import test_host_ingest_messages as pinned
    refused, accepted = pinned.check_program_agrees(exe, "mhi_seg_crc32")
    assert refused >= 8 and accepted >= 2
    refused, accepted = pinned.check_program_agrees(exe, "mhi_bin_events")
    assert refused >= 21 + 5 and accepted == 0


# ---- container revision 4 -----------------------------------------------------------------------------
def _with_crc(c):
    return cio.Compressed(dict(c.header, format_revision=4), c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words,
                          c.payload, cio.seg_crc_host(c))


@pytest.fixture(scope="module")
def pair():
    """(plain container, the same with checksums): five channels, S = 3, two chunks per segment"""
    c, _ = _oracle_container([20000, 50000, 3000, 17 * CH + 5, 9], 3, 6, 2, 2)
    return c, _with_crc(c)


def test_seg_crc_host_is_zlib_per_segment(pair):
    c, k = pair
    off = np.concatenate([[0], np.cumsum(c.seg_words)]).astype(int)
    assert k.seg_crc.dtype == np.uint32 and len(k.seg_crc) == len(c.seg_words) > 5
    for s in range(len(c.seg_words)):
        assert int(k.seg_crc[s]) == zlib.crc32(c.payload[off[s]:off[s + 1]].astype("<u4").tobytes())
    empty = cio.Compressed(c.header, c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, np.array([0, 3, 0], np.uint64),
                           c.payload[:3])
    assert cio.seg_crc_host(empty).tolist() == [0, zlib.crc32(c.payload[:3].tobytes()), 0]


def test_plain_container_bytes_are_what_they_were(pair):
    c, _ = pair
    assert c.seg_crc is None and c.header["format_revision"] == cio.FORMAT_REVISION == 3
    assert cio.READ_REVISIONS == (2, 3, 4)
    hdr = dict(c.header, sizes={name: int(getattr(c, name).size) for name, _ in cio.ARRAYS})
    blob = json.dumps(hdr, sort_keys=True).encode()
    want = cio.MAGIC + struct.pack("<I", len(blob)) + blob
    for name, dt in cio.ARRAYS:
        raw = np.ascontiguousarray(getattr(c, name), dt).tobytes()
        want += raw + b"\0" * (-len(raw) % 8)
    assert c.tobytes() == want and cio.nbytes(c) == len(want)
    assert b"checksum" not in want and b"seg_crc" not in want


def test_round_trip_with_checksums(pair, tmp_path):
    c, k = pair
    raw = k.tobytes()
    assert len(raw) == cio.nbytes(k) == cio.nbytes(c) + 4 * len(k.seg_crc) + (-4 * len(k.seg_crc) % 8) + len(
        cio._header_blob(k)) - len(cio._header_blob(c))
    back = cio.read(io.BytesIO(raw))
    assert back.header["format_revision"] == 4 and back.header["checksum"] == "crc32"
    assert back.header["sizes"]["seg_crc"] == len(k.seg_crc) and isinstance(back.header["arrays_crc32"], int)
    for name, _ in cio.ARRAYS + (("seg_crc", None),):
        a, b = getattr(back, name), getattr(k, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    pay_bytes = 4 * k.payload.size + (-4 * k.payload.size % 8)
    # arrays_crc32 is zlib over the bytes between the header and the payload, padding included
    head = 12 + int.from_bytes(raw[8:12], "little")
    assert back.header["arrays_crc32"] == zlib.crc32(raw[head:len(raw) - pay_bytes])
    for offset in (0, 24):
        fn = str(tmp_path / ("k%d.muahuff" % offset))
        with open(fn, "wb") as f:
            f.write(b"\xee" * offset + raw)
        with cio.ContainerFile(fn, offset) as cf:
            assert cf.header == back.header and cf.payload_offset == offset + len(raw) - pay_bytes
            assert np.array_equal(cf.seg_crc, k.seg_crc) and cf.seg_crc.dtype == np.uint32
            assert np.array_equal(cf.read_words(0, cf.payload_words), k.payload)
            assert np.array_equal(cio.seg_crc_host(cf), k.seg_crc)
    fn = str(tmp_path / "plain.muahuff")
    cio.save(fn, c)
    with cio.ContainerFile(fn) as cf:
        assert cf.seg_crc is None
    assert cio.load(fn).seg_crc is None
    cio.validate(back)      # revision 4 walks as revision 3


def test_revision_and_sizes_must_agree(pair):
    c, k = pair
    with pytest.raises(ValueError):     # revision 3 with seg_crc
        cio.Compressed(c.header, *[getattr(k, n) for n, _ in cio.ARRAYS], k.seg_crc).tobytes()
    with pytest.raises(ValueError):     # revision 4 without
        cio.Compressed(k.header, *[getattr(k, n) for n, _ in cio.ARRAYS]).tobytes()

    def reheadered(raw, edit):
        n = int.from_bytes(raw[8:12], "little")
        hdr = json.loads(raw[12:12 + n].decode())
        edit(hdr)
        blob = json.dumps(hdr, sort_keys=True).encode()
        return cio.MAGIC + struct.pack("<I", len(blob)) + blob + raw[12 + n:]

    for raw, edit in ((k.tobytes(), lambda h: h["sizes"].pop("seg_crc")),
                      (k.tobytes(), lambda h: h.update(format_revision=3)),
                      (c.tobytes(), lambda h: h.update(format_revision=4)),
                      (c.tobytes(), lambda h: h["sizes"].update(seg_crc=0))):
        with pytest.raises(ValueError, match="seg_crc"):
            cio.read(io.BytesIO(reheadered(raw, edit)))
    with pytest.raises(ValueError, match="unsupported container revision"):
        cio.read(io.BytesIO(reheadered(c.tobytes(), lambda h: h.update(format_revision=5))))


def test_a_flipped_byte_in_front_of_the_payload_fails_arrays_crc32(pair, tmp_path):
    _c, k = pair
    raw = bytearray(k.tobytes())
    head = 12 + int.from_bytes(raw[8:12], "little")
    C = len(k.ch_len)
    peak_at = head + 8 * C                      # ch_len u64[C], then peak u8[C]
    assert raw[peak_at:peak_at + C] == k.peak.tobytes()
    seg_words_at = peak_at + 3 * (C + (-C % 8)) + 8 * C
    assert raw[seg_words_at:seg_words_at + 8] == k.seg_words[:1].tobytes()
    for at in (peak_at + 1, peak_at + C + (-C % 8) + 2, seg_words_at + 8, peak_at + C):     # peak, enc, seg_words, padding
        bad = bytearray(raw)
        bad[at] ^= 1
        with pytest.raises(ValueError, match="checksum of the arrays"):
            cio.read(io.BytesIO(bytes(bad)))
        fn = str(tmp_path / "bad.muahuff")
        with open(fn, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError, match="checksum of the arrays"):
            cio.ContainerFile(fn)
    cio.read(io.BytesIO(bytes(raw)))


# ---- archive revision 2 -------------------------------------------------------------------------------
AC, AS, ASC = 4, 3, 2
ALENS = (CH + 1, 5 * CH + 7, 40)


@pytest.fixture(scope="module")
def ablocks():
    return [_block(Tb, n_ch=AC, S_=AS, sc=ASC, seed=k) for k, Tb in enumerate(ALENS)]


def _create(fn, blocks, **kw):
    with archive.create(fn, AC, S=AS, sclv_rows=helpers.sclv_tables()[AS], seg_chunks=ASC, **kw) as w:
        for c in blocks:
            w.append_compressed(c)


def test_checksum_false_is_the_default_byte_for_byte(ablocks, tmp_path):
    a, b = str(tmp_path / "a.mua"), str(tmp_path / "b.mua")
    _create(a, ablocks)
    _create(b, ablocks, checksum=False)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read() and b"checksum" not in raw
    with archive.open(a) as r:
        assert r.header["archive_revision"] == 1 and not r.checksum
        with pytest.raises(ValueError, match="no checksums"):
            r.verify(device=False)
    with archive.open(a, "a") as w:
        with pytest.raises(ValueError):         # a block with checksums does not go into a plain archive
            w.append_compressed(_with_crc(ablocks[0]))


def test_checksummed_archive_holds_revision_4_blocks_and_goes_on_with_them(ablocks, tmp_path):
    fn = str(tmp_path / "k.mua")
    _create(fn, ablocks[:2], checksum=True)
    with archive.open(fn, "a") as w:            # continues in the file's own mode; takes a block's own values as well
        assert w.checksum
        w.append_compressed(_with_crc(ablocks[2]))
    with archive.open(fn) as r:
        assert r.header["archive_revision"] == 2 and r.header["checksum"] == "crc32" and r.checksum
        assert len(r.blocks) == 3 and r.T == sum(ALENS)
        for i, c in enumerate(ablocks):
            b = r.block(i)
            assert b.header["format_revision"] == 4 and np.array_equal(b.payload, c.payload)
            assert np.array_equal(b.seg_crc, cio.seg_crc_host(c))
            assert np.array_equal(r.block_file(i).seg_crc, b.seg_crc)
        assert r.verify(device=False) == []


def _flip_behind_a_chunk_header(fn, rd, block, seg):
    """flip one payload bit of segment `seg` of block `block` in the file, three words behind its first chunk header"""
    bf = rd.block_file(block)
    off = int(np.sum(bf.seg_words[:seg]))
    w0 = int(bf.read_words(off, 1)[0])
    hdr_words = (16 + 64 * ((w0 >> 12) & 15) + 31) >> 5
    word = off + hdr_words + 3
    assert hdr_words + 3 < int(bf.seg_words[seg])
    at = bf.payload_offset + 4 * word + 1
    with open(fn, "r+b") as f:
        f.seek(at)
        b = f.read(1)[0]
        f.seek(at)
        f.write(bytes([b ^ 0x10]))


def test_one_flipped_payload_bit_passes_the_structural_walks_and_fails_the_checksum(ablocks, tmp_path):
    clean = str(tmp_path / "clean.mua")
    _create(clean, ablocks, checksum=True)
    fn = str(tmp_path / "flipped.mua")
    shutil.copy(clean, fn)
    block, seg = 1, 4       # channel 1's second segment of the 5-chunk block (three segments per channel: 2 chunks, 2 chunks, the rest)
    with archive.open(clean) as r:
        assert len(r.block_file(block).seg_words) == 3 * AC
        _flip_behind_a_chunk_header(fn, r, block, seg)
    assert open(fn, "rb").read() != open(clean, "rb").read()
    with archive.open(fn) as r:
        assert r.verify(device=False) == [(block, seg)]
        c = r.block(block)
        cio.validate(c)                                                         # mh_validate_stream: accepts
        job = cio._range_job(c, 0, ALENS[block], None, True)                    # mh_validate_segments: too
        assert job.payload.size == c.payload.size and seg in job.segs.tolist()
        bf = r.block_file(block)
        cio._range_job(bf, 2 * CH, 4 * CH, [1], True)
