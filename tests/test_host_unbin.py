"""Counts back to events (mhi_unbin_scratch_bytes, mhi_unbin_count, mhi_unbin_emit; include/muahuff_ingest.h), the part
that needs no GPU: every argument error comes back before a pointer is used, and the scratch size is host arithmetic and
equals what tests/unbin_layout_check.cpp -- csrc/mh_unbin_layout.hpp built alone under AddressSanitizer + UBSan --
prints, over a grid of shapes around every step of the layout; the launch grids follow their rule, and the argument rules
give the same codes and texts in that program as in the library."""
import ctypes as ct
import importlib
import os
import subprocess

import numpy as np
import pytest

from muahuff import _ingest, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "unbin_layout_check.cpp")
FIELDS = ("tile", "group", "tiles_per_row", "tiles", "groups", "off_sum", "off_base", "off_partial", "bytes", "grid", "grid_scan")
CSR, AER = 0, 1


@pytest.fixture(scope="module", autouse=True)
def built():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unbin") / "unbin_layout_check_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, SRC, "-o", out])
    return out


def layouts(exe_path, triples):
    """[(form, rows, cols)] -> [dict of FIELDS, or None where the layout rejects the triple], under the sanitizers"""
    text = "".join("%d %d %d\n" % t for t in triples)
    r = subprocess.run([exe_path], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(triples)
    return [None if ln.startswith("error") else dict(zip(FIELDS, (int(v) for v in ln.split()))) for ln in lines]


def scratch_bytes(form, rows, cols):
    b = ct.c_uint64(0)
    rc = _ingest.lib().mhi_unbin_scratch_bytes(form, rows, cols, ct.byref(b))
    return rc, b.value


def test_prototypes_and_constants():
    for name in ("mhi_unbin_scratch_bytes", "mhi_unbin_count", "mhi_unbin_emit"):
        assert name in _ingest.PROTOTYPES and hasattr(_ingest.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "muahuff_ingest.h")).read()
    assert "#define MHI_UNBIN_CSR 0u" in hdr and "#define MHI_UNBIN_AER 1u" in hdr
    assert (_ingest.UNBIN_CSR, _ingest.UNBIN_AER) == (CSR, AER)
    assert _ingest.lib().mhi_version() == 103
    assert _ingest.unbin_scratch_bytes(CSR, 3, 100) == scratch_bytes(CSR, 3, 100)[1] > 0


# ---- argument errors ---------------------------------------------------------------------------------------------
def _buffers(form, rows, cols):
    rows, cols = max(rows, 1), max(cols, 1)                # (a refused shape still gets stand-ins)
    rc, need = scratch_bytes(form, rows, cols)
    assert rc == _lib.MH_OK
    keep = dict(inp=np.zeros(rows * cols + 64, np.uint8), row_off=np.zeros(rows + 2, np.uint64),
                ev_off=np.zeros(rows + 3, np.uint64), total=np.zeros(2, np.uint64), out_ticks=np.zeros(64, np.uint64),
                out_ch=np.zeros(64, np.uint32), over=np.zeros(2, np.uint64), scratch=np.zeros(need // 8 + 4, np.uint64))
    ptr = {k: ct.c_void_p(v.ctypes.data + (-v.ctypes.data) % 16) for k, v in keep.items()}
    return keep, ptr, need


def _count(form=CSR, rows=3, cols=100, short=0, misalign=0, row_off="fits", **null):
    """mhi_unbin_count with host stand-ins for the device buffers: an argument error must come back before any of them is
    used as a device pointer.  null: name=None for a NULL pointer."""
    keep, ptr, need = _buffers(CSR if form not in (CSR, AER) else form, rows, cols)
    if row_off == "none" or (row_off == "fits" and form == AER):     # "given": a table in any form
        ptr["row_off"] = None
    for k in null:
        ptr[k] = None
    L = _ingest.lib()
    rc = L.mhi_unbin_count(form, ptr["inp"], ptr["row_off"], rows, cols, ptr["ev_off"], ptr["total"],
                           ct.c_void_p(ptr["scratch"].value + misalign) if ptr["scratch"] else None, need - short, None)
    return rc, L.mhi_last_error().decode()


def _emit(form=CSR, rows=3, cols=100, origin=0, period=30, phase=0, ch_bits=32, capacity=8, short=0, misalign=0,
          row_off="fits", overlap=False, **null):
    keep, ptr, need = _buffers(CSR if form not in (CSR, AER) else form, min(rows, 1 << 16), min(cols, 1 << 16))
    if form in (CSR, AER) and rows and cols:
        need = scratch_bytes(form, rows, cols)[1]       # no buffer of that size is made: an error comes back first
    if row_off == "none" or (row_off == "fits" and form == AER):
        ptr["row_off"] = None
    if overlap:
        ptr["out_ticks"] = ct.c_void_p(ptr["inp"].value + rows * cols - 1)      # its first byte is the input's last
    for k in null:
        ptr[k] = None
    L = _ingest.lib()
    rc = L.mhi_unbin_emit(form, ptr["inp"], ptr["row_off"], rows, cols, origin, period, phase, ptr["out_ticks"],
                          ptr["out_ch"], ch_bits, capacity, ptr["over"],
                          ct.c_void_p(ptr["scratch"].value + misalign) if ptr["scratch"] else None, need - short, None)
    return rc, L.mhi_last_error().decode()


COUNT_BAD = [dict(inp=None), dict(row_off="none"), dict(form=AER, row_off="given"), dict(ev_off=None), dict(total=None),
             dict(form=AER, total=None), dict(scratch=None), dict(form=2), dict(form=7), dict(rows=0), dict(cols=0),
             dict(form=AER, rows=0), dict(short=1), dict(form=AER, short=16), dict(misalign=8), dict(form=AER, misalign=4)]

EMIT_BAD = [dict(inp=None), dict(row_off="none"), dict(form=AER, row_off="given"), dict(out_ticks=None), dict(over=None),
            dict(form=AER, out_ch=None), dict(scratch=None), dict(form=2), dict(rows=0), dict(cols=0),
            dict(period=0), dict(period=30, phase=30), dict(period=30, phase=31), dict(period=1, phase=1),
            dict(form=AER, period=0), dict(form=AER, period=7, phase=7),
            dict(origin=(1 << 63) - 99 * 30, period=30, phase=0),               # CSR: the tick of column 99 is 2^63
            dict(origin=(1 << 63) - 99 * 30 - 29, period=30, phase=29),
            dict(origin=1 << 63, period=1), dict(origin=(1 << 64) - 1, period=(1 << 64) - 1, phase=(1 << 64) - 2),
            dict(form=AER, origin=(1 << 63) - 2 * 30, period=30),               # AER: the tick of row 2 is 2^63
            dict(form=AER, ch_bits=0), dict(form=AER, ch_bits=8), dict(form=AER, ch_bits=64), dict(form=AER, ch_bits=24),
            dict(form=AER, rows=2, cols=65537, ch_bits=16),
            dict(short=1), dict(form=AER, short=16), dict(misalign=8), dict(form=AER, misalign=4),
            dict(form=AER, overlap=True)]

_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items())   # noqa: E731


@pytest.mark.parametrize("bad", COUNT_BAD, ids=_ids)
def test_count_argument_errors_come_before_any_device_work(bad):
    rc, msg = _count(**bad)
    assert rc == _lib.ERR_ARG, (rc, msg)
    assert "mhi_unbin_count" in msg, msg


@pytest.mark.parametrize("bad", EMIT_BAD, ids=_ids)
def test_emit_argument_errors_come_before_any_device_work(bad):
    rc, msg = _emit(**bad)
    assert rc == _lib.ERR_ARG, (rc, msg)
    assert "mhi_unbin_emit" in msg, msg


def test_scratch_bytes_argument_errors():
    L = _ingest.lib()
    assert L.mhi_unbin_scratch_bytes(CSR, 3, 100, None) == _lib.ERR_ARG
    for form, rows, cols in ((2, 3, 100), (CSR, 0, 100), (CSR, 3, 0), (AER, 0, 5), (AER, 5, 0), (AER, 5, (1 << 32) + 1),
                             (CSR, 1 << 32, 5), (CSR, 1 << 31, 16385), (AER, 1 << 40, 1 << 20), (CSR, 1 << 63, 1 << 63),
                             (AER, (1 << 64) - 1, 1 << 32)):
        rc, _ = scratch_bytes(form, rows, cols)
        assert rc == _lib.ERR_ARG and "mhi_unbin_scratch_bytes" in L.mhi_last_error().decode(), (form, rows, cols)
    # the largest shapes that are taken: 2^32 - 1 tiles
    assert scratch_bytes(CSR, (1 << 32) - 1, 16384)[0] == _lib.MH_OK
    assert scratch_bytes(AER, (1 << 32) - 1, 16384)[0] == _lib.MH_OK
    L2 = _ingest.lib()                                   # (buffers of that size are not made)
    one = np.zeros(8, np.uint64)
    p = ct.c_void_p(one.ctypes.data + (-one.ctypes.data) % 16)
    assert L2.mhi_unbin_count(CSR, p, p, 1 << 32, 5, p, p, p, 1 << 60, None) == _lib.ERR_ARG
    assert "mhi_unbin_count" in L2.mhi_last_error().decode() and "tiles" in L2.mhi_last_error().decode()


# ---- the layout --------------------------------------------------------------------------------------------------
def _grid():
    tile, group = 16384, 1024
    around = lambda x: [x - 1, x, x + 1]     # noqa: E731
    cols = [1, 15, 16, 17, 1023, 1024, 1025] + around(tile) + around(2 * tile) + [2 * tile + 5, 10 ** 7]
    out = []
    for c in cols:                                               # CSR: a row's tiles step at every multiple of the tile
        for r in (1, 3, 5, 1024):
            out.append((CSR, r, c))
    for tpr, c in ((1, 100), (2, tile + 1), (3, 3 * tile)):      # ... and the groups at every 1024 tiles
        for tiles in around(group) + around(2 * group):
            if tiles % tpr == 0:
                out.append((CSR, tiles // tpr, c))
    for C in (1, 3, 96, 128, 1000, 1024, 65536, 1 << 32):        # AER: the flat block steps at T * C = k * tile
        for k in (1, 2, group, group + 1):
            for d in (-1, 0, 1):
                T = (k * tile + d * C) // C
                if T >= 1:
                    out += [(AER, T, C), (AER, T + 1, C)]
    out += [(CSR, 1024, 10 ** 7), (AER, 10 ** 7, 1024), (CSR, (1 << 32) - 1, 1), (AER, (1 << 32) - 1, 16384)]
    return sorted(set(out))


def test_scratch_bytes_is_the_layout_programs_under_the_sanitizers(exe):
    grid = _grid()
    assert len(grid) > 120
    lays = layouts(exe, grid)
    seen_tiles, seen_groups = set(), set()
    for (form, rows, cols), lay in zip(grid, lays):
        rc, b = scratch_bytes(form, rows, cols)
        assert rc == _lib.MH_OK and lay is not None and b == lay["bytes"] and b > 0, (form, rows, cols, b, lay)
        assert lay["tile"] == 16384 and lay["group"] == 1024
        want = rows * -(-cols // 16384) if form == CSR else -(-rows * cols // 16384)
        assert lay["tiles"] == want and lay["groups"] == -(-want // 1024)
        seen_tiles.add(min(lay["tiles"], 5))
        seen_groups.add(min(lay["groups"], 4))
    assert seen_tiles == {1, 2, 3, 4, 5} and seen_groups == {1, 2, 3, 4}
    bad = layouts(exe, [(2, 5, 5), (CSR, 0, 5), (AER, 5, 0), (CSR, 1 << 32, 5), (AER, 5, (1 << 32) + 1), (1 << 33, 5, 5)])
    assert bad == [None] * 6


def test_the_grids_are_the_rule_restated(exe):
    """count / emit: a workgroup of 4 waves, a wave per tile; the scan's two group kernels: a workgroup per 1024 tiles.
    Neither is capped -- the layout refuses more than 2^32 - 1 tiles"""
    grid = _grid()
    for (form, rows, cols), lay in zip(grid, layouts(exe, grid)):
        tiles = rows * -(-cols // 16384) if form == CSR else -(-rows * cols // 16384)
        assert (lay["grid"], lay["grid_scan"]) == (-(-tiles // 4), -(-tiles // 1024)), (form, rows, cols, lay)
    top = layouts(exe, [(CSR, (1 << 32) - 1, 1)])[0]
    assert top["grid"] == 1 << 30 and top["grid_scan"] == 1 << 22


def test_the_check_program_and_the_library_give_the_same_codes_and_messages(exe):
    """every row of tests/test_host_ingest_messages.py for the three entry points -- 2^32, 2^63 and 2^64 - 1 among the
    values -- through mh_unbin_layout.hpp's checks under the sanitizers"""
    from tests import test_host_ingest_messages as pinned
    refused, accepted = pinned.check_program_agrees(exe, "mhi_unbin_scratch_bytes", "mhi_unbin_count", "mhi_unbin_emit")
    assert refused >= len(COUNT_BAD) + len(EMIT_BAD) + 11 and accepted >= 5


def test_host_arrays_are_refused():
    """there is no CPU path: a NumPy matrix or a host tensor raises before anything is loaded or launched"""
    import torch

    from muahuff import events
    with pytest.raises(ValueError, match="no CPU path"):
        events.EventSet.from_counts(np.zeros((3, 100), np.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        events.EventSet.from_counts(torch.zeros((3, 100), dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        events.aer_from_counts(torch.zeros((100, 3), dtype=torch.uint8))
