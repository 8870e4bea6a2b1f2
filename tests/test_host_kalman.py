"""The Kalman filter decoder without a GPU (include/muahuff_kalman.h, libmuahuff_kalman.so, muahuff.kalman): the ABI's three
descriptions agree and the six older libraries are as they were, every argument error comes back before a pointer is used
-- with the text tests/kalman_check.cpp prints, which is csrc/mh_kalman_layout.hpp built alone under AddressSanitizer +
UBSan --, the tiles, the loads, the scratch and the capped grids hold over a sweep of shapes, the fit from statistics is
the reference's fit, KalmanStats add without the junction pair, the gain table converges, and the information form
agrees with the reference's explicit recursion."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _cascade, _ingest, _kalman, _lib, _smooth, _sweep, _wiener, kalman, wiener
from tests import kalman_oracle as ko
from tests.test_host_wiener import D_REF_W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "kalman_check.cpp")
# mh_kalman_layout.hpp: kProjTileCols, kProjMaxBlocks, kScanTile, kScanThreads, kScanMaxBlocks
PROJ_TILE, PROJ_MAX_BLOCKS, TILE, SCAN_THREADS, SCAN_MAX_BLOCKS = 1024, 4096, 512, 64, 512

# The host-route figure: the largest difference between ko.information_predict (the gain table K_t = B_t M and the serial
# recurrence, what the device runs) and ko.reference_predict (the reference's loop with inv(H P H^T + Q) in every step) on
# the data of test_the_information_form_agrees_with_the_explicit_recursion, in units of the state's standard deviation, as
# measured per shape: 7 x 4000 clip 4: 1.4e-15; 33 x 3000 lead 2: 6.0e-15; 96 x 6000 clip 3: 3.1e-15 (the larger of alpha 0
# and 1e-2).  Recorded at twice the largest, since a LAPACK may pivot or sum in another order elsewhere.
# tests/test_gpu_kalman.py allows the device 64 times this.
D_KALMAN = 1.2e-14
# The largest difference between ko.tiled_scan (three phases over tiles of 512 steps) and ko.serial_scan on SCAN_CASES,
# relative to the largest state of the case, as measured by test_the_tiled_scan_agrees_with_the_serial_one: 4.54e-16 in
# case 5, 2.5e-16 and less in the others (the cases of spectral radius 0.5 agree bit for bit: a tile forgets its start).  tests/test_gpu_kalman.py allows mhk_scan 64
# times this.
D_SCAN = 4.6e-16

# (k, cols, ranges, n_gain, spectral radius, in place, pitched): shorter than a tile, exactly one tile (513 columns), two and
# many tiles, 0 and 1 columns; 1, 3 and 16 ranges; n_gain 1, 5, tile + 3, 4096 and larger than the range; k 1, 2, 3, 8
SCAN_CASES = [
    (2, 3000, [(0, 3000)], 5, 0.98, False, False),
    (3, 2500, [(3, 200), (200, 200 + TILE + 1), (800, 800 + 2 * TILE + 8)], TILE + 3, 0.98, False, True),
    (8, 1500, [(0, 0), (0, 1), (1, 40), (40, 40), (41, 42), (50, 50 + TILE + 2), (600, 601), (601, 700), (700, 700), (700, 702),
               (710, 720), (720, 730), (730, 731), (740, 1300), (1300, 1301), (1400, 1500)], 1, 0.5, True, False),
    (1, 6000, [(5, 5900)], 4096, 0.98, True, True),
    (2, 700, [(0, 300), (300, 700)], 600, 0.5, False, False),
    (8, 1200, [(0, 100), (100, 1150), (1150, 1200)], 5, 0.98, False, True),
]


def scan_inputs(i):
    k, cols, ranges, n_gain, radius, _inplace, _pitched = SCAN_CASES[i]
    F, B = ko.contractive(k, n_gain, radius, 40 + i)
    rng = np.random.RandomState(60 + i)
    return rng.randn(k, cols), F, B, rng.randn(len(ranges), k)


_serial = {}


def scan_reference(i):
    """ko.serial_scan of case i, computed once and shared with tests/test_gpu_kalman.py (never written to)"""
    if i not in _serial:
        v, F, B, init = scan_inputs(i)
        _serial[i] = ko.serial_scan(v, SCAN_CASES[i][2], F, B, init)
        _serial[i].setflags(write=False)
    return _serial[i]


@pytest.fixture(scope="module", autouse=True)
def built():
    b = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    b.build_kalman()
    b.build(), b.build_ingest(), b.build_wiener(), b.build_cascade(), b.build_smooth(), b.build_sweep()   # (no-ops when fresh)


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_kalman.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhk_\w+)\s*\(", code))
    assert declared == set(_kalman.PROTOTYPES) == {"mhk_version", "mhk_last_error", "mhk_project", "mhk_scan_scratch_bytes", "mhk_scan"}
    nm = subprocess.run(["nm", "-D", "--defined-only", _kalman.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared                                  # nothing else is exported
    for fn in ("mhk_project", "mhk_scan_scratch_bytes", "mhk_scan"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % fn, code).group(1)
        assert len(args.split(",")) == len(_kalman.PROTOTYPES[fn][1])
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_kalman.hpp", "csrc/mh_kalman_layout.hpp", "csrc/exports_kalman.map"} <= set(build.KALMAN_HEADERS)
    assert build.KALMAN_SOURCES == ["csrc/mh_kalman.hip"] and build.KALMAN_SO == _kalman.SO
    with open(os.path.join(ROOT, "include", "muahuff.h")) as f:
        version = int(re.search(r"#define\s+MH_VERSION\s+(\d+)", f.read()).group(1))
    assert _kalman.lib().mhk_version() == version == 103 == _wiener.lib().mhw_version()
    assert muahuff.kalman is kalman and muahuff._kalman is _kalman
    # the new entry points went into none of the older libraries
    older = [n for m in (_ingest, _lib, _wiener, _cascade, _smooth, _sweep) for n in m.PROTOTYPES]
    assert not any(n.startswith("mhk_") for n in older)
    for so in (build.SO, build.INGEST_SO, build.WIENER_SO, build.CASCADE_SO, build.SMOOTH_SO, build.SWEEP_SO):
        assert "mhk_" not in subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert (_kalman.PROJ_TILE_COLS, _kalman.PROJ_MAX_BLOCKS, _kalman.SCAN_TILE, _kalman.SCAN_THREADS, _kalman.SCAN_MAX_BLOCKS) == (
        PROJ_TILE, PROJ_MAX_BLOCKS, TILE, SCAN_THREADS, SCAN_MAX_BLOCKS)
    assert (_kalman.MAX_K, _kalman.MAX_ROWS, _kalman.MAX_GAINS, _kalman.MAX_RANGES) == (8, 65536, 4096, 16)


# ---- argument errors ---------------------------------------------------------------------------------------------------
PROJECT = ("x", "x_row_stride", "rows", "cols", "clip", "m", "m0", "k", "v", "v_row_stride")
SCAN = ("v", "v_row_stride", "k", "cols", "ranges", "n_ranges", "f", "b", "n_gain", "init", "out", "out_row_stride", "scratch", "scratch_bytes")
POINTERS = ("x", "m", "m0", "v", "f", "b", "init", "out", "scratch")
T40, T48 = 1 << 40, 1 << 48


def _args(order, **over):
    """the arguments of mhk_project / mhk_scan with host stand-ins for the device buffers (kept alive in the first item);
    a pointer given as the name of another one starts where that one does (before any shift); ranges: a list of pairs, or
    None for a NULL pointer"""
    keep = {k: np.zeros(1 << 14, np.uint64) for k in POINTERS if k in order}
    a = dict(x_row_stride=128, rows=3, cols=100, clip=39, k=2, v_row_stride=800, out_row_stride=800, n_gain=7, scratch_bytes=1 << 16,
             ranges=[(0, 40), (40, 100)])
    a = {k: v for k, v in a.items() if k in order}
    for k, v in keep.items():
        a[k] = v.ctypes.data + (-v.ctypes.data) % 16
    alias = {k: over.pop(k) for k in list(over) if isinstance(over[k], str)}
    shift = {k[:-6]: over.pop(k) for k in list(over) if k.endswith("_shift")}
    for k, v in over.items():
        a[k] = (0 if v is None and k != "ranges" else v)
    for k, other in alias.items():
        a[k] = a[other]
    for k, s in shift.items():
        a[k] += s
    if "ranges" in a:
        a.setdefault("n_ranges", len(a["ranges"] or []))
    return keep, a


def _call(order, a):
    L = _kalman.lib()
    if order is PROJECT:
        vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in order]
        rc = L.mhk_project(*vals, None)
    else:
        flat = [u for ab in (a["ranges"] or []) for u in ab]
        host = (ct.c_uint64 * max(len(flat), 1))(*flat)
        vals = [(ct.cast(host, ct.c_void_p) if a["ranges"] is not None else None) if k == "ranges"
                else ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in order]
        rc = L.mhk_scan(*vals, None)
    return rc, L.mhk_last_error().decode()


def _line(order, a):
    if order is PROJECT:
        return "project " + " ".join(str(a[k]) for k in order) + "\n"
    flat = [u for ab in (a["ranges"] or []) for u in ab]
    head = [str(int(a["ranges"] is not None)) if k == "ranges" else str(a[k]) for k in order]
    return "scan " + " ".join(head + [str(u) for u in flat]) + "\n"


PROJECT_BAD = [dict(x=None), dict(m=None), dict(v=None), dict(k=0), dict(k=9), dict(rows=0), dict(rows=65537), dict(cols=0),
               dict(cols=T40, x_row_stride=T40, v_row_stride=8 * T40), dict(clip=0), dict(clip=256), dict(m_shift=4), dict(m0_shift=4),
               dict(v_shift=4), dict(v_row_stride=804), dict(x_row_stride=99), dict(x_row_stride=0), dict(x_row_stride=T48),
               dict(v_row_stride=792), dict(v_row_stride=0), dict(v_row_stride=T48), dict(v="x"), dict(v="m"), dict(v="m0"),
               dict(v="x", v_shift=296), dict(m="v", m_shift=1592), dict(m0="v", m0_shift=8)]
PROJECT_GOOD = [dict(), dict(m0=None), dict(x_shift=1), dict(x_shift=3, x_row_stride=100), dict(rows=1, x_row_stride=0), dict(k=1, v_row_stride=0),
                dict(k=8, v=1 << 60), dict(clip=1), dict(clip=255), dict(rows=65536, m=1 << 50, x=1 << 55), dict(v_shift=8),
                dict(cols=T40 - 1, x_row_stride=T40, v_row_stride=8 * T40, v=1 << 60), dict(v="x", v_shift=360),
                dict(x_row_stride=T48 - 1, v_row_stride=T48 - 8, v=1 << 60), dict(m="v", m_shift=1600)]
SCAN_BAD = [dict(v=None), dict(f=None), dict(b=None), dict(init=None), dict(out=None), dict(scratch=None), dict(ranges=None, n_ranges=2),
            dict(k=0), dict(k=9), dict(cols=0), dict(cols=T40, v_row_stride=8 * T40, out_row_stride=8 * T40), dict(ranges=[], n_ranges=0),
            dict(ranges=[(i, i + 1) for i in range(17)]), dict(n_gain=0), dict(n_gain=4097), dict(v_shift=4), dict(out_shift=4),
            dict(v_row_stride=804), dict(out_row_stride=804), dict(f_shift=4), dict(b_shift=4), dict(init_shift=4), dict(scratch_shift=4),
            dict(v_row_stride=792), dict(out_row_stride=792), dict(out_row_stride=0), dict(v_row_stride=T48), dict(ranges=[(5, 4)]),
            dict(ranges=[(0, 50), (49, 60)]), dict(ranges=[(0, 101)]), dict(ranges=[(50, 60), (0, 10)]), dict(out="v", out_shift=8),
            dict(out="v", out_row_stride=808), dict(out="v", out_shift=1592), dict(cols=2000, v_row_stride=16000, out_row_stride=16000,
                                                                                  ranges=[(0, 2000)], scratch_bytes=4 * 8 * 8 - 1),
            dict(scratch="out"), dict(scratch="v", scratch_shift=1592), dict(f="out"), dict(b="out", b_shift=1592), dict(init="out", init_shift=800)]
SCAN_GOOD = [dict(), dict(out="v"), dict(k=1, v_row_stride=0, out_row_stride=0), dict(k=8, v=1 << 60, out=1 << 61), dict(n_gain=1), dict(n_gain=4096, f=1 << 50, b=1 << 51),
             dict(ranges=[(0, 0)]), dict(ranges=[(100, 100)]), dict(ranges=[(0, 100)]), dict(ranges=[(i, i + 1) for i in range(16)]),
             dict(ranges=[(0, 1), (1, 1), (1, 5)]), dict(out="v", out_shift=1600), dict(v_row_stride=808, out_row_stride=816),
             dict(cols=2000, v_row_stride=16000, out_row_stride=16000, ranges=[(0, 2000)], scratch_bytes=4 * 8 * 8),
             dict(scratch_bytes=0, ranges=[(0, 1), (5, 6)]), dict(scratch="out", scratch_shift=1600),
             dict(cols=T40 - 1, v_row_stride=8 * T40, out_row_stride=8 * T40, v=1 << 60, out=1 << 61, ranges=[(0, 10)])]
SCRATCH_BAD = [(0, 2, 1), (T40, 2, 1), (100, 0, 1), (100, 9, 1), (100, 2, 0), (100, 2, 17)]
_ids = lambda d: ",".join("%s=%s" % (k, v if not isinstance(v, list) or len(v) < 4 else "%d ranges" % len(v)) for k, v in d.items()) or "default"   # noqa: E731


@pytest.mark.parametrize("bad", PROJECT_BAD, ids=_ids)
def test_project_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(PROJECT, **dict(bad))
    rc, msg = _call(PROJECT, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhk_project:"), (rc, msg)


@pytest.mark.parametrize("bad", SCAN_BAD, ids=_ids)
def test_scan_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(SCAN, **dict(bad))
    rc, msg = _call(SCAN, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhk_scan:"), (rc, msg)


def test_scan_scratch_bytes_is_host_arithmetic():
    assert _kalman.scan_scratch_bytes(10 ** 7, 2, 5) == (10 ** 7 // TILE + 5) * 8 * 8
    assert _kalman.scan_scratch_bytes(1, 8, 16) == 16 * 80 * 8
    for cols, k, n in SCRATCH_BAD:
        with pytest.raises(muahuff.MuaHuffError, match="mhk_scan_scratch_bytes:"):
            _kalman.scan_scratch_bytes(cols, k, n)
    assert _kalman.lib().mhk_scan_scratch_bytes(100, 2, 1, None) == _lib.ERR_ARG


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kalman") / "kalman_check_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def _run(exe_path, text):
    r = subprocess.run([exe_path], input=text, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_the_check_program_and_the_library_give_the_same_codes_and_messages(exe):
    for order, bad, good, rules in ((PROJECT, PROJECT_BAD, PROJECT_GOOD, 9), (SCAN, SCAN_BAD, SCAN_GOOD, 12)):
        cases = [_args(order, **dict(b)) for b in bad]
        lines = _run(exe, "".join(_line(order, a) for _k, a in cases))
        assert len(lines) == len(bad)
        seen = set()
        for (keep, a), ln, b in zip(cases, lines, bad):
            rc, msg = _call(order, a)
            assert ln == "error %d %s" % (rc, msg) and rc == _lib.ERR_ARG, (b, ln, msg)
            seen.add(re.sub(r"\d+", "#", msg))
        assert len(seen) >= rules, seen                            # the table reaches every rule, not one message over and over
        ok = [_args(order, **dict(g)) for g in good]
        # (accepted arguments would be launched: they are checked through the program alone)
        assert _run(exe, "".join(_line(order, a) for _k, a in ok)) == ["ok"] * len(good), order
    text = "".join("scratch %d %d %d 64\n" % s for s in SCRATCH_BAD) + "scratch 100 2 1 0\nscratch 100 2 1 64\n"
    lines = _run(exe, text)
    head = "error %d mhk_scan_scratch_bytes:" % _lib.ERR_ARG
    assert len(lines) == len(SCRATCH_BAD) + 2 and all(ln.startswith(head) for ln in lines[:-1]) and lines[-1] == "ok"


def layout(cols, k, ranges):
    """mh_kalman_layout.hpp's rules, restated -> [proj tiles, proj grid, scan tiles, scan grid, scratch bytes]"""
    pt = -(-cols // PROJ_TILE)
    st = sum(-(-max(b - a - 1, 0) // TILE) for a, b in ranges)
    return [pt, min(pt, PROJ_MAX_BLOCKS), st, min(-(-st // SCAN_THREADS), SCAN_MAX_BLOCKS), st * k * (k + 2) * 8]


# the shapes tests/test_gpu_kalman.py runs past the grid caps
PROJECT_PAST_CAP = PROJ_MAX_BLOCKS * PROJ_TILE + 1
SCAN_PAST_CAP_RANGE = (SCAN_MAX_BLOCKS * SCAN_THREADS // 16 + 3) * TILE + 7      # columns of each of 16 ranges
SCAN_PAST_CAP = [(r * SCAN_PAST_CAP_RANGE, (r + 1) * SCAN_PAST_CAP_RANGE - (r % 3)) for r in range(16)]


def test_tiles_loads_scratch_and_grids_over_the_sweep(exe):
    """kalman_check asserts per shape what its header comment lists"""
    grid = []
    for cols in (1, 2, 3, 4, 5, 63, TILE, TILE + 1, TILE + 2, PROJ_TILE - 1, PROJ_TILE, PROJ_TILE + 1, 3 * PROJ_TILE + 5, 72000, 10 ** 7):
        for k in (1, 2, 3, 8):
            fifth = cols // 5
            for ranges in ([(0, cols)], [(0, 0)], [(cols, cols)], [(cols - 1, cols)], [(i * fifth, (i + 1) * fifth) for i in range(5)],
                           [(min(2 * i, cols), min(2 * i + (i % 3), cols)) for i in range(16)],
                           [(cols * i // 16, cols * (i + 1) // 16 - (1 if cols >= 32 and i % 2 else 0)) for i in range(16)]):
                grid.append((cols, k, ranges))
    grid += [(c, k, r) for k, c, r, _n, _rad, _i, _p in SCAN_CASES]
    grid += [(T40 - 1, 8, [(0, T40 - 1)]), (T40 - 1, 1, [(i * (T40 // 16), (i + 1) * (T40 // 16) - 1) for i in range(16)]),
             (T40 - 1, 2, [(5, 6), (T40 - 600, T40 - 1)])]
    grid += [(PROJECT_PAST_CAP, 1, [(0, PROJECT_PAST_CAP)]), (SCAN_PAST_CAP[-1][1], 1, SCAN_PAST_CAP)]
    text = "".join("layout %d %d %d %s\n" % (c, k, len(r), " ".join("%d %d" % ab for ab in r)) for c, k, r in grid)
    lines = _run(exe, text)
    assert len(lines) == len(grid)
    strided_proj = strided_scan = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == layout(*g), (g, got)
        assert got[4] <= _kalman.scan_scratch_bytes(g[0], g[1], len(g[2]))
        strided_proj += got[0] > got[1]
        strided_scan += got[2] > got[3] * SCAN_THREADS
    assert strided_proj > 20 and strided_scan >= 3                 # (only 2^40 columns and the shape built for it pass the scan cap)
    assert layout(PROJECT_PAST_CAP, 1, [])[:2] == [PROJ_MAX_BLOCKS + 1, PROJ_MAX_BLOCKS]
    assert layout(1, 1, SCAN_PAST_CAP)[2] > SCAN_MAX_BLOCKS * SCAN_THREADS
    assert all(layout(1, 1, [ab])[2] <= SCAN_MAX_BLOCKS * SCAN_THREADS for ab in SCAN_PAST_CAP)   # each alone stays under the cap
    assert layout(10 ** 7, 2, [(0, 10 ** 7)]) == [9766, 4096, 19532, 306, 19532 * 64]


# ---- the fit -------------------------------------------------------------------------------------------------------------
FIT_SHAPES = [(7, 2, 4000, 0, 4), (33, 2, 3000, 2, None), (96, 2, 6000, 0, 3)]      # C, K, T, lead, clip


def host_stats(r, lead, clip, C):
    t = torch.from_numpy
    w = wiener.Stats(r["n"], t(r["sum_x"]), t(r["gram"]), t(r["xty"]), t(r["sum_y"]), t(r["sum_yy"]), 1, lead, 255 if clip is None else clip, C)
    return kalman.KalmanStats(w, r["n_pairs"], t(r["sum_a"]), t(r["sum_b"]), t(r["aa"]), t(r["bb"]), t(r["ab"]), t(r["sum_d"]), t(r["dd"]), t(r["ad"]))


@pytest.mark.parametrize("shape", FIT_SHAPES[:2], ids=str)
def test_the_fit_from_statistics_is_the_reference_fit(shape):
    """A, W, H, Q from KalmanStats against Ridge and np.cov on the explicit z-scored data, within the 64 x D_REF_W of the
    largest entry that the Wiener fit from statistics is allowed against its explicit routes (the statistics are the same)"""
    C, K, T, lead, clip = shape
    x, y = ko.data(C, K, T, 1)
    p = ko.prepare(x, y, lead, clip)
    silent = min(3, C - 1)
    assert silent not in p["keep"] and len(p["keep"]) == C - 1
    for alpha in (0.0, 1e-2):
        model = ko.reference_fit(p["Z"], p["Y"], alpha)
        f = kalman.KalmanFilter(alpha).fit(host_stats(ko.stats(x, y, lead, clip), lead, clip, C))
        for name, ref in zip("AWHQ", model):
            got = getattr(f, name).numpy()
            d = np.abs(got - ref).max() / np.abs(ref).max()
            print("%s alpha %g: %s differs by %.2e of its largest entry" % (shape, alpha, name, d))
            assert got.shape == ref.shape and d <= 64 * D_REF_W
        M = np.linalg.solve(model[3], model[2]).T
        assert np.allclose(f.gain.numpy(), M, rtol=0, atol=1e-9 * np.abs(M).max())       # (the right product, not a precision claim)
        assert (f.lead, f.clip, f.channels) == (lead, clip or 255, C) and np.array_equal(f.kept.numpy(), p["keep"])
        m = f.m.numpy()
        assert (m[:, silent] == 0).all() and np.allclose(m[:, p["keep"]], M / p["std"][p["keep"]], rtol=1e-9, atol=0)
        assert np.allclose(f.m0.numpy(), -(m * p["mean"]).sum(1), rtol=1e-12) and np.allclose(f.mean_y.numpy(), p["ybar"], rtol=1e-12)
    with pytest.raises(ValueError):
        kalman.KalmanFilter(-1.0)


def test_a_collinear_pair_of_channels_is_refused():
    x, y = ko.data(7, 2, 600, 2)
    x[5] = x[4]
    with pytest.raises(ValueError, match="positive definite"):
        kalman.KalmanFilter(0.0).fit(host_stats(ko.stats(x, y), 0, None, 7))


def test_stats_add_without_the_junction_pair():
    C, K, T, lead, clip = 7, 2, 900, 2, 4
    x, y = ko.data(C, K, T, 3)
    a = host_stats(ko.stats(x, y, lead, clip, 0, 400), lead, clip, C)
    b = host_stats(ko.stats(x, y, lead, clip, 400, T - lead), lead, clip, C)
    whole = host_stats(ko.stats(x, y, lead, clip), lead, clip, C)
    tot = sum([a, b])
    assert tot.w.n == whole.w.n == T - lead and torch.equal(tot.w.gram, whole.w.gram) and torch.equal(tot.w.sum_x, whole.w.sum_x)
    assert (a.n_pairs, b.n_pairs, tot.n_pairs, whole.n_pairs) == (399, T - lead - 401, T - lead - 2, T - lead - 1)
    # what is missing is exactly the pair (399, 400) across the junction
    u, v = torch.from_numpy(y[:, 399 + lead].astype(np.float64)), torch.from_numpy(y[:, 400 + lead].astype(np.float64))
    for got, full, miss in ((tot.sum_a, whole.sum_a, u), (tot.sum_b, whole.sum_b, v), (tot.aa, whole.aa, torch.outer(u, u)),
                            (tot.bb, whole.bb, torch.outer(v, v)), (tot.ab, whole.ab, torch.outer(u, v)), (tot.sum_d, whole.sum_d, v - u),
                            (tot.dd, whole.dd, torch.outer(v - u, v - u)), (tot.ad, whole.ad, torch.outer(u, v - u))):
        assert torch.allclose(got + miss, full, rtol=1e-12, atol=1e-9)
    assert tot.to("cpu").n_pairs == tot.n_pairs
    # the reference, fitted on the concatenation of two folds that are not neighbours, counts the spurious pair; the sum does not
    far = host_stats(ko.stats(x, y, lead, clip, 600, T - lead), lead, clip, C)
    f = kalman.KalmanFilter(0.0).fit(a + far)
    Y = np.concatenate([y[:, lead:400 + lead], y[:, 600 + lead:]], 1).T.astype(np.float64)
    X1, X2 = np.delete(Y[:-1], 399, 0), np.delete(Y[1:], 399, 0)
    A = ko.ridge(X1, X2, 0.0)
    assert np.abs(f.A.numpy() - A).max() <= 64 * D_REF_W * np.abs(A).max()
    assert np.abs(ko.ridge(Y[:-1], Y[1:], 0.0) - A).max() > 1e-6 * np.abs(A).max()


def test_the_gain_table_converges_and_a_tight_tolerance_raises():
    for C, K, T, lead, clip in FIT_SHAPES[:2]:
        x, y = ko.data(C, K, T, 1)
        f = kalman.KalmanFilter(0.0).fit(host_stats(ko.stats(x, y, lead, clip), lead, clip, C))
        F, B = f.gains()
        p = ko.prepare(x, y, lead, clip)
        Fo, Bo, _M = ko.gain_table(ko.reference_fit(p["Z"], p["Y"], 0.0))
        print("%d x %d: the gains settle after %d steps (the oracle's after %d)" % (C, T, len(F), len(Fo)))
        assert 3 <= len(F) <= 400 and F.shape == B.shape == (len(F), K, K) and abs(len(F) - len(Fo)) <= 2
        n = min(len(F), len(Fo))
        assert np.abs(F[:n] - Fo[:n]).max() <= 64 * D_KALMAN * np.abs(Fo).max() and np.abs(B[:n] - Bo[:n]).max() <= 64 * D_KALMAN * np.abs(Bo).max()
        assert np.abs(F[-1] - F[-2]).max() <= 2.0 ** -50 * np.abs(F[-1]).max() and np.abs(B[-1] - B[-2]).max() <= 2.0 ** -50 * np.abs(B[-1]).max()
        assert np.abs(np.linalg.eigvals(F[-1])).max() < 1                       # the steady filter forgets
        assert len(f.gains(1e-6)[0]) < len(F)
        with pytest.raises(ValueError, match="after 4096 steps: use a tol above"):
            f.gains(-1.0)                                                       # (no change is small enough)
    with pytest.raises(ValueError):
        kalman.KalmanFilter(0.0).gains()


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=str)
def test_the_information_form_agrees_with_the_explicit_recursion(shape):
    C, K, T, lead, clip = shape
    x, y = ko.data(C, K, T, 1)
    p = ko.prepare(x, y, lead, clip)
    for alpha in (0.0, 1e-2):
        model = ko.reference_fit(p["Z"], p["Y"], alpha)
        ref = ko.reference_predict(model, p["Z"], p["Y"][0])
        got = ko.information_predict(model, p["Z"], p["Y"][0])
        d = (np.abs(got - ref).max(0) / p["Y"].std(0)).max()
        cc = [np.corrcoef(ref[:, j], p["Y"][:, j])[0, 1] for j in range(K)]
        print("%s alpha %g: the two routes differ by %.2e of the state's standard deviation; r = %s" % (shape, alpha, d, np.round(cc, 3)))
        assert d <= D_KALMAN
        assert min(cc) > 0.6                                                    # the data give a Kalman filter something to track


@pytest.mark.parametrize("i", range(len(SCAN_CASES)))
def test_the_tiled_scan_agrees_with_the_serial_one(i):
    k, cols, ranges, n_gain, radius, _inplace, _pitched = SCAN_CASES[i]
    v, F, B, init = scan_inputs(i)
    ref = scan_reference(i)
    got = ko.tiled_scan(v, ranges, F, B, init, TILE)
    inside = np.zeros(cols, bool)
    for a, b in ranges:
        inside[a:b] = True
        if b > a:
            assert np.array_equal(ref[:, a], init[ranges.index((a, b))])
    assert np.isnan(ref[:, ~inside]).all() and np.isnan(got[:, ~inside]).all() and np.isfinite(ref[:, inside]).all()
    d = np.abs(got[:, inside] - ref[:, inside]).max() / np.abs(ref[:, inside]).max()
    print("case %d (k %d, %d ranges, n_gain %d, radius %g): tiled and serial differ by %.2e of the largest state %.3g"
          % (i, k, len(ranges), n_gain, radius, d, np.abs(ref[:, inside]).max()))
    assert d <= D_SCAN
    # another tile size is another rounding, not another result
    other = ko.tiled_scan(v, ranges, F, B, init, 37)
    assert np.abs(other[:, inside] - ref[:, inside]).max() <= 4 * D_SCAN * np.abs(ref[:, inside]).max()


def test_host_matrices_are_refused(monkeypatch):
    monkeypatch.setattr(_kalman, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_wiener, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_ingest, "lib", lambda: pytest.fail("the library was loaded"))
    x, y = ko.data(7, 2, 100, 0)
    f = kalman.KalmanFilter(0.0).fit(host_stats(ko.stats(x, y), 0, None, 7))
    for bad in (x, torch.from_numpy(x)):
        with pytest.raises(ValueError, match="no CPU path"):
            kalman.stats(bad, torch.from_numpy(y))
        with pytest.raises(ValueError, match="no CPU path"):
            f.predict(bad)
        with pytest.raises(ValueError, match="no CPU path"):
            f.score(bad, torch.from_numpy(y))
        with pytest.raises(ValueError, match="no CPU path"):
            kalman.cross_validate(bad, torch.from_numpy(y))
    with pytest.raises(ValueError, match="after fit"):
        kalman.KalmanFilter(0.0).predict(torch.from_numpy(x))
