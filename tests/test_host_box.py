"""The moving-average window without a GPU (include/muahuff_smooth.h, libmuahuff_smooth.so, smooth.py, wiener.stats(window=)):
the ABI's three descriptions agree and the four older libraries are as they were, every argument error comes back before
a pointer is used -- with the text tests/box_check.cpp prints, which is csrc/mh_smooth_layout.hpp built alone under
AddressSanitizer + UBSan --, the tiles, the halos, the dwords a workgroup may load and the capped grids hold over a sweep
of shapes, the oracle's smoothed design is the triple loop of the definition, the fit from window statistics agrees with
least squares on the explicit z-scored design, and a constant channel is handled as cascade.cross_validate documents."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _cascade, _ingest, _lib, _smooth, _wiener, smooth, wiener
from tests import box_oracle as bo
from tests import wiener_oracle as wo
from tests.test_host_wiener import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "box_check.cpp")
# mh_smooth_layout.hpp: kBoxTileCols, kBoxMaxBlocks, kBoxSpan, kBoxfTile, kBoxfMaxBlocks
TILE_COLS, MAX_BLOCKS, SPAN, F32_TILE, F32_MAX_BLOCKS = 3824, 2048, 4096, 256, 4096

# The disagreement between the routes of test_the_fit_from_window_statistics_agrees_with_least_squares (least squares on
# the explicit z-scored smoothed design against wo.fit_from_stats on its statistics) on C = 7, L = 5, K = 2, T = 4000, lead
# 3, alpha 0, 1e-2 and 1, no constant channel, relative to the largest weight, as measured per (window, clip), the largest
# over the three alphas: the weights (4, 2) 1.56e-14, (50, None) 1.23e-12, (200, 39) 1.74e-11; the bias 9.09e-14, 6.15e-13,
# 1.66e-11.  Smoothed lags are nearly collinear (the z-scored Gram matrix has a condition number of 30, 7.8e2 and 3.3e4
# where the unsmoothed one has 2.5), which is why these are looser than D_REF_W of tests/test_host_wiener.py.  Recorded
# at twice the largest per window, since a BLAS or LAPACK may sum in another order elsewhere.  WienerFilter.fit (torch,
# Cholesky; measured here at 1.3e-14, 1.1e-12, 3.8e-11 and 2.0e-14, 9.3e-13, 2.1e-11) is allowed 64 times these, and so is
# the device's fit in tests/test_gpu_box.py.
D_BOX_W = {4: 3.2e-14, 50: 2.5e-12, 200: 3.5e-11}
D_BOX = {4: 1.9e-13, 50: 1.3e-12, 200: 3.4e-11}
WINDOWS = [(4, 2), (50, None), (200, 39)]


@pytest.fixture(scope="module", autouse=True)
def built():
    b = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    b.build_smooth()
    b.build(), b.build_ingest(), b.build_wiener(), b.build_cascade()   # (no-ops when fresh) the older libraries are looked into below


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_smooth.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhs_\w+)\s*\(", code))
    assert declared == set(_smooth.PROTOTYPES) == {"mhs_version", "mhs_last_error", "mhs_box", "mhs_box_f32"}
    nm = subprocess.run(["nm", "-D", "--defined-only", _smooth.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared                                  # nothing else is exported
    for fn in ("mhs_box", "mhs_box_f32"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % fn, code).group(1)
        assert len(args.split(",")) == len(_smooth.PROTOTYPES[fn][1])
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_smooth.hpp", "csrc/mh_smooth_layout.hpp", "csrc/exports_smooth.map"} <= set(build.SMOOTH_HEADERS)
    assert build.SMOOTH_SOURCES == ["csrc/mh_smooth.hip"] and build.SMOOTH_SO == _smooth.SO
    with open(os.path.join(ROOT, "include", "muahuff.h")) as f:
        version = int(re.search(r"#define\s+MH_VERSION\s+(\d+)", f.read()).group(1))
    assert _smooth.lib().mhs_version() == version == 103 == _wiener.lib().mhw_version()
    assert muahuff.smooth is smooth and muahuff._smooth is _smooth
    # the new entry points went into none of the older libraries
    older = list(_ingest.PROTOTYPES) + list(_lib.PROTOTYPES) + list(_wiener.PROTOTYPES) + list(_cascade.PROTOTYPES)
    assert not any(n.startswith("mhs_") for n in older)
    for so in (build.SO, build.INGEST_SO, build.WIENER_SO, build.CASCADE_SO):
        assert "mhs_" not in subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert (_smooth.TILE_COLS, _smooth.MAX_BLOCKS, _smooth.MAX_WINDOW, _smooth.MAX_K) == (TILE_COLS, MAX_BLOCKS, 256, 8)


# ---- argument errors ---------------------------------------------------------------------------------------------------
BOX = ("x", "x_row_stride", "rows", "cols", "window", "clip", "lo", "hi", "out_row_stride")
BOXF = ("in", "in_row_stride", "k", "cols", "window", "bias", "out", "out_row_stride")
POINTERS = ("x", "lo", "hi", "in", "bias", "out")
T40, T48 = 1 << 40, 1 << 48


def _args(order, **over):
    """the arguments of mhs_box / mhs_box_f32 with host stand-ins for the device buffers (kept alive in the first item);
    a pointer given as the name of another one starts where that one does (before any shift)"""
    keep = {k: np.zeros(4096, np.uint64) for k in POINTERS if k in order}
    a = dict(x_row_stride=128, rows=3, cols=100, window=5, clip=39, out_row_stride=112, in_row_stride=400, k=2)
    a = {k: v for k, v in a.items() if k in order}
    for k, v in keep.items():
        a[k] = v.ctypes.data + (-v.ctypes.data) % 16
    alias = {k: over.pop(k) for k in list(over) if isinstance(over[k], str)}
    shift = {k[:-6]: over.pop(k) for k in list(over) if k.endswith("_shift")}
    for k, v in over.items():
        a[k] = (0 if v is None else v)
    for k, other in alias.items():
        a[k] = a[other]
    for k, s in shift.items():
        a[k] += s
    return keep, a


def _call(order, a):
    L = _smooth.lib()
    vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in order]
    rc = (L.mhs_box if order is BOX else L.mhs_box_f32)(*vals, None)
    return rc, L.mhs_last_error().decode()


BOX_BAD = [dict(x=None), dict(lo=None), dict(window=0), dict(window=257), dict(clip=0), dict(clip=256), dict(rows=0), dict(rows=65537),
           dict(cols=0), dict(cols=T40, x_row_stride=T40 + 8, out_row_stride=T40),
           dict(hi=None, window=4, clip=64), dict(hi=None, window=256, clip=1), dict(hi=None, window=2, clip=255),
           dict(lo_shift=8), dict(lo_shift=1), dict(hi_shift=4), dict(out_row_stride=104), dict(out_row_stride=120),
           dict(x_row_stride=103), dict(x_row_stride=0), dict(x_row_stride=T48), dict(out_row_stride=96), dict(out_row_stride=0),
           dict(out_row_stride=T48), dict(lo="x"), dict(hi="x"), dict(lo="x", lo_shift=352), dict(hi="x", hi_shift=16),
           dict(hi="lo"), dict(hi="lo", hi_shift=320), dict(cols=40, x_row_stride=64, hi="lo", hi_shift=32),
           dict(cols=40, x_row_stride=64, hi="lo", hi_shift=80), dict(cols=40, x_row_stride=64, lo="hi", lo_shift=192), dict(rows=1, hi="lo", hi_shift=96), dict(rows=1, lo="x", lo_shift=96)]
BOX_GOOD = [dict(), dict(hi=None, window=5, clip=51), dict(hi=None, window=255, clip=1, x_row_stride=354), dict(hi=None, window=1, clip=255),
            dict(window=4, clip=64), dict(window=1), dict(window=256, clip=255, x_row_stride=355), dict(x_shift=1), dict(x_shift=15, x_row_stride=104),
            dict(rows=1, x_row_stride=0, out_row_stride=0), dict(rows=1, hi="lo", hi_shift=112), dict(rows=1, lo="x", lo_shift=112),
            dict(hi="lo", hi_shift=336), dict(cols=40, x_row_stride=64, hi="lo", hi_shift=48),   # (interleaved rows)
            dict(cols=40, x_row_stride=64, lo="hi", lo_shift=64 + 112 * 7), dict(rows=65536, lo=1 << 50, hi=1 << 51), dict(clip=1), dict(clip=255),
            dict(cols=T40 - 1, x_row_stride=T40 + 3, out_row_stride=T40, lo=1 << 60, hi=1 << 61),
            dict(x_row_stride=T48 - 1, out_row_stride=T48 - 16, lo=1 << 60, hi=1 << 61)]
BOXF_BAD = [dict(bias=None), dict(out=None), dict(k=0), dict(k=9), dict(cols=0),
            dict(cols=T40, in_row_stride=4 * T40, out_row_stride=4 * T40), dict(window=0), dict(window=257), dict(in_shift=2), dict(out_shift=1),
            dict(bias_shift=2), dict(in_row_stride=402), dict(out_row_stride=398), dict(in_row_stride=396), dict(out_row_stride=0),
            dict(in_row_stride=T48), dict(out="in"), dict(out="in", out_shift=796), dict(out="bias"), dict(out="bias", out_shift=4)]
BOXF_BAD.insert(0, {"in": None})
BOXF_GOOD = [dict(), dict(k=1, in_row_stride=0, out_row_stride=0), dict(k=8), dict(window=1), dict(window=256), dict(in_shift=4, out_shift=8),
             dict(out="in", out_shift=800), dict(in_row_stride=404, out_row_stride=408),
             dict(cols=T40 - 1, in_row_stride=4 * T40, out_row_stride=4 * T40, out=1 << 60, bias=1 << 61)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items()) or "default"   # noqa: E731


def _boxf_args(**over):
    keep, a = _args(BOXF, out_row_stride=over.pop("out_row_stride", 400), **over)
    return keep, a


@pytest.mark.parametrize("bad", BOX_BAD, ids=_ids)
def test_box_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(BOX, **bad)
    rc, msg = _call(BOX, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhs_box:"), (rc, msg)


@pytest.mark.parametrize("bad", BOXF_BAD, ids=_ids)
def test_box_f32_argument_errors_come_before_any_device_work(bad):
    keep, a = _boxf_args(**bad)
    rc, msg = _call(BOXF, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhs_box_f32:"), (rc, msg)


def _line(word, order, a):
    return word + " " + " ".join(str(a[k]) for k in order) + "\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("box") / "box_check_asan")
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
    for word, order, make, bad, good, rules in (("box", BOX, lambda **o: _args(BOX, **o), BOX_BAD, BOX_GOOD, 10),
                                                ("boxf", BOXF, _boxf_args, BOXF_BAD, BOXF_GOOD, 8)):
        cases = [make(**b) for b in bad]
        lines = _run(exe, "".join(_line(word, order, a) for _k, a in cases))
        assert len(lines) == len(bad)
        seen = set()
        for (keep, a), ln, b in zip(cases, lines, bad):
            rc, msg = _call(order, a)
            assert ln == "error %d %s" % (rc, msg) and rc == _lib.ERR_ARG, (b, ln, msg)
            seen.add(re.sub(r"\d+", "#", msg))
        assert len(seen) >= rules, seen                            # the table reaches every rule, not one message over and over
        ok = [make(**g) for g in good]
        # (accepted arguments would be launched: they are checked through the program alone)
        assert _run(exe, "".join(_line(word, order, a) for _k, a in ok)) == ["ok"] * len(good), word
    # hi may be NULL exactly up to window * clip = 255
    for w, q, ok in ((5, 51, True), (1, 255, True), (255, 1, True), (4, 64, False), (16, 16, False), (256, 1, False)):
        keep, a = _args(BOX, hi=None, window=w, clip=q, x_row_stride=512)
        assert _run(exe, _line("box", BOX, a)) == (["ok"] if ok else ["error -1 mhs_box: hi is NULL and window * clip = %d is above 255" % (w * q)])


def layout(rows, cols, k):
    """mh_smooth_layout.hpp's rules, restated -> [tiles, items, grid, f32 tiles, f32 items, f32 grid]"""
    tiles = -(-cols // TILE_COLS)
    ft = -(-cols // F32_TILE)
    return [tiles, rows * tiles, min(rows * tiles, MAX_BLOCKS), ft, ft * k, min(ft * k, F32_MAX_BLOCKS)]


def test_tiles_halos_loads_and_grids_over_the_sweep(exe):
    """box_check asserts per shape: the tiles partition the columns on 16-byte boundaries, the span holds the shift, the
    tile and the halo, every byte a tile needs is loaded and every loaded dword holds a byte of the row, the grids are
    under their caps and the stride loops reach every item once"""
    grid = []
    for rows in (1, 5, 70, 65536):
        for cols in (1, 3, 63, TILE_COLS - 1, TILE_COLS, TILE_COLS + 1, 3 * TILE_COLS + 5, 72000, 10 ** 7):
            for window, k in ((1, 1), (2, 3), (5, 2), (50, 2), (200, 8), (256, 8)):
                x = (1 << 30) + (rows * 7 + cols * 3 + window) % 16          # the first byte at every offset 0..15 over the sweep
                grid.append((rows, cols, window, k, x, cols + window - 1 + (cols + rows) % 5))
    for off in range(16):                                                   # ... and each of them at the tile-edge shapes
        grid.append((3, TILE_COLS + 1, 256, 1, (1 << 30) + off, TILE_COLS + 256 + off))
        grid.append((2, 1, 1, 1, (1 << 30) + off, 1 + off % 3))
    grid += [(1, T40 - 1, 256, 8, (1 << 30) + 5, 0), (65536, T40 - 1, 1, 1, 3, T40 + 3), (2, T40 - 1, 200, 2, 1 << 20, (1 << 47) + 1),
             (96, 72000, 50, 2, 1 << 30, 72064), (1024, 10 ** 7, 200, 2, 1 << 30, 10 ** 7 + 256)]
    # the shape tests/test_gpu_box.py runs past the cap
    grid += [(1, MAX_BLOCKS * TILE_COLS + 1, 2, 1, (1 << 30) + 1, 0)]
    assert {g[4] % 16 for g in grid} == set(range(16))
    lines = _run(exe, "".join("layout %d %d %d %d %d %d\n" % g for g in grid))
    assert len(lines) == len(grid)
    strided_box = strided_f32 = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == layout(g[0], g[1], g[3]), (g, got)
        strided_box += got[1] > got[2]
        strided_f32 += got[4] > got[5]
    assert strided_box > 20 and strided_f32 > 20
    assert layout(1, MAX_BLOCKS * TILE_COLS + 1, 1)[:3] == [MAX_BLOCKS + 1, MAX_BLOCKS + 1, MAX_BLOCKS]
    assert 15 + TILE_COLS + 255 <= SPAN and TILE_COLS % 16 == 0


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_the_oracle_is_the_triple_loop_of_the_definition():
    rng = np.random.RandomState(1)
    C, T, L, g, w, q = 3, 23, 4, 2, 5, 3
    x = rng.randint(0, 7, (C, T)).astype(np.uint8)
    y = rng.randn(2, T).astype(np.float32)
    X, Y = bo.design(x, y, L, g, q, w)
    assert X.shape == (T - g - (L - 1), L * C) and X.dtype == np.int64
    for t in range(L - 1, T - g):
        for l in range(L):
            for c in range(C):
                want = sum(min(int(x[c, t - l - j]), q) for j in range(min(w - 1, t - (L - 1)) + 1))
                assert X[t - (L - 1), l * C + c] == want
        assert np.array_equal(Y[t - (L - 1)], y[:, t + g].astype(np.float64))
    part, _ = bo.design(x, y, L, g, q, w, 6, 11)
    assert np.array_equal(part, X[6 - (L - 1):11 - (L - 1)])
    assert np.array_equal(bo.design(x, y, L, g, q, 1)[0], wo.design(x, y, L, g, q)[0])           # window 1 is no window
    # behind the warm-up the features are the box sums of the clipped counts
    B = bo.box(x, w, q)                                          # B[:, i] is the box that ends at column i + w - 1
    for l in range(L):
        assert np.array_equal(X[w - 1:, l * C:(l + 1) * C].T, B[:, L - 1 - l:L - 1 - l + X.shape[0] - (w - 1)])
    lo, hi = bo.planes(np.full((2, 300), 255, np.uint8), 256, None)
    assert (lo.astype(np.int64) + 256 * hi.astype(np.int64) == 65280).all() and lo.shape == (2, 45) and lo.dtype == hi.dtype == np.uint8
    # the float box: integers stay integers, the front columns sum fewer
    p = rng.randint(-9, 10, (2, 12)).astype(np.int64)
    out, mag = bo.box_f32(p, 4, np.array([3, -2]))
    for j in range(2):
        for i in range(12):
            assert out[j, i] == [3, -2][j] + p[j, max(0, i - 3):i + 1].sum()
            assert mag[j, i] == [3, 2][j] + np.abs(p[j, max(0, i - 3):i + 1]).sum()


# ---- the fit -------------------------------------------------------------------------------------------------------------
C, L, K, T, LEAD = 7, 5, 2, 4000, 3


def box_data():
    """tests.test_host_wiener.data() with its silent channel 3 replaced by counts: no constant channel"""
    x, y = data(C, L, K, T)
    x[3] = np.minimum(np.random.RandomState(77).poisson(1.2, T), 255).astype(np.uint8)
    return x, y


def _host_stats(r, clip, window):
    t = torch.from_numpy
    return wiener.Stats(r["n"], t(r["sum_x"]), t(r["gram"]), t(r["xty"]), t(r["sum_y"]), t(r["sum_yy"]), L, LEAD, 255 if clip is None else clip,
                        C, window)


@pytest.mark.parametrize("w,clip", WINDOWS)
def test_the_fit_from_window_statistics_agrees_with_least_squares(w, clip):
    x, y = box_data()
    X, Y = bo.design(x, y, L, LEAD, clip, w)
    Z, keep, _mean, _std = wo.zscored(X)
    assert len(keep) == C * L
    print("window %d clip %s: condition number of the z-scored Gram matrix %.3g" % (w, clip, np.linalg.cond(Z.T @ Z / len(Z))))
    r = bo.stats(x, y, L, LEAD, clip, w)
    assert r["gram"].max() < 2 ** 53 and r["n"] == T - LEAD - (L - 1)
    for alpha in (0, 1e-2, 1):
        wt, b = wo.fit_from_stats(r["n"], r["sum_x"], r["gram"], r["xty"], r["sum_y"], alpha, L, C)
        w2, b2 = wo.fit_lstsq(X, Y, alpha)
        scale = np.abs(wt).max()
        dw, db = np.abs(w2 - wt.reshape(K, L * C).T).max() / scale, np.abs(b2 - b).max() / scale
        f = wiener.WienerFilter(alpha).fit(_host_stats(r, clip, w))
        tw, tb = np.abs(f.weights.numpy() - wt).max() / scale, np.abs(f.bias.numpy() - b).max() / scale
        print("window %d clip %s alpha %g: the two host routes differ by %.2e (weights) %.2e (bias), torch by %.2e %.2e" % (w, clip, alpha, dw, db, tw, tb))
        assert dw <= D_BOX_W[w] and db <= D_BOX[w]
        assert tw <= 64 * D_BOX_W[w] and tb <= 64 * D_BOX[w]
        assert f.window == w and f.clip == (clip or 255) and tuple(f.weights.shape) == (K, L, C)


def test_stats_carry_the_window_and_refuse_a_mismatch():
    x, y = box_data()
    a = _host_stats(bo.stats(x, y, L, LEAD, 2, 4, L - 1, 2000), 2, 4)
    b = _host_stats(bo.stats(x, y, L, LEAD, 2, 4, 2000, T - LEAD), 2, 4)
    whole = _host_stats(bo.stats(x, y, L, LEAD, 2, 4), 2, 4)
    tot = a + b
    assert tot.window == 4 and tot.to("cpu").window == 4 and torch.equal(tot.gram, whole.gram) and torch.equal(tot.sum_x, whole.sum_x)
    with pytest.raises(ValueError):
        a + _host_stats(bo.stats(x, y, L, LEAD, 2, 5, 2000, T - LEAD), 2, 5)
    plain = wiener.Stats(a.n, a.sum_x, a.gram, a.xty, a.sum_y, a.sum_yy, L, LEAD, 2, C)
    assert plain.window == 1
    with pytest.raises(ValueError):
        a + plain


def test_a_constant_channel_is_constant_only_behind_the_warm_up():
    """channel 3 holds 2 in every bin.  Over ranges that hold the warm-up its five lags are one and the same ramp: alpha 0
    is refused, alpha 1e-2 fits.  Over ranges that start at L-1 + w-1 its features are constant, are dropped, and get
    weights that are exactly zero."""
    w, clip = 50, None
    x, y = box_data()
    x[3] = 2
    r = bo.stats(x, y, L, LEAD, clip, w)
    with pytest.raises(ValueError, match="positive definite"):
        wiener.WienerFilter(0.0).fit(_host_stats(r, clip, w))
    f = wiener.WienerFilter(1e-2).fit(_host_stats(r, clip, w))
    assert bool(torch.isfinite(f.weights).all()) and bool((f.weights[:, :, 3] != 0).any())
    # (the five ramps stay collinear, so the ridge alone decides how their weight is shared: no tight comparison here)
    wt, _b = wo.fit_from_stats(r["n"], r["sum_x"], r["gram"], r["xty"], r["sum_y"], 1e-2, L, C)
    other = [c for c in range(C) if c != 3]
    assert np.abs(f.weights.numpy() - wt)[:, :, other].max() <= 64 * D_BOX_W[w] * np.abs(wt).max()
    r = bo.stats(x, y, L, LEAD, clip, w, L - 1 + w - 1, T - LEAD)
    for alpha in (0.0, 1e-2):
        f = wiener.WienerFilter(alpha).fit(_host_stats(r, clip, w))
        assert bool((f.weights[:, :, 3] == 0).all()) and bool((f.weights[:, :, :3] != 0).all())


def test_host_matrices_and_bad_windows_are_refused(monkeypatch):
    monkeypatch.setattr(_smooth, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_wiener, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_ingest, "lib", lambda: pytest.fail("the library was loaded"))
    x, y = data(T=100)
    for bad in (x, torch.from_numpy(x)):
        with pytest.raises(ValueError, match="no CPU path"):
            smooth.box_sum(bad, 5)
        with pytest.raises(ValueError, match="no CPU path"):
            smooth.moving_average(bad, 5)
        with pytest.raises(ValueError, match="no CPU path"):
            wiener.stats(bad, torch.from_numpy(y), 5, window=4)
    for w in (0, 257, -1):
        with pytest.raises(ValueError, match="outside 1..256"):
            smooth._window(w, 1)
    assert smooth._window(256, 255) == 256 and smooth._window(256, 1) == 256 and smooth._window(1, 255) == 1
    with pytest.raises(ValueError, match="65535"):                 # (out of reach while the clip ends at 255: 256 * 255 = 65280)
        smooth._window(256, 256)
    # (wiener.stats refuses a host matrix before it looks at the window: its own window check runs in
    # tests/test_gpu_box.py::test_window_stats_equal_the_explicit_smoothed_design)


def test_a_filter_set_up_by_hand_without_a_window_takes_the_route_without_one(monkeypatch):
    """tools/bench_cascade.py and users of the earlier release assign weights, bias, lags, lead, clip and channels and
    call predict(): a new filter's window is 1, so predict() is one mhw_fir and mhs_box_f32 is never reached"""
    f = wiener.WienerFilter(0.0)
    assert f.window == 1
    f.weights, f.bias = torch.zeros((K, L, C), dtype=torch.float64), torch.zeros((K,), dtype=torch.float64)
    f.lags, f.lead, f.clip, f.channels = L, 0, 255, C
    calls = []
    x = torch.zeros((C, 40), dtype=torch.uint8)
    monkeypatch.setattr(wiener, "_matrix", lambda m, who: (m, int(m.shape[0]), int(m.shape[1])))
    monkeypatch.setattr(_wiener, "fir", lambda *a: calls.append("fir"))
    monkeypatch.setattr(_smooth, "box_f32", lambda *a: calls.append("box_f32"))
    out = f.predict(x)
    assert calls == ["fir"] and tuple(out.shape) == (K, 40 - L + 1)
    f.window = 50                                                  # what fit() records from Stats with a window
    f.predict(x)
    assert calls == ["fir", "fir", "box_f32"]
