"""The Wiener filter without a GPU (include/muahuff_wiener.h, libmuahuff_wiener.so, wiener.py): the ABI's three descriptions
agree and the two older libraries are as they were, every argument error comes back before a pointer is used -- with the
text tests/wiener_check.cpp prints, which is csrc/mh_wiener_layout.hpp built alone under AddressSanitizer + UBSan --, the
runs, the scratch, the tiles, the M-tiles and the capped grids hold over a sweep of shapes, the fit restated from the
statistics agrees with scikit-learn's Ridge and with least squares on the explicit z-scored design, and folds() is the
reference's split."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _ingest, _lib, _wiener, wiener
from tests import wiener_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "wiener_check.cpp")
RUN, MAX_BLOCKS, SUM_THREADS, SUM_MAX_BLOCKS = 32768, 4096, 256, 4096     # mh_wiener_layout.hpp: kXty*
TILE_COLS, M_ROWS, FIR_MAX_BLOCKS = 512, 32, 4096                        # kFirTileCols, kFirMRows, kFirMaxBlocks

# The disagreement between the three routes of test_the_fit_from_statistics_agrees_with_ridge_and_least_squares on
# C = 7, L = 5, K = 2, T = 4000, relative to the largest weight, as measured: 1.3e-15 .. 4.5e-15 on the weights, 2.1e-14
# .. 1.5e-13 on the bias (ybar - sum w mean cancels some hundred times the largest weight).  Recorded at twice the
# largest, since a BLAS may sum in another order elsewhere.  tests/test_gpu_wiener.py allows the device solver 64 times
# D_REF_W on the weights and 64 times D_REF on the bias.
D_REF_W = 9e-15
D_REF = 3e-13


@pytest.fixture(scope="module", autouse=True)
def built():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_wiener()


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_wiener.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhw_\w+)\s*\(", code))
    assert declared == set(_wiener.PROTOTYPES) == {"mhw_version", "mhw_last_error", "mhw_xty_scratch_bytes", "mhw_xty", "mhw_fir"}
    nm = subprocess.run(["nm", "-D", "--defined-only", _wiener.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared                                  # nothing else is exported
    for fn in ("mhw_xty", "mhw_fir", "mhw_xty_scratch_bytes"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % fn, code).group(1)
        assert len(args.split(",")) == len(_wiener.PROTOTYPES[fn][1])
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_wiener.hpp", "csrc/mh_wiener_layout.hpp", "csrc/exports_wiener.map"} <= set(build.WIENER_HEADERS)
    assert _wiener.lib().mhw_version() == 103
    assert muahuff.wiener is wiener and muahuff._wiener is _wiener
    # the new entry points went into neither of the older libraries
    assert not any(n.startswith("mhw_") for n in list(_ingest.PROTOTYPES) + list(_lib.PROTOTYPES))


# ---- argument errors ---------------------------------------------------------------------------------------------------
XTY = ("x", "x_row_stride", "rows", "cols", "lags", "clip", "y", "y_row_stride", "k", "out", "accumulate", "scratch", "scratch_bytes")
FIR = ("x", "x_row_stride", "rows", "cols", "lags", "clip", "w", "bias", "k", "out", "out_row_stride")
POINTERS = ("x", "y", "out", "scratch", "w", "bias")


def _args(order, **over):
    """the arguments of mhw_xty / mhw_fir with host stand-ins for the device buffers (kept alive in the first item)"""
    keep = {k: np.zeros(4096, np.uint64) for k in POINTERS if k in order}
    a = dict(x_row_stride=128, rows=3, cols=100, lags=5, clip=255, y_row_stride=400, k=2, accumulate=0,
             scratch_bytes=3 * 5 * 2 * 8, out_row_stride=400)
    a = {k: v for k, v in a.items() if k in order}
    for k, v in keep.items():
        a[k] = v.ctypes.data + (-v.ctypes.data) % 16
    shift = {k[:-6]: over.pop(k) for k in list(over) if k.endswith("_shift")}
    for k, v in over.items():
        a[k] = (0 if v is None else v)
    for k, s in shift.items():
        a[k] += s
    return keep, a


def _call(order, a):
    L = _wiener.lib()
    vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in order]
    rc = (L.mhw_xty if order is XTY else L.mhw_fir)(*vals, None)
    return rc, L.mhw_last_error().decode()


T40 = 1 << 40
SHAPE_BAD = [dict(lags=0), dict(lags=33), dict(k=0), dict(k=9), dict(rows=0), dict(rows=65537, x_row_stride=128),
             dict(cols=0), dict(cols=T40, x_row_stride=T40 + 8, y_row_stride=4 * T40, out_row_stride=4 * T40,
                                scratch_bytes=1 << 62),
             dict(clip=0), dict(clip=256), dict(x=None), dict(out=None), dict(x_row_stride=103), dict(x_row_stride=0)]
XTY_BAD = SHAPE_BAD + [dict(y=None), dict(scratch=None), dict(accumulate=2), dict(out_shift=4), dict(out_shift=1),
                       dict(scratch_shift=4), dict(y_shift=2), dict(y_row_stride=402), dict(y_row_stride=396),
                       dict(y_row_stride=0), dict(scratch_bytes=3 * 5 * 2 * 8 - 8), dict(scratch_bytes=0),
                       dict(cols=RUN + 1, x_row_stride=RUN + 8, y_row_stride=4 * RUN + 4, scratch_bytes=3 * 5 * 2 * 8)]
FIR_BAD = SHAPE_BAD + [dict(w=None), dict(bias=None), dict(w_shift=2), dict(bias_shift=1), dict(out_shift=2),
                       dict(out_row_stride=402), dict(out_row_stride=396), dict(out_row_stride=0)]
XTY_GOOD = [dict(), dict(accumulate=1), dict(x_shift=1), dict(x_shift=3, x_row_stride=104), dict(rows=1, x_row_stride=0),
            dict(k=1, y_row_stride=0), dict(lags=32, x_row_stride=131, scratch_bytes=3 * 32 * 2 * 8), dict(clip=1),
            dict(k=8, y_row_stride=400, scratch_bytes=3 * 5 * 8 * 8), dict(rows=65536, scratch_bytes=65536 * 5 * 2 * 8),
            dict(cols=T40 - 1, x_row_stride=T40 + 3, y_row_stride=4 * T40, scratch_bytes=(1 << 25) * 3 * 5 * 2 * 8)]
FIR_GOOD = [dict(), dict(x_shift=1), dict(rows=1, x_row_stride=0), dict(k=1, out_row_stride=0), dict(lags=32, x_row_stride=131),
            dict(clip=1), dict(k=8), dict(rows=65536), dict(cols=T40 - 1, x_row_stride=T40 + 3, out_row_stride=4 * T40)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items()) or "default"   # noqa: E731


@pytest.mark.parametrize("bad", XTY_BAD, ids=_ids)
def test_xty_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(XTY, **bad)
    rc, msg = _call(XTY, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhw_xty:"), (rc, msg)


@pytest.mark.parametrize("bad", FIR_BAD, ids=_ids)
def test_fir_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(FIR, **bad)
    rc, msg = _call(FIR, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhw_fir:"), (rc, msg)


SCRATCH_BAD = [(0, 100, 5, 2), (65537, 100, 5, 2), (3, 0, 5, 2), (3, T40, 5, 2), (3, 100, 0, 2), (3, 100, 33, 2), (3, 100, 5, 0),
               (3, 100, 5, 9)]


def test_scratch_bytes_and_its_argument_errors():
    L = _wiener.lib()
    b = ct.c_uint64(7)
    for rows, cols, lags, k in SCRATCH_BAD:
        rc = L.mhw_xty_scratch_bytes(rows, cols, lags, k, ct.byref(b))
        assert rc == _lib.ERR_ARG and L.mhw_last_error().decode().startswith("mhw_xty_scratch_bytes:") and b.value == 7
    assert L.mhw_xty_scratch_bytes(3, 100, 5, 2, None) == _lib.ERR_ARG
    assert L.mhw_last_error().decode().startswith("mhw_xty_scratch_bytes:")
    with pytest.raises(muahuff.MuaHuffError):
        _wiener.xty_scratch_bytes(3, 100, 33, 2)
    for rows, cols, lags, k in [(3, 100, 5, 2), (1, 1, 1, 1), (70, RUN, 32, 8), (70, RUN + 1, 32, 8), (65536, 3 * RUN + 5, 4, 1),
                                (1024, 10 ** 7, 15, 2), (65536, T40 - 1, 32, 8)]:
        assert _wiener.xty_scratch_bytes(rows, cols, lags, k) == -(-cols // RUN) * rows * lags * k * 8


def _line(word, order, a):
    return word + " " + " ".join(str(a[k]) for k in order) + "\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wiener") / "wiener_check_asan")
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
    for word, order, bad, good in (("xty", XTY, XTY_BAD, XTY_GOOD), ("fir", FIR, FIR_BAD, FIR_GOOD)):
        cases = [_args(order, **b) for b in bad]
        lines = _run(exe, "".join(_line(word, order, a) for _k, a in cases))
        assert len(lines) == len(bad)
        for (keep, a), ln, b in zip(cases, lines, bad):
            rc, msg = _call(order, a)
            assert ln == "error %d %s" % (rc, msg) and rc == _lib.ERR_ARG, (b, ln, msg)
        ok = [_args(order, **g) for g in good]
        assert _run(exe, "".join(_line(word, order, a) for _k, a in ok)) == ["ok"] * len(good), word
    text = "".join("scratch %d %d %d %d 64\n" % s for s in SCRATCH_BAD) + "scratch 3 100 5 2 0\nscratch 3 100 5 2 64\n"
    lines = _run(exe, text)
    head = "error %d mhw_xty_scratch_bytes:" % _lib.ERR_ARG
    assert len(lines) == len(SCRATCH_BAD) + 2 and all(ln.startswith(head) for ln in lines[:-1]) and lines[-1] == "ok"


def layout(rows, cols, lags, k):
    """mh_wiener_layout.hpp's rules, restated -> [runs, items, per_item, scratch_bytes, grid, elements, sum_grid,
    tile_outputs, tiles, per_mtile, mtiles, fir_items, fir_grid]"""
    runs = -(-cols // RUN)
    items, per = runs * rows, lags * k
    elements = rows * per
    tile_outputs = TILE_COLS - (lags - 1)
    tiles, per_mtile = -(-cols // tile_outputs), M_ROWS // lags
    mtiles = -(-k // per_mtile)
    return [runs, items, per, items * per * 8, min(items, MAX_BLOCKS), elements, min(-(-elements // SUM_THREADS), SUM_MAX_BLOCKS),
            tile_outputs, tiles, per_mtile, mtiles, tiles * mtiles, min(tiles * mtiles, FIR_MAX_BLOCKS)]


def test_runs_scratch_tiles_mtiles_and_grids_over_the_sweep(exe):
    """wiener_check asserts per shape: the runs partition [0, cols), the scratch covers every item and every read of the
    sum kernel, the fir tiles own every output once and overlap by lags - 1, the M-tiles hold whole outputs, the grids
    are under their caps and the stride loops reach every item"""
    grid = [(r, c, l, k) for r in (1, 2, 5, 70, 1024, 65536) for c in (1, 63, 481, 512, 513, RUN, RUN + 3, 3 * RUN + 5, 10 ** 7)
            for l, k in ((1, 1), (4, 2), (5, 8), (15, 2), (15, 3), (16, 8), (17, 8), (32, 1), (32, 8))]
    grid += [(1, T40 - 1, 1, 1), (65536, T40 - 1, 32, 8), (1, T40 - 1, 32, 8), (65536, T40 - 1, 1, 1), (96, 72000, 15, 2)]
    # the shapes tests/test_gpu_wiener.py runs past the caps
    grid += [(1, FIR_MAX_BLOCKS * TILE_COLS + 1, 1, 1), (1, (MAX_BLOCKS + 1) * RUN, 1, 1), (4100, 63, 32, 8)]
    lines = _run(exe, "".join("layout %d %d %d %d\n" % g for g in grid))
    assert len(lines) == len(grid)
    strided_xty = strided_fir = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == layout(*g), (g, got)
        strided_xty += got[1] > got[4]
        strided_fir += got[11] > got[12]
    assert strided_xty > 20 and strided_fir > 20
    assert layout(70, 10, 15, 3)[9:11] == [2, 2] and layout(70, 10, 32, 8)[9:11] == [1, 8] and layout(70, 10, 15, 2)[9:11] == [2, 1]
    assert layout(1, FIR_MAX_BLOCKS * TILE_COLS + 1, 1, 1)[11:] == [FIR_MAX_BLOCKS + 1, FIR_MAX_BLOCKS]
    assert layout(1024, 10 ** 7, 15, 2)[:5] == [306, 306 * 1024, 30, 306 * 1024 * 240, MAX_BLOCKS]


# ---- the fit -------------------------------------------------------------------------------------------------------------
def data(C=7, L=5, K=2, T=4000, seed=0):
    """Poisson counts with a few 255s, channel 3 silent; covariates that follow the counts of four bins earlier (so a
    lead of up to 3 bins leaves the cause among the lagged features) plus noise"""
    rng = np.random.RandomState(seed)
    x = np.minimum(rng.poisson(1.2, (C, T)), 255).astype(np.uint8)
    x[rng.rand(C, T) < 0.01] = 255
    x[3] = 0
    mix = rng.randn(K, C)
    y = (mix @ np.roll(np.minimum(x, 4), 4, axis=1).astype(np.float64) + 2.0 * rng.randn(K, T)).astype(np.float32)
    return x, y


def _host_stats(r, L, lead, clip, C):
    t = torch.from_numpy
    return wiener.Stats(r["n"], t(r["sum_x"]), t(r["gram"]), t(r["xty"]), t(r["sum_y"]), t(r["sum_yy"]), L, lead, 255 if clip is None else clip, C)


@pytest.mark.parametrize("alpha", [0, 1e-2, 1])
def test_the_fit_from_statistics_agrees_with_ridge_and_least_squares(alpha):
    C, L, K, lead = 7, 5, 2, 3
    x, y = data(C, L, K)
    r = wo.stats(x, y, L, lead)
    w, b = wo.fit_from_stats(r["n"], r["sum_x"], r["gram"], r["xty"], r["sum_y"], alpha, L, C)
    X, Y = wo.design(x, y, L, lead)
    Z, keep, mean, std = wo.zscored(X)
    assert len(keep) == (C - 1) * L and np.linalg.cond(Z.T @ Z / len(Z)) < 2.5
    scale = np.abs(w).max()
    flat = w.reshape(K, L * C).T
    w2, b2 = wo.fit_lstsq(X, Y, alpha)
    d = [np.abs(w2 - flat).max() / scale, np.abs(b2 - b).max() / scale]
    linear_model = pytest.importorskip("sklearn.linear_model")
    m = linear_model.Ridge(alpha=alpha, fit_intercept=True, solver="svd" if alpha == 0 else "cholesky").fit(Z, Y)
    w3, b3 = wo.unfold(m.coef_.T, m.intercept_, keep, mean, std, L * C)
    d += [np.abs(w3 - flat).max() / scale, np.abs(b3 - b).max() / scale, np.abs(w3 - w2).max() / scale]
    print("alpha %g: disagreement of the three routes %s" % (alpha, ["%.2e" % v for v in d]))
    assert max(d[0], d[2], d[4]) <= D_REF_W and max(d) <= D_REF
    assert (w[:, :, 3] == 0).all()
    # WienerFilter.fit is the same restatement in torch (Cholesky): on host Stats it runs without a device
    f = wiener.WienerFilter(alpha).fit(_host_stats(r, L, lead, None, C))
    assert np.abs(f.weights.numpy() - w).max() / scale <= 64 * D_REF_W and np.abs(f.bias.numpy() - b).max() / scale <= 64 * D_REF
    assert f.weights.dtype == torch.float64 and tuple(f.weights.shape) == (K, L, C) and (f.weights[:, :, 3] == 0).all()


def test_a_singular_fit_says_to_use_alpha():
    x, y = data()
    x[5] = x[4]                                                   # two identical channels
    r = wo.stats(x, y, 5, 3)
    s = _host_stats(r, 5, 3, None, 7)
    with pytest.raises(ValueError, match="alpha > 0"):
        wiener.WienerFilter(0.0).fit(s)
    assert wiener.WienerFilter(1.0).fit(s).weights is not None
    with pytest.raises(ValueError):
        wiener.WienerFilter(-1.0)


def test_stats_add_over_disjoint_ranges_and_refuse_a_mismatch():
    x, y = data()
    whole = _host_stats(wo.stats(x, y, 5, 3), 5, 3, None, 7)
    parts = [_host_stats(wo.stats(x, y, 5, 3, None, a, b), 5, 3, None, 7) for a, b in ((4, 1000), (1000, 2501), (2501, 3997))]
    tot = sum(parts)
    assert tot.n == whole.n and torch.equal(tot.gram, whole.gram) and torch.equal(tot.sum_x, whole.sum_x)
    assert torch.allclose(tot.xty, whole.xty, rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        whole + _host_stats(wo.stats(x, y, 5, 2), 5, 2, None, 7)
    with pytest.raises(ValueError):
        whole + _host_stats(wo.stats(x, y, 5, 3, 2), 5, 3, 2, 7)


@pytest.mark.parametrize("n", [10, 23, 100])
@pytest.mark.parametrize("num_fold", [2, 5])
def test_folds_are_the_reference_split(n, num_fold):
    got, want = wiener.folds(n, num_fold), wo.split_index(n, num_fold)
    assert len(got) == len(want) == num_fold
    for (tr, va, te), (rtr, rva, rte) in zip(got, want):
        cat = np.concatenate([np.arange(a, b) for a, b in tr]) if tr else np.arange(0)
        assert np.array_equal(cat, rtr) and np.array_equal(np.arange(*va), rva) and np.array_equal(np.arange(*te), rte)
    per = n // num_fold
    assert wiener.fold_ranges(n, num_fold, first=4) == [(4 + i * per, 4 + (i + 1) * per) for i in range(num_fold)]
    with pytest.raises(ValueError):
        wiener.folds(n, 1)


def test_host_matrices_and_bad_settings_are_refused(monkeypatch):
    monkeypatch.setattr(_wiener, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_ingest, "lib", lambda: pytest.fail("the library was loaded"))
    x, y = data(T=100)
    for bad in (x, torch.from_numpy(x)):
        with pytest.raises(ValueError, match="no CPU path"):
            wiener.stats(bad, torch.from_numpy(y), 5)
    f = wiener.WienerFilter()
    with pytest.raises(ValueError):
        f.predict(torch.from_numpy(x))
    for kw in (dict(lags=0), dict(lags=33), dict(lags=5, lead=-1), dict(lags=5, lead=96)):
        with pytest.raises(ValueError):
            wiener._settings(kw["lags"], kw.get("lead", 0), 7, 100)
    with pytest.raises(ValueError, match="16384"):
        wiener._settings(17, 0, 1024, 100)
    assert wiener._settings(16, 0, 1024, 100) == (16, 0)
    for clip in (0, 256):
        with pytest.raises(ValueError):
            wiener._clip(clip)
    assert wiener._clip(None) == 255 and wiener._clip(2) == 2
    for r in ([(3, 10)], [(4, 98)], [(10, 9)]):
        with pytest.raises(ValueError):
            wiener._ranges(r, 5, 3, 100)
    assert wiener._ranges(None, 5, 3, 100) == [(4, 97)] and wiener._ranges([(4, 4), (4, 97)], 5, 3, 100) == [(4, 4), (4, 97)]
