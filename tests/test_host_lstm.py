"""The LSTM decoder without a GPU (include/muahuff_lstm.h, libmuahuff_lstm.so, muahuff.lstm): the ABI's three descriptions
agree and the seven older libraries are as they were, every argument error comes back before a pointer is used -- with
the text tests/lstm_check.cpp prints, which is csrc/mh_lstm_layout.hpp built alone under AddressSanitizer + UBSan --, the
tiles, the loads, the permutation of the gates, the scratch and the capped grids hold over a sweep of shapes, the oracle
(tests/lstm_oracle.py) agrees with float64 torch.nn.LSTM + nn.Linear through from_torch, the weights round-trip, the
folded input weights reproduce explicit z-scoring, and float32 torch.nn.LSTM on the CPU gives the yardstick D_LSTM_F32
that tests/test_gpu_lstm.py holds the device to."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _cascade, _ingest, _kalman, _lib, _lstm, _smooth, _sweep, _wiener, lstm
from tests import lstm_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lstm_check.cpp")
# mh_lstm_layout.hpp: kInTileCols, kInGTile, kInMaxBlocks, kWinTile, kWinWaves, kWinBlockUnits, kWinKGroup, kWinMaxBlocks
IN_TILE, IN_GTILE, IN_MAX_BLOCKS, WIN_TILE, WIN_WAVES, WIN_BLOCK, WIN_KGROUP, WIN_MAX_BLOCKS = 512, 32, 8192, 32, 8, 8, 8, 4096

# The largest difference between lo.predict (NumPy float64 on explicit windows) and float64 torch.nn.LSTM + nn.Linear on the
# CPU over CASES, relative to the largest |out| of the case, as measured by test_the_oracle_agrees_with_float64_torch:
# 2.6e-15 in case 5 (one window, whose |out| is 0.02), 1.0e-15 in case 4, 7.6e-16 and less in the others.  Recorded at
# twice the largest, since a BLAS may sum in another order elsewhere.
D_LSTM_ORACLE = 5.2e-15
# The yardstick of the device: the largest error of FLOAT32 torch.nn.LSTM + nn.Linear on the CPU (explicit float32 windows)
# against lo.predict over CASES, relative to the largest |out| of the case, as measured by
# test_float32_torch_against_the_oracle, case by case: 0: 3.0e-7; 1: 3.0e-7; 2: 1.5e-7; 3: 1.4e-7; 4: 6.4e-7; 5: 9.9e-7;
# 6: 4.6e-7; 7: 4.2e-7; 8: 1.7e-7; 9 (pre-activations past +-100): 3.5e-7.  Recorded at twice the largest.
# tests/test_gpu_lstm.py allows the device 16 times this.
D_LSTM_F32 = 2.0e-6

# (C, T, L, U, K, clip, silent channel, scale of the weights): case 0 is the end-to-end shape; the others are the smallest
# where mhl_windows can go wrong -- lags 1, 2, 5, 15, 32; one window (cols == lags); 31, 32 and 33 windows around the tile of
# 32, three tiles + 5; units 1, 7, 33, 64, 65, 100, 128 (one and two blocks per wave, every k-step group edge); k 1, 2, 8 --
# and case 9 saturates: input weights and bias scaled until pre-activations reach +-100.
CASES = [
    (96, 3000, 15, 100, 2, 3, 5, 1.0),
    (5, 1, 1, 1, 1, 3, None, 1.0),
    (5, 31 + 1, 2, 7, 2, 3, None, 1.0),
    (5, 32 + 4, 5, 33, 8, 3, None, 1.0),
    (5, 33 + 14, 15, 100, 2, 3, None, 1.0),
    (5, 32, 32, 128, 1, 3, None, 1.0),
    (5, 101 + 14, 15, 128, 8, 255, None, 1.0),
    (5, 70 + 4, 5, 64, 2, 3, None, 1.0),
    (5, 40 + 2, 3, 65, 2, 3, None, 1.0),
    (12, 90, 5, 33, 2, 255, None, 60.0),
]


def case_inputs(i):
    """-> x uint8 [C, T], the weights in Keras layout, mean, std (the counts' own where there are enough bins; 0 and 1,
    the clipped counts as they are, in the short cases)"""
    C, T, L, U, K, clip, silent, scale = CASES[i]
    x = lo.counts(C, T, 100 + i, silent)
    w = lo.weights(C, U, K, 200 + i, scale)
    mean, std = lo.moments(x, clip) if T >= 100 else (np.zeros(C), np.ones(C))
    return x, w, mean, std


_ref = {}


def case_reference(i):
    """lo.predict of case i, computed once and shared with tests/test_gpu_lstm.py (never written to)"""
    if i not in _ref:
        x, w, mean, std = case_inputs(i)
        _ref[i] = lo.predict(x, CASES[i][2], CASES[i][5], *w, mean, std)
        _ref[i].setflags(write=False)
    return _ref[i]


def torch_modules(w, dtype):
    kernel, rec, bias, dk, db = w
    m = torch.nn.LSTM(kernel.shape[0], rec.shape[0], batch_first=True).to(dtype)
    d = torch.nn.Linear(rec.shape[0], dk.shape[1]).to(dtype)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.from_numpy(kernel.T)), m.weight_hh_l0.copy_(torch.from_numpy(rec.T))
        m.bias_ih_l0.copy_(torch.from_numpy(bias)), m.bias_hh_l0.zero_()
        d.weight.copy_(torch.from_numpy(dk.T)), d.bias.copy_(torch.from_numpy(db))
    return m, d


def torch_predict(i, dtype):
    """torch.nn.LSTM + nn.Linear of `dtype` on the CPU over the explicit z-scored windows of case i -> float64 numpy [K, n]"""
    x, w, mean, std = case_inputs(i)
    m, d = torch_modules(w, dtype)
    u = torch.from_numpy(lo.input_shaping(lo.zscore(x, CASES[i][5], mean, std), CASES[i][2], 1)).to(dtype)
    with torch.no_grad():
        hs, _ = m(u)
        return d(hs[:, -1]).double().numpy().T, (m, d)


@pytest.fixture(scope="module", autouse=True)
def built():
    b = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    b.build_lstm()
    b.build(), b.build_ingest(), b.build_wiener(), b.build_cascade(), b.build_smooth(), b.build_sweep(), b.build_kalman()   # (no-ops when fresh)


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_lstm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhl_\w+)\s*\(", code))
    assert declared == set(_lstm.PROTOTYPES) == {"mhl_version", "mhl_last_error", "mhl_inproj", "mhl_windows"}
    nm = subprocess.run(["nm", "-D", "--defined-only", _lstm.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared                                  # nothing else is exported
    for fn in ("mhl_inproj", "mhl_windows"):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % fn, code).group(1)
        assert len(args.split(",")) == len(_lstm.PROTOTYPES[fn][1])
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_lstm.hpp", "csrc/mh_lstm_layout.hpp", "csrc/exports_lstm.map"} <= set(build.LSTM_HEADERS)
    assert build.LSTM_SOURCES == ["csrc/mh_lstm.hip"] and build.LSTM_SO == _lstm.SO
    with open(os.path.join(ROOT, "include", "muahuff.h")) as f:
        version = int(re.search(r"#define\s+MH_VERSION\s+(\d+)", f.read()).group(1))
    assert _lstm.lib().mhl_version() == version == 103 == _kalman.lib().mhk_version()
    assert muahuff.lstm is lstm and muahuff._lstm is _lstm
    # the new entry points went into none of the older libraries, which export what their prototypes list
    older = (_lib, _ingest, _wiener, _cascade, _smooth, _sweep, _kalman)
    sos = (build.SO, build.INGEST_SO, build.WIENER_SO, build.CASCADE_SO, build.SMOOTH_SO, build.SWEEP_SO, build.KALMAN_SO)
    for m, so in zip(older, sos):
        assert not any(n.startswith("mhl_") for n in m.PROTOTYPES)
        nm = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
        assert {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[1] in "TDBR"} == set(m.PROTOTYPES), so
    assert (_lstm.IN_TILE_COLS, _lstm.IN_GTILE, _lstm.IN_MAX_BLOCKS, _lstm.WIN_TILE, _lstm.WIN_WAVES, _lstm.WIN_BLOCK_UNITS, _lstm.WIN_KGROUP,
            _lstm.WIN_MAX_BLOCKS) == (IN_TILE, IN_GTILE, IN_MAX_BLOCKS, WIN_TILE, WIN_WAVES, WIN_BLOCK, WIN_KGROUP, WIN_MAX_BLOCKS)
    assert (_lstm.MAX_UNITS, _lstm.MAX_LAGS, _lstm.MAX_K, _lstm.MAX_ROWS) == (128, 32, 8, 65536)


# ---- argument errors ---------------------------------------------------------------------------------------------------
INPROJ = ("x", "x_row_stride", "rows", "cols", "clip", "wx", "bias", "units", "p")
WINDOWS = ("p", "cols", "lags", "units", "wh", "wd", "bd", "k", "out", "out_row_stride")
POINTERS = ("x", "wx", "bias", "p", "wh", "wd", "bd", "out")
T40, T48 = 1 << 40, 1 << 48


def _args(order, **over):
    """the arguments of mhl_inproj / mhl_windows with host stand-ins for the device buffers (kept alive in the first item);
    a pointer given as the name of another one starts where that one does (before any shift)"""
    keep = {k: np.zeros(1 << 14, np.uint64) for k in POINTERS if k in order}
    a = dict(x_row_stride=128, rows=3, cols=100, clip=39, units=4, lags=5, k=2, out_row_stride=384)
    a = {k: v for k, v in a.items() if k in order}
    for k, v in keep.items():
        a[k] = v.ctypes.data + (-v.ctypes.data) % 16
    alias = {k: over.pop(k) for k in list(over) if isinstance(over[k], str)}
    shift = {k[:-6]: over.pop(k) for k in list(over) if k.endswith("_shift")}
    for k, v in over.items():
        a[k] = 0 if v is None else v
    for k, other in alias.items():
        a[k] = a[other]
    for k, s in shift.items():
        a[k] += s
    return keep, a


def _call(order, a):
    L = _lstm.lib()
    vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in order]
    rc = (L.mhl_inproj if order is INPROJ else L.mhl_windows)(*vals, None)
    return rc, L.mhl_last_error().decode()


def _line(order, a):
    return ("inproj " if order is INPROJ else "windows ") + " ".join(str(a[k]) for k in order) + "\n"


# p of the defaults: 100 bins x 16 pre-activations x 4 bytes = 6400; out: 2 rows of 96 floats, 384 bytes apart
INPROJ_BAD = [dict(x=None), dict(wx=None), dict(bias=None), dict(p=None), dict(units=0), dict(units=129), dict(rows=0), dict(rows=65537),
              dict(cols=0), dict(cols=T40, x_row_stride=T40), dict(clip=0), dict(clip=256), dict(wx_shift=2), dict(bias_shift=1), dict(p_shift=2),
              dict(x_row_stride=99), dict(x_row_stride=0), dict(x_row_stride=T48), dict(p="x"), dict(p="wx"), dict(p="bias"),
              dict(p="x", p_shift=296), dict(wx="p", wx_shift=6396), dict(bias="p", bias_shift=6396)]
INPROJ_GOOD = [dict(), dict(x_shift=1), dict(x_shift=3, x_row_stride=100), dict(rows=1, x_row_stride=0), dict(units=1), dict(units=128, p=1 << 60),
               dict(clip=1), dict(clip=255), dict(rows=65536, wx=1 << 50, x=1 << 55), dict(p_shift=4), dict(p="x", p_shift=360),
               dict(cols=T40 - 1, x_row_stride=T40, p=1 << 60), dict(x_row_stride=T48 - 1, p=1 << 60), dict(wx="p", wx_shift=6400), dict(bias="p", bias_shift=6400)]
WINDOWS_BAD = [dict(p=None), dict(wh=None), dict(wd=None), dict(bd=None), dict(out=None), dict(units=0), dict(units=129), dict(lags=0),
               dict(lags=33), dict(k=0), dict(k=9), dict(cols=4), dict(cols=0), dict(cols=T40, out_row_stride=4 * T40), dict(p_shift=2),
               dict(wh_shift=1), dict(wd_shift=2), dict(bd_shift=3), dict(out_shift=2), dict(out_row_stride=386), dict(out_row_stride=380),
               dict(out_row_stride=0), dict(out_row_stride=T48), dict(out="p"), dict(out="wh"), dict(out="wd"), dict(out="bd"),
               dict(out="p", out_shift=6396), dict(wh="out", wh_shift=764), dict(bd="out", bd_shift=384)]
WINDOWS_GOOD = [dict(), dict(k=1, out_row_stride=0), dict(k=8, out=1 << 60), dict(lags=1, out_row_stride=400), dict(lags=32, cols=32),
                dict(units=1), dict(units=128, p=1 << 60, wh=1 << 58), dict(cols=5), dict(out_row_stride=T48 - 4, out=1 << 60),
                dict(cols=T40 - 1, out_row_stride=4 * T40, out=1 << 60, p=1 << 61), dict(out="p", out_shift=6400), dict(wh="out", wh_shift=768),
                dict(out_row_stride=388)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items()) or "default"   # noqa: E731


@pytest.mark.parametrize("bad", INPROJ_BAD, ids=_ids)
def test_inproj_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(INPROJ, **dict(bad))
    rc, msg = _call(INPROJ, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhl_inproj:"), (rc, msg)


@pytest.mark.parametrize("bad", WINDOWS_BAD, ids=_ids)
def test_windows_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(WINDOWS, **dict(bad))
    rc, msg = _call(WINDOWS, a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mhl_windows:"), (rc, msg)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lstm") / "lstm_check_asan")
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
    for order, bad, good, rules in ((INPROJ, INPROJ_BAD, INPROJ_GOOD, 8), (WINDOWS, WINDOWS_BAD, WINDOWS_GOOD, 8)):
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


def layout(cols, lags, units):
    """mh_lstm_layout.hpp's rules, restated -> [in tiles, g-tiles, in grid, win tiles, blocks, per wave, k-steps, win grid, p bytes]"""
    it, gt = -(-cols // IN_TILE), -(-4 * units // IN_GTILE)
    wt = -(-(cols - lags + 1) // WIN_TILE)
    blocks = -(-units // WIN_BLOCK)
    ks = -(-((units + 1) // 2) // WIN_KGROUP) * WIN_KGROUP
    return [it, gt, min(it * gt, IN_MAX_BLOCKS), wt, blocks, 2 if blocks > WIN_WAVES else 1, ks, min(wt, WIN_MAX_BLOCKS), cols * 16 * units]


def test_tiles_loads_permutation_scratch_and_grids_over_the_sweep(exe):
    """lstm_check asserts per shape what its header comment lists"""
    grid = []
    for cols in (32, 33, 63, 64, 65, IN_TILE - 1, IN_TILE, IN_TILE + 1, 3 * IN_TILE + 5, 3000, 72000, 10 ** 7):
        for lags in (1, 2, 5, 15, 32):
            for units in (1, 7, 33, 64, 65, 100, 128):
                grid.append((cols, lags, units))
    grid += [(L, L, U) for L in (1, 2, 15, 32) for U in (1, 100)]                 # one window
    grid += [(1, 1, 1), (2, 1, 3), (3, 2, 128), (5, 5, 16)]
    grid += [(T, L, U) for _C, T, L, U, _K, _q, _s, _w in CASES]
    grid += [(T40 - 1, 1, 128), (T40 - 1, 32, 1)]
    text = "".join("layout %d %d %d\n" % g for g in grid)
    lines = _run(exe, text)
    assert len(lines) == len(grid)
    strided_in = strided_win = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == layout(*g), (g, got)
        assert got[8] == _lstm.inproj_bytes(g[0], g[2])
        strided_in += got[0] * got[1] > got[2]
        strided_win += got[3] > got[7]
    assert strided_in > 20 and strided_win > 20
    assert layout(10 ** 7, 15, 100) == [19532, 13, 8192, 312500, 13, 2, 56, 4096, 16 * 10 ** 9]
    assert [layout(100, 1, u)[5:7] for u in (1, 16, 17, 64, 65, 112, 113, 128)] == [[1, 8], [1, 8], [1, 16], [1, 32], [2, 40], [2, 56], [2, 64], [2, 64]]


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_the_oracle_agrees_with_float64_torch(i):
    C, T, L, U, K, clip, _silent, _scale = CASES[i]
    ref = case_reference(i)
    got, (m, d) = torch_predict(i, torch.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("case %d: the oracle and float64 torch differ by %.2e of the largest |out| %.3g" % (i, err, np.abs(ref).max()))
    assert ref.shape == (K, T - L + 1) and np.isfinite(ref).all() and err <= D_LSTM_ORACLE
    # and the same again with the weights read back through from_torch
    x, w, mean, std = case_inputs(i)
    dec = lstm.LSTMDecoder(U, L, 0, clip).from_torch(m, d, mean, std)
    again = lo.predict(x, L, clip, *dec.get_weights())
    assert np.array_equal(again, ref)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_float32_torch_against_the_oracle(i):
    ref = case_reference(i)
    got, _ = torch_predict(i, torch.float32)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("case %d: float32 torch differs from the oracle by %.2e of the largest |out| %.3g" % (i, err, np.abs(ref).max()))
    assert err <= D_LSTM_F32


def test_the_saturating_case_saturates():
    x, w, mean, std = case_inputs(9)
    z = lo.zscore(x, CASES[9][5], mean, std) @ w[0] + w[2]
    assert np.abs(z).max() >= 100 and np.isfinite(case_reference(9)).all()


def test_weights_round_trip():
    C, U, K, L = 7, 5, 3, 4
    w = lo.weights(C, U, K, 3)
    mean, std = np.linspace(0.5, 2, C), np.linspace(1, 3, C)
    std[2] = 0.0
    d = lstm.LSTMDecoder(U, L, 1, 4).set_weights(*w, mean, std)
    back = d.get_weights()
    assert all(np.array_equal(a, b) for a, b in zip(back, (*w, mean, std))) and (d.channels, d.outputs) == (C, K)
    assert d.num_params() == 4 * U * (C + U + 1) + K * (U + 1)
    e = lstm.LSTMDecoder(U, L).set_weights(*back)
    assert all(np.array_equal(a, b) for a, b in zip(e.get_weights(), back))
    # through torch: b_ih + b_hh are summed, the gate order stays
    m, lin = torch_modules(w, torch.float64)
    with torch.no_grad():
        m.bias_hh_l0.copy_(torch.arange(4 * U, dtype=torch.float64))
    t = lstm.LSTMDecoder(U, L).from_torch(m, lin, mean, std).get_weights()
    assert np.array_equal(t[0], w[0]) and np.array_equal(t[1], w[1]) and np.array_equal(t[2], w[2] + np.arange(4 * U))
    assert np.array_equal(t[3], w[3]) and np.array_equal(t[4], w[4]) and np.array_equal(t[5], mean) and np.array_equal(t[6], std)
    # defaults: the clipped counts as they are
    assert np.array_equal(lstm.LSTMDecoder(U, L).set_weights(*w).get_weights()[6], np.ones(C))
    for bad in (dict(kernel=w[0][:, :-1]), dict(recurrent_kernel=w[1][:-1]), dict(bias=w[2][:-1]), dict(dense_bias=np.zeros(K + 1)),
                dict(mean=np.zeros(C + 1)), dict(std=-np.ones(C)), dict(kernel=np.full_like(w[0], np.nan))):
        kw = dict(kernel=w[0], recurrent_kernel=w[1], bias=w[2], dense_kernel=w[3], dense_bias=w[4], mean=mean, std=std)
        kw.update(bad)
        with pytest.raises(ValueError):
            lstm.LSTMDecoder(U, L).set_weights(**kw)
    with pytest.raises(ValueError):
        lstm.LSTMDecoder(U + 1, L).from_torch(m, lin)
    with pytest.raises(ValueError):
        lstm.LSTMDecoder(U, L).from_torch(torch.nn.LSTM(C, U, num_layers=2), lin)
    with pytest.raises(ValueError):
        lstm.LSTMDecoder(U, L).get_weights()


def test_the_folded_weights_reproduce_explicit_z_scoring():
    C, T, L, U, K, clip, silent, _scale = CASES[0]
    x, w, mean, std = case_inputs(0)
    assert std[silent] == 0 and (np.delete(std, silent) > 0).all()
    wx, b, wh, wd, bd = lstm.LSTMDecoder(U, L, 0, clip).set_weights(*w, mean, std).folded()
    assert (wx.dtype, wx.shape, b.shape, wh.shape, wd.shape, bd.shape) == (np.float32, (4 * U, C), (4 * U,), (4 * U, U), (K, U), (K,))
    assert (wx[:, silent] == 0).all() and np.array_equal(wh, w[1].T.astype(np.float32)) and np.array_equal(wd, w[3].T.astype(np.float32))
    q = np.minimum(x, clip).astype(np.float64)
    p = q.T @ wx.astype(np.float64).T + b.astype(np.float64)       # what mhl_inproj computes, in float64
    z = lo.zscore(x, clip, mean, std) @ w[0] + w[2]                # explicit z-scoring
    # float32 weights: 2^-24 per weight against sum |w x|, far inside the bound of the device
    assert np.abs(p - z).max() <= 2.0 ** -23 * (np.abs(wx).astype(np.float64) @ q).max()
    # and through the recurrence the folded route is the model
    got = lo.recurrence(p, L, w[1], w[3], w[4])
    assert np.abs(got - case_reference(0)).max() <= D_LSTM_F32 * np.abs(case_reference(0)).max()


def test_what_is_not_built_is_refused():
    for bad in (dict(num_layers=2), dict(stateful=True), dict(dropout=0.1), dict(window=3), dict(units=0), dict(units=129), dict(lags=0),
                dict(lags=33), dict(lead=-1), dict(clip=0), dict(clip=256)):
        with pytest.raises(ValueError):
            lstm.LSTMDecoder(**bad)
    d = lstm.LSTMDecoder(units=100, lags=15, lead=2, clip=None)
    assert (d.units, d.lags, d.lead, d.clip) == (100, 15, 2, 255)


def test_host_matrices_are_refused(monkeypatch):
    monkeypatch.setattr(_lstm, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_wiener, "lib", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(_ingest, "lib", lambda: pytest.fail("the library was loaded"))
    x, w, mean, std = case_inputs(2)
    C, T, L, U, K, clip, _s, _w = CASES[2]
    d = lstm.LSTMDecoder(U, L, 0, clip).set_weights(*w, mean, std)
    y = torch.zeros((K, T))
    for bad in (x, torch.from_numpy(x)):
        with pytest.raises(ValueError, match="no CPU path"):
            d.predict(bad)
        with pytest.raises(ValueError, match="no CPU path"):
            d.score(bad, y)
        with pytest.raises(ValueError, match="no CPU path"):
            d.fit(bad, y)
        with pytest.raises(ValueError, match="no CPU path"):
            lstm.cross_validate(bad, y, L)
    with pytest.raises(ValueError, match="BinSource"):
        d.predict_from(torch.from_numpy(x))
    with pytest.raises(ValueError, match="comes after"):
        lstm.LSTMDecoder(U, L).folded()
