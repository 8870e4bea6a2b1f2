"""The minibatch loss and gradient of the LSTM decoder without a GPU (include/muahuff_train.h, libmuahuff_train.so,
muahuff.lstm.loss_and_grad): the ABI's three descriptions agree and the eight older libraries are as they were, every argument
error comes back before a pointer is used -- with the text tests/train_check.cpp prints, which is csrc/mh_train_layout.hpp
built alone under AddressSanitizer + UBSan --, the scratch, the clamp, the tiles and the capped grids hold over a sweep of
shapes, the oracle (tests/lstm_grad_oracle.py: NumPy float64, hand-written backward pass) agrees with float64 torch autograd,
and float32 torch autograd on the CPU gives the yardstick D_GRAD_F32 that tests/test_gpu_train.py holds the device to."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _cascade, _ingest, _kalman, _lib, _lstm, _smooth, _sweep, _train, _wiener, lstm, train
from tests import lstm_grad_oracle as go
from tests import lstm_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "train_check.cpp")
# mh_train_layout.hpp: kTrainMaxBatch, kTrainInRows, kTrainInMaxBlocks, kTrainMaxTiles, kBwdKSteps, kGradTile, kGradThreads,
# kGradMaxBlocks, kTrainDoutPitch
MAX_BATCH, IN_ROWS, IN_MAX_BLOCKS, MAX_TILES, BWD_KSTEPS, GRAD_TILE, GRAD_THREADS, GRAD_MAX_BLOCKS, DOUT_PITCH = 65536, 128, 4096, 1024, 32, 32, 64, 1024, 8
GRADS = ("wx", "bias", "wh", "wd", "bd")

# The largest difference between go.loss_grad (NumPy float64, hand-written backward pass through time) and float64 torch
# autograd on the CPU over CASES, per tensor (out, loss and the five gradients) relative to that tensor's largest |entry|, as
# measured by test_the_oracle_agrees_with_float64_autograd: 4.8e-15 (bias of case 9, the saturating one), 1.2e-15 (cases 0
# and 4) and 1.0e-15 or less in the others.  Recorded at twice the largest, since a BLAS may sum in another order elsewhere.
D_GRAD_ORACLE = 9.6e-15
# The yardstick of the device: the largest error of FLOAT32 torch autograd on the CPU (explicit float32 windows, nn.LSTM +
# nn.Linear, the reference's rmse) against go.loss_grad over CASES, per gradient tensor relative to that tensor's largest
# |entry|, as measured by test_float32_autograd_against_the_oracle, case by case (the largest of wx, bias, wh, wd, bd):
# 0: 2.8e-7 (bias); 1: 1.9e-7 (bias); 2: 5.8e-7 (bias); 3: 8.7e-7 (bias); 4: 4.4e-7 (wx); 5: 4.7e-7 (bias); 6: 3.1e-7 (wx);
# 7: 5.0e-7 (wh); 8: 9.6e-7 (bias); 9 (saturating): 2.0e-6 (wh).  Recorded at twice the largest.  out and loss of the same
# runs stay inside test_host_lstm.D_LSTM_F32 (4.2e-7 at most).  tests/test_gpu_train.py allows the device 16 times these.
D_GRAD_F32 = 4.0e-6

# (C, T, L, U, K, clip, batch, lead, silent channel, scale of the input weights): the smallest shapes where the kernels can go
# wrong -- lags 1 (no recurrent product: dwh is exactly 0), 2, 3, 5, 15, 32; batch 1, 31, 32, 33 (a tail tile of one window),
# 40, 70, 5, 16; units 1, 7, 8, 33, 64, 65, 100, 128; k 1, 2, 8; an odd channel count; 130 channels (more than four channel
# tiles, with a remainder); case 8 is the study's own minibatch with a silent channel; case 9 saturates the gates.
CASES = [
    (5, 40, 1, 1, 1, 3, 1, 0, None, 1.0),
    (5, 60, 2, 7, 2, 3, 31, 1, None, 1.0),
    (5, 80, 5, 33, 8, 3, 32, 0, None, 1.0),
    (3, 120, 15, 100, 2, 3, 33, 2, None, 1.0),
    (5, 64, 32, 128, 1, 255, 5, 0, None, 1.0),
    (12, 200, 5, 64, 2, 3, 70, 0, None, 1.0),
    (12, 200, 3, 65, 2, 3, 40, 0, None, 1.0),
    (130, 300, 3, 8, 2, 255, 40, 0, None, 1.0),
    (96, 3000, 15, 100, 2, 3, 32, 0, 5, 1.0),
    (12, 90, 5, 33, 2, 255, 16, 0, None, 60.0),
]


def windows_index(T, L, lead, batch, seed):
    """int64 [batch]: unsorted, with a duplicate, the first design row (L-1) and the last (T-1-lead) among them (a single
    window is the last row)"""
    rng = np.random.RandomState(seed)
    idx = rng.randint(L - 1, T - lead, size=batch).astype(np.int64)
    idx[0] = T - 1 - lead
    if batch >= 2:
        idx[-1] = L - 1
    if batch >= 4:
        idx[1] = idx[2] = (L - 1 + T - 1 - lead) // 2 + 1
    return idx


def case_inputs(i):
    """-> dict(x uint8 [C, T], y float32 [K, T], idx int64 [B], w: the weights in Keras layout, mean, inv, std float64 [C]).
    mean and inv are exactly representable in float32, so that the device and the oracle start from the same numbers; the
    silent channel has std = inv = 0."""
    C, T, L, U, K, clip, batch, lead, silent, scale = CASES[i]
    x = lo.counts(C, T, 300 + i, silent)
    w = lo.weights(C, U, K, 400 + i, scale)
    mean, std = lo.moments(x, clip)
    keep = std > 0
    mean = mean.astype(np.float32).astype(np.float64)
    inv = np.where(keep, 1.0 / np.where(keep, std, 1.0), 0.0).astype(np.float32).astype(np.float64)
    std = np.where(keep, 1.0 / np.where(keep, inv, 1.0), 0.0)
    y = lo.target(x, L, lead, K, 500 + i)
    return dict(x=x, y=y, idx=windows_index(T, L, lead, batch, 600 + i), w=w, mean=mean, inv=inv, std=std)


def case_windows(i, inp=None):
    """-> the explicit windows u float64 [B, L, C] and their targets float64 [B, K]"""
    C, T, L, U, K, clip, batch, lead, silent, scale = CASES[i]
    inp = case_inputs(i) if inp is None else inp
    u = go.gather(go.zscored(inp["x"], clip, inp["mean"], inp["inv"]), inp["idx"], L)
    return u, inp["y"].astype(np.float64)[:, inp["idx"] + lead].T


_ref = {}


def case_reference(i):
    """go.loss_grad of case i at scale 1 / batch, computed once and shared with tests/test_gpu_train.py (never written to)"""
    if i not in _ref:
        inp = case_inputs(i)
        u, tgt = case_windows(i, inp)
        _ref[i] = go.loss_grad(u, tgt, *inp["w"], 1.0 / CASES[i][6])
        for a in _ref[i].values():
            a.setflags(write=False)
    return _ref[i]


def torch_modules(w, dtype):
    kernel, rec, bias, dk, db = w
    m = torch.nn.LSTM(kernel.shape[0], rec.shape[0], batch_first=True).to(dtype)
    d = torch.nn.Linear(rec.shape[0], dk.shape[1]).to(dtype)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.from_numpy(kernel.T)), m.weight_hh_l0.copy_(torch.from_numpy(rec.T))
        m.bias_ih_l0.copy_(torch.from_numpy(bias)), m.bias_hh_l0.zero_()
        d.weight.copy_(torch.from_numpy(dk.T)), d.bias.copy_(torch.from_numpy(db))
    m.bias_hh_l0.requires_grad_(False)
    return m, d


def autograd(i, dtype):
    """torch autograd of `dtype` on the CPU over the explicit windows of case i, the loss as LSTMDecoder.fit forms it ->
    dict(out [K, B], loss [B], wx, bias, wh, wd, bd), float64 numpy"""
    inp = case_inputs(i)
    u, tgt = case_windows(i, inp)
    m, d = torch_modules(inp["w"], dtype)
    hs, _ = m(torch.from_numpy(u).to(dtype))
    out = d(hs[:, -1])
    loss = torch.sqrt(((out - torch.from_numpy(tgt).to(dtype)) ** 2).mean(1))
    (loss.sum() / CASES[i][6]).backward()
    f = lambda t: t.detach().double().numpy()  # noqa: E731
    return dict(out=f(out).T, loss=f(loss), wx=f(m.weight_ih_l0.grad), bias=f(m.bias_ih_l0.grad), wh=f(m.weight_hh_l0.grad),
                wd=f(d.weight.grad), bd=f(d.bias.grad))


def rel(got, ref):
    """the largest difference relative to the reference's largest |entry| (0 where the reference is all zero and so is got)"""
    top = np.abs(ref).max()
    return np.abs(got - ref).max() / top if top > 0 else np.abs(got).max()


@pytest.fixture(scope="module", autouse=True)
def built():
    b = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    b.build_train()
    b.build(), b.build_ingest(), b.build_wiener(), b.build_cascade(), b.build_smooth(), b.build_sweep(), b.build_kalman(), b.build_lstm()


def _exports(so):
    nm = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[1] in "TDBR"}


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_train.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mht_\w+)\s*\(", code))
    assert declared == set(_train.PROTOTYPES) == {"mht_version", "mht_last_error", "mht_loss_grad"}
    assert _exports(_train.SO) == declared                       # nothing else is exported
    args = re.search(r"\bmht_loss_grad\s*\(([^)]*)\)", code).group(1)
    assert len(args.split(",")) == len(_train.PROTOTYPES["mht_loss_grad"][1]) == 30
    assert "mht_*" in open(os.path.join(CSRC, "exports_train.map")).read()
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert set(build.TRAIN_HEADERS) == {"csrc/exports_train.map", "csrc/mh_abi.hpp", "csrc/mh_train.hpp", "csrc/mh_train_layout.hpp",
                                        "csrc/mh_msg.hpp", "../include/muahuff.h", "csrc/mh_lstm.hpp", "csrc/mh_lstm_layout.hpp",
                                        "csrc/mh_rows.hpp", "../include/muahuff_train.h"}
    assert build.TRAIN_HEADERS == build.headers("muahuff_train") and build.TRAIN_HEADERS[0] == "csrc/exports_train.map"
    assert build.TRAIN_SOURCES == ["csrc/mh_train.hip"] and build.TRAIN_SO == _train.SO == build.so_path("muahuff_train")
    assert build.TRAINING == [("muahuff_train", "csrc/mh_train.hip", "csrc/exports_train.map", "../include/muahuff_train.h")]
    with open(os.path.join(ROOT, "include", "muahuff.h")) as f:
        version = int(re.search(r"#define\s+MH_VERSION\s+(\d+)", f.read()).group(1))
    assert _train.lib().mht_version() == version == 103 == _lstm.lib().mhl_version()
    assert muahuff.train is train and muahuff._train is _train and train.loss_and_grad is lstm.loss_and_grad
    # the new entry points went into none of the older libraries, which export what their prototypes list, and the table of
    # those libraries is as it was
    assert [r[0] for r in build.LIBRARIES] == ["muahuff"] + ["muahuff_" + n for n in ("ingest", "wiener", "cascade", "smooth", "sweep", "kalman", "lstm")]
    older = (_lib, _ingest, _wiener, _cascade, _smooth, _sweep, _kalman, _lstm)
    sos = (build.SO, build.INGEST_SO, build.WIENER_SO, build.CASCADE_SO, build.SMOOTH_SO, build.SWEEP_SO, build.KALMAN_SO, build.LSTM_SO)
    for m, so in zip(older, sos):
        assert not any(n.startswith("mht_") for n in m.PROTOTYPES)
        assert _exports(so) == set(m.PROTOTYPES), so
    assert (_train.MAX_BATCH, _train.IN_ROWS, _train.IN_MAX_BLOCKS, _train.MAX_TILES, _train.BWD_KSTEPS, _train.GRAD_TILE, _train.GRAD_THREADS,
            _train.GRAD_MAX_BLOCKS, _train.DOUT_PITCH) == (MAX_BATCH, IN_ROWS, IN_MAX_BLOCKS, MAX_TILES, BWD_KSTEPS, GRAD_TILE, GRAD_THREADS,
                                                          GRAD_MAX_BLOCKS, DOUT_PITCH)
    assert train.MAX_BATCH == MAX_BATCH


# ---- argument errors ---------------------------------------------------------------------------------------------------
ORDER = ("x", "x_row_stride", "rows", "cols", "clip", "mean", "inv", "idx", "batch", "lags", "units", "k", "lead", "wx", "bias", "wh", "wd", "bd",
         "y", "y_row_stride", "scale", "scratch", "out", "loss", "dwx", "dbias", "dwh", "dwd", "dbd")
POINTERS = ("x", "mean", "inv", "idx", "wx", "bias", "wh", "wd", "bd", "y", "scratch", "out", "loss", "dwx", "dbias", "dwh", "dwd", "dbd")
T40, T48 = 1 << 40, 1 << 48


def _args(**over):
    """the arguments of mht_loss_grad with host stand-ins for the device buffers (kept alive in the first item); a pointer
    given as the name of another one starts where that one does (before any shift)"""
    keep = {k: np.zeros(1 << 13, np.uint64) for k in POINTERS}
    a = dict(x_row_stride=128, rows=3, cols=100, clip=39, batch=6, lags=5, units=4, k=2, lead=1, y_row_stride=400, scale=0.25)
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


def _call(a):
    L = _train.lib()
    vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in ORDER]
    rc = L.mht_loss_grad(*vals, None)
    return rc, L.mht_last_error().decode()


def _line(a):
    return "loss_grad " + " ".join(repr(float(a[k])) if k == "scale" else str(a[k]) for k in ORDER) + "\n"


# the defaults: 6 windows x 5 lags = 30 rows, 16 pre-activations: the scratch holds 4 * (30 * 40 + 48) = 4992 bytes; out 48 bytes,
# loss 24, dwx 192, dbias 64, dwh 256, dwd 32, dbd 8; x 3 rows of 100 bytes 128 apart; y 2 rows of 400 bytes; idx 48 bytes
BAD = [dict([(p, None)]) for p in POINTERS] + [
    dict(units=0), dict(units=129), dict(lags=0), dict(lags=33), dict(k=0), dict(k=9), dict(rows=0), dict(rows=65537), dict(batch=0),
    dict(batch=65537), dict(clip=0), dict(clip=256), dict(cols=0), dict(cols=T40, x_row_stride=T40, y_row_stride=4 * T40), dict(cols=5),
    dict(cols=4, lead=0), dict(lead=96), dict(lead=100), dict(lead=1 << 63), dict(scale=float("nan")), dict(scale=float("inf")),
    dict(scale=float("-inf")), dict(mean_shift=2), dict(inv_shift=1), dict(wx_shift=2), dict(bias_shift=3), dict(wh_shift=2), dict(wd_shift=1),
    dict(bd_shift=2), dict(y_shift=2), dict(y_row_stride=402), dict(scratch_shift=2), dict(out_shift=1), dict(loss_shift=2), dict(dwx_shift=2),
    dict(dbias_shift=2), dict(dwh_shift=2), dict(dwd_shift=2), dict(dbd_shift=2), dict(idx_shift=4), dict(x_row_stride=99), dict(x_row_stride=0),
    dict(x_row_stride=T48), dict(y_row_stride=396), dict(y_row_stride=0), dict(y_row_stride=T48), dict(scratch="x"), dict(scratch="wx"),
    dict(scratch="idx"), dict(scratch="y", scratch_shift=796), dict(out="bd"), dict(loss="mean"), dict(dwx="wx"), dict(dbias="bias"), dict(dwh="wh"),
    dict(dwd="wd"), dict(dbd="bd", dbd_shift=4), dict(dbd="inv", dbd_shift=8), dict(x="scratch", x_shift=4988), dict(out="scratch"),
    dict(loss="out", loss_shift=44), dict(dwx="scratch", dwx_shift=4988), dict(dbias="dwx", dbias_shift=188), dict(dwh="dbias"), dict(dwd="dwh", dwd_shift=252),
    dict(dbd="dwd", dbd_shift=28)]
GOOD = [dict(), dict(x_shift=1), dict(x_shift=3, x_row_stride=100), dict(rows=1, x_row_stride=0), dict(k=1, y_row_stride=0), dict(units=1),
        dict(units=128, lags=32, batch=65536, rows=65536, k=8, x=1 << 40, wx=1 << 50, wh=1 << 51, scratch=1 << 52, out=1 << 53, loss=1 << 54,
             dwx=1 << 55, dwh=1 << 56, mean=1 << 57, inv=1 << 58, idx=1 << 59, wd=1 << 60, dwd=1 << 61, y=3 << 60), dict(clip=1), dict(clip=255),
        dict(cols=6), dict(cols=5, lead=0), dict(lead=95), dict(lead=0), dict(scale=0.0), dict(scale=-1.0),
        dict(cols=T40 - 1, x_row_stride=T40, y_row_stride=4 * T40, x=1 << 50, y=1 << 60), dict(x_row_stride=T48 - 1, x=1 << 60),
        dict(y_row_stride=T48 - 4, y=1 << 60), dict(out="scratch", out_shift=4992), dict(x="scratch", x_shift=4992), dict(loss="out", loss_shift=48),
        dict(dbias="dwx", dbias_shift=192), dict(dbd="dwd", dbd_shift=32), dict(dbd="bd", dbd_shift=8), dict(idx_shift=8)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items()) or "default"   # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=_ids)
def test_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(**dict(bad))
    rc, msg = _call(a)
    del keep
    assert rc == _lib.ERR_ARG and msg.startswith("mht_loss_grad:"), (rc, msg)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("train") / "train_check_asan")
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
    cases = [_args(**dict(b)) for b in BAD]
    lines = _run(exe, "".join(_line(a) for _k, a in cases))
    assert len(lines) == len(BAD)
    seen = set()
    for (keep, a), ln, b in zip(cases, lines, BAD):
        rc, msg = _call(a)
        assert ln == "error %d %s" % (rc, msg) and rc == _lib.ERR_ARG, (b, ln, msg)
        seen.add(re.sub(r"\d+", "#", msg))
    assert len(seen) == 16, seen                                   # the table reaches every rule
    ok = [_args(**dict(g)) for g in GOOD]
    # (accepted arguments would be launched: they are checked through the program alone)
    assert _run(exe, "".join(_line(a) for _k, a in ok)) == ["ok"] * len(GOOD)


def layout(rows, batch, lags, units, k):
    """mh_train_layout.hpp's rules, restated -> [R, g-tiles, in items, in grid, tiles, recurrence grid, forward k-steps, unit
    blocks, channel tiles, dwx items, dwh items, sum items, items, gradient grid, scratch bytes]"""
    R, gt = batch * lags, -(-4 * units // GRAD_TILE)
    ini = -(-R // IN_ROWS) * gt
    tiles, ub, ct = -(-batch // 32), -(-units // 32), -(-rows // GRAD_TILE)
    ks = -(-((units + 1) // 2) // 8) * 8
    sums = -(-(4 * units + k * units + k) // GRAD_THREADS)
    items = gt * ct + gt * ub + sums
    return [R, gt, ini, min(ini, IN_MAX_BLOCKS), tiles, min(tiles, MAX_TILES), ks, ub, ct, gt * ct, gt * ub, sums, items,
            min(items, GRAD_MAX_BLOCKS), 4 * (R * 10 * units + DOUT_PITCH * batch)]


def test_scratch_clamp_tiles_and_grids_over_the_sweep(exe):
    """train_check asserts per shape what its header comment lists"""
    grid = []
    for batch in (1, 31, 32, 33, 70, 32 * MAX_TILES + 1):
        for lags in (1, 2, 5, 15, 32):
            for units in (1, 7, 33, 64, 65, 100, 128):
                grid.append((5 if units % 2 else 96, batch, lags, units, 1 + units % 8))
    grid += [(C, B, L, U, K) for C, _T, L, U, K, _q, B, _g, _s, _w in CASES]
    grid += [(32 * GRAD_MAX_BLOCKS + 5, 3, 2, 1, 1), (65536, 1, 1, 128, 8), (1, 65536, 2, 1, 1), (2, 32 * MAX_TILES + 1, 2, 1, 1), (1024, 32, 15, 100, 2)]
    lines = _run(exe, "".join("layout %d %d %d %d %d\n" % g for g in grid))
    assert len(lines) == len(grid)
    strided_rec = strided_grad = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == layout(*g), (g, got)
        assert got[14] == _train.scratch_bytes(g[1], g[2], g[3]) == 4 * _train.scratch_layout(g[1], g[2], g[3])["floats"]
        strided_rec += got[4] > got[5]
        strided_grad += got[12] > got[13]
    assert strided_rec >= 10 and strided_grad >= 2
    assert layout(96, 32, 15, 100, 2) == [480, 13, 52, 52, 1, 1, 56, 4, 3, 39, 52, 10, 101, 101, 1921024]
    s = _train.scratch_layout(32, 15, 100)
    assert (s["act"], s["dz"], s["c"], s["h"], s["dout"], s["floats"]) == (0, 192000, 384000, 432000, 480000, 480256)


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_the_cases_are_what_they_claim(i):
    C, T, L, U, K, clip, batch, lead, silent, scale = CASES[i]
    inp = case_inputs(i)
    idx = inp["idx"]
    assert idx.shape == (batch,) and idx.min() >= L - 1 and idx.max() <= T - 1 - lead and (T - 1 - lead) in idx
    if batch >= 2:
        assert (L - 1) in idx and (np.diff(idx) < 0).any()
    if batch >= 4:
        assert len(set(idx.tolist())) < batch
    assert np.array_equal(inp["mean"].astype(np.float32).astype(np.float64), inp["mean"])
    assert np.array_equal(inp["inv"].astype(np.float32).astype(np.float64), inp["inv"])
    if silent is not None:
        assert inp["inv"][silent] == 0 and inp["std"][silent] == 0 and (case_reference(i)["wx"][:, silent] == 0).all()
    # 1 / std in float64, rounded to float32, is inv again: lstm.loss_and_grad starts from the oracle's numbers
    keep = inp["std"] > 0
    assert np.array_equal((1.0 / inp["std"][keep]).astype(np.float32).astype(np.float64), inp["inv"][keep])
    ref = case_reference(i)
    assert all(np.isfinite(ref[n]).all() for n in ref) and (ref["loss"] > 0).all()
    if L == 1:
        assert (ref["wh"] == 0).all()
    if scale > 1:
        u, _ = case_windows(i, inp)
        assert np.abs(u @ inp["w"][0] + inp["w"][2]).max() >= 100


@pytest.mark.parametrize("i", range(len(CASES)))
def test_the_oracle_agrees_with_float64_autograd(i):
    ref, got = case_reference(i), autograd(i, torch.float64)
    for n in ("out", "loss") + GRADS:
        err = rel(got[n], ref[n])
        print("case %d %s: the oracle and float64 autograd differ by %.2e of the largest |entry| %.3g" % (i, n, err, np.abs(ref[n]).max()))
        assert got[n].shape == ref[n].shape and err <= D_GRAD_ORACLE, (n, err)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_float32_autograd_against_the_oracle(i):
    from tests.test_host_lstm import D_LSTM_F32
    ref, got = case_reference(i), autograd(i, torch.float32)
    for n in ("out", "loss") + GRADS:
        err = rel(got[n], ref[n])
        print("case %d %s: float32 autograd differs from the oracle by %.2e of the largest |entry| %.3g" % (i, n, err, np.abs(ref[n]).max()))
        assert err <= (D_LSTM_F32 if n in ("out", "loss") else D_GRAD_F32), (n, err)


def test_a_window_of_zero_loss_adds_nothing():
    inp = case_inputs(1)
    u, tgt = case_windows(1, inp)
    full = go.loss_grad(u, tgt, *inp["w"], 0.5)
    tgt2 = tgt.copy()
    tgt2[3] = full["out"][:, 3]                                    # window 3 hits its target exactly
    hit = go.loss_grad(u, tgt2, *inp["w"], 0.5)
    rest = np.delete(np.arange(len(u)), 3)
    alone = go.loss_grad(u[rest], tgt[rest], *inp["w"], 0.5)
    assert hit["loss"][3] == 0 and (hit["dz"][3] == 0).all()
    for n in GRADS:
        assert np.isfinite(hit[n]).all() and np.allclose(hit[n], alone[n], rtol=0, atol=1e-15 * max(np.abs(alone[n]).max(), 1e-300))


def test_host_matrices_and_bad_arguments_are_refused(monkeypatch):
    monkeypatch.setattr(_train, "lib", lambda: pytest.fail("the library was loaded"))
    inp = case_inputs(1)
    C, T, L, U, K, clip, batch, lead, _s, _w = CASES[1]
    y = torch.zeros((K, T))
    w = tuple(torch.zeros(s) for s in ((4 * U, C), (4 * U,), (4 * U, U), (K, U), (K,)))
    for bad in (inp["x"], torch.from_numpy(inp["x"])):
        with pytest.raises(ValueError, match="no CPU path"):
            lstm.loss_and_grad(bad, y, torch.from_numpy(inp["idx"]), w, inp["mean"], inp["std"], L, lead, clip)
        with pytest.raises(ValueError, match="no CPU path"):
            lstm.LSTMDecoder(U, L, lead, clip).fit(bad, y, engine="device")
        with pytest.raises(ValueError, match="no CPU path"):
            lstm.cross_validate(bad, y, L, engine="device")
    with pytest.raises(ValueError, match="engine"):
        lstm.LSTMDecoder(U, L, lead, clip).fit(torch.from_numpy(inp["x"]), y, engine="triton")
