"""The spike-count Gram matrix without a GPU (mhi_gram, include/muahuff_ingest.h; gram.py): the ABI's three descriptions
agree, every argument error comes back before a pointer is used -- with the text tests/gram_check.cpp prints, which is
csrc/mh_gram_layout.hpp built alone under AddressSanitizer + UBSan --, the tiles and the runs of K slices cover the result
and the columns exactly once with no int32 run past its bound, the XOR fix-up identity holds on the boundary values, and
Gram's float arithmetic is what its docstrings say."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _ingest, _lib, gram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "gram_check.cpp")
TILE, SLICE, RUN_SLICES, STEP, INT32_COLS, MAX_BLOCKS, TARGET = 128, 4096, 16, 64, 131071, 2048, 4096


@pytest.fixture(scope="module", autouse=True)
def built():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_ingest.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhi_\w+)\s*\(", code))
    assert declared == set(_ingest.PROTOTYPES) and "mhi_gram" in declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _ingest.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[-1].startswith("mhi_")}
    assert exported == declared
    args = re.search(r"\bmhi_gram\s*\(([^)]*)\)", code).group(1)
    assert len(args.split(",")) == len(_ingest.PROTOTYPES["mhi_gram"][1]) == 13
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_gram.hpp", "csrc/mh_gram_layout.hpp"} <= set(build.INGEST_HEADERS)
    assert _ingest.lib().mhi_version() == 103
    assert muahuff.gram is gram


# ---- argument errors ---------------------------------------------------------------------------------------------------
ORDER = ("a", "a_row_stride", "a_rows", "b", "b_row_stride", "b_rows", "cols", "gram", "gram_row_stride", "sum_a", "sum_b",
         "accumulate")
POINTERS = ("a", "b", "gram", "sum_a", "sum_b")


def _args(**over):
    """mhi_gram's arguments with host stand-ins for the device buffers (kept alive in the first item)"""
    keep = {k: np.zeros(4096, np.uint64) for k in POINTERS}
    a = dict(a_row_stride=128, a_rows=3, b_row_stride=128, b_rows=4, cols=100, gram_row_stride=32, accumulate=0)
    for k, v in keep.items():
        a[k] = v.ctypes.data + (-v.ctypes.data) % 16
    shift = {k[:-6]: over.pop(k) for k in list(over) if k.endswith("_shift")}
    for k, v in over.items():
        a[k] = (0 if v is None else v)
    for k, s in shift.items():
        a[k] += s
    return keep, a


def _call(a):
    L = _ingest.lib()
    vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in ORDER]
    rc = L.mhi_gram(*vals, None)
    return rc, L.mhi_last_error().decode()


T40 = 1 << 40
SYM = dict(b=None, gram_row_stride=24)
BAD = [dict(a=None), dict(gram=None), dict(SYM, a=None), dict(SYM, gram=None),
       dict(a_rows=0), dict(b_rows=0), dict(cols=0), dict(SYM, a_rows=0), dict(SYM, cols=0),
       dict(cols=T40, a_row_stride=T40, b_row_stride=T40), dict(cols=T40 + 5, a_row_stride=T40 + 5, b_row_stride=T40 + 5),
       dict(SYM, cols=T40, a_row_stride=T40),
       dict(a_row_stride=99), dict(a_row_stride=0), dict(b_row_stride=99), dict(b_row_stride=0), dict(SYM, a_row_stride=99),
       dict(gram_shift=4), dict(gram_shift=1), dict(gram_row_stride=36), dict(gram_row_stride=33), dict(gram_row_stride=24),
       dict(SYM, gram_row_stride=16), dict(sum_a_shift=4), dict(sum_b_shift=1), dict(SYM, sum_a_shift=2),
       dict(accumulate=2),
       dict(a_rows=(1 << 31) + 1, gram_row_stride=1 << 20), dict(b_rows=(1 << 31) + 1, gram_row_stride=1 << 40),
       dict(a_rows=1 << 31, b_rows=1 << 31, gram_row_stride=1 << 40, cols=T40 - 1, a_row_stride=T40, b_row_stride=T40)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items())   # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=_ids)
def test_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(**bad)
    rc, msg = _call(a)
    del keep
    assert rc == _lib.ERR_ARG and "mhi_gram" in msg, (rc, msg)


def _line(a):
    return "check " + " ".join(str(a[k]) for k in ORDER) + "\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gram") / "gram_check_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def _run(exe_path, text):
    r = subprocess.run([exe_path], input=text, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


# arguments on the accepted side of every bound: the check program says "ok" (the library would launch: not called here)
GOOD = [dict(), dict(SYM), dict(sum_a=None, sum_b=None), dict(accumulate=1), dict(a_row_stride=100, b_row_stride=100),
        dict(a_rows=1, a_row_stride=0, gram_row_stride=0), dict(b_rows=1, b_row_stride=0, gram_row_stride=8),
        dict(SYM, a_rows=1, a_row_stride=0, gram_row_stride=0), dict(a_shift=1, b_shift=15),
        dict(cols=T40 - 1, a_row_stride=T40 - 1, b_row_stride=T40),
        dict(SYM, b_rows=0, b_row_stride=0),                              # ignored in the symmetric form
        dict(a_rows=1 << 31, b_rows=1, gram_row_stride=8, cols=64)]


def test_the_check_program_and_the_library_give_the_same_codes_and_messages(exe):
    cases = [_args(**b) for b in BAD]
    lines = _run(exe, "".join(_line(a) for _k, a in cases))
    assert len(lines) == len(BAD)
    for (keep, a), ln, b in zip(cases, lines, BAD):
        rc, msg = _call(a)
        assert ln == "error %d %s" % (rc, msg) and rc == _lib.ERR_ARG, (b, ln, msg)
    good = [_args(**g) for g in GOOD]
    assert _run(exe, "".join(_line(a) for _k, a in good)) == ["ok"] * len(GOOD)


def layout(a_rows, b_rows, cols, symmetric):
    """mh_gram_layout.hpp's rule, restated -> [nta, ntb, tiles, slices, run_slices, runs, items, grid, max_blocks,
    longest run]"""
    nta = -(-a_rows // TILE)
    ntb = nta if symmetric else -(-b_rows // TILE)
    tiles = nta * (nta + 1) // 2 if symmetric else nta * ntb
    slices = -(-cols // SLICE)
    run_slices = min(max(-(-tiles * slices // TARGET), 1), RUN_SLICES)
    runs = -(-slices // run_slices)
    items = runs * tiles
    grid = -(-min(items, MAX_BLOCKS) // 8) * 8
    return [nta, ntb, tiles, slices, run_slices, runs, items, grid, MAX_BLOCKS, min(cols, run_slices * SLICE)]


ROWS = [1, 15, 16, 17, 127, 129, 1024, 16385]
COLS = [1, 63, 64, 65, 131071, 131072, 10 ** 7, 2 ** 40 - 1]
# the shapes of tests/test_gpu_gram_tiles.py: the header itself answers for them, not only its restatement
GPU_SHAPES = [(260, 129, 200, 0), (129, 260, 200, 0), (643, 643, 130, 1), (515, 515, 139 * SLICE + 65, 1),
              (7803, 7803, 131072 + 65, 1), (7803, 300, 131072 + 65, 0), (1, 1, 2 ** 32 + 4099, 1), (1, 1, 2 ** 32 + 4092, 0)]


def test_tiles_slices_runs_and_the_grid_over_the_sweep(exe):
    """gram_check asserts per shape: every (tile, column) owned once per run of slices, the runs cover [0, cols) once,
    no int32 run above 131071 columns, the symmetric grid owns exactly the tiles with j >= i, the grid under its cap"""
    grid = [(ra, rb, c, 0) for ra in ROWS for rb in (ROWS[0], ROWS[-1], ra) for c in COLS]
    grid += [(ra, ra, c, 1) for ra in ROWS for c in COLS]
    grid += GPU_SHAPES
    lines = _run(exe, "".join("layout %d %d %d %d\n" % g for g in grid))
    assert len(lines) == len(grid)
    strided = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == layout(*g), (g, got)
        assert got[9] <= SLICE * RUN_SLICES <= INT32_COLS and got[7] <= MAX_BLOCKS and got[7] % 8 == 0
        strided += got[6] > got[7]
    assert strided > 20
    # the shapes tests/test_gpu_gram.py relies on: at least three runs in the int32 case, a strided grid in the long one
    assert layout(18, 18, 131072 + 65, 1)[5] >= 3
    assert layout(18, 18, MAX_BLOCKS * SLICE * RUN_SLICES + SLICE + 65, 1)[6] > MAX_BLOCKS
    # ... and tests/test_gpu_gram_tiles.py: [nta, ntb, tiles, slices, run_slices, runs, items, grid] of each of its shapes
    assert layout(18, 18, 131072 + 65, 1)[:6] == [1, 1, 1, 33, 1, 33]          # the int32 case above: runs of ONE slice
    assert layout(260, 129, 200, 0)[:8] == [3, 2, 6, 1, 1, 1, 6, 8] and layout(129, 260, 200, 0)[:8] == [2, 3, 6, 1, 1, 1, 6, 8]
    assert layout(643, 643, 130, 1)[:8] == [6, 6, 21, 1, 1, 1, 21, 24]
    assert layout(515, 515, 139 * SLICE + 65, 1)[:8] == [5, 5, 15, 140, 1, 140, 2100, MAX_BLOCKS]
    assert layout(7803, 7803, 131072 + 65, 1) == [61, 61, 1891, 33, 16, 3, 5673, MAX_BLOCKS, MAX_BLOCKS, 65536]
    assert layout(7803, 300, 131072 + 65, 0) == [61, 3, 183, 33, 2, 17, 3111, MAX_BLOCKS, MAX_BLOCKS, 8192]
    assert layout(1, 1, 2 ** 32 + 4099, 1) == [1, 1, 1, 2 ** 20 + 2, 16, 65537, 65537, MAX_BLOCKS, MAX_BLOCKS, 65536]
    assert layout(1, 1, 2 ** 32 + 4099 - 7, 0)[4:7] == [16, 65537, 65537]
    # the headline shape of DESIGN.md, for comparison: the same regime as the 7803-row case
    assert layout(1024, 1024, 10 ** 7, 1)[:7] == [8, 8, 36, 2442, 16, 153, 5508]


def test_the_xor_fix_up_identity_on_the_boundary_values():
    """sum x_i x_j = sum z_i z_j + 128 (sum x_i + sum x_j) - 16384 K with z = (x XOR 0x80) as int8 and K the padded
    column count, padding loaded as x = 0"""
    vals = np.array([0, 1, 127, 128, 255], np.uint8)
    rng = np.random.RandomState(0)
    for cols in (1, 5, 63, 64, 65, 200):
        K = -(-cols // STEP) * STEP
        x = np.concatenate([np.repeat(vals[:, None], cols, 1), vals[rng.randint(0, 5, (6, cols))]])
        xp = np.zeros((x.shape[0], K), np.uint8)
        xp[:, :cols] = x
        z = (xp ^ 0x80).view(np.int8).astype(np.int64)
        assert np.array_equal(z, xp.astype(np.int64) - 128)
        s = x.sum(1, dtype=np.int64)
        fixed = z @ z.T + 128 * (s[:, None] + s[None, :]) - 16384 * K
        assert np.array_equal(fixed, x.astype(np.int64) @ x.astype(np.int64).T)
    # the worst case of an int32 accumulator is the all-zero matrix: 16384 per column
    assert 16384 * INT32_COLS < 2 ** 31 <= 16384 * (INT32_COLS + 1)


def test_gram_cov_and_corr_on_hand_made_integers():
    x = np.array([[1, 2, 3, 4], [2, 4, 6, 8], [5, 5, 5, 5], [4, 1, 0, 3]], np.int64)
    G, s, n = x @ x.T, x.sum(1), 4
    g = gram.Gram(n, torch.from_numpy(s), torch.from_numpy(s.copy()), torch.from_numpy(G), True)
    assert np.allclose(g.cov().numpy(), np.cov(x), rtol=0, atol=1e-12)
    assert np.allclose(g.cov(ddof=0).numpy(), np.cov(x, ddof=0), rtol=0, atol=1e-12)
    assert g.cov().dtype == torch.float64 and g.mean()[0].tolist() == [2.5, 5.0, 5.0, 2.0]
    c = g.corr().numpy()
    want = np.corrcoef(x[[0, 1, 3]])
    assert np.allclose(c[np.ix_([0, 1, 3], [0, 1, 3])], want, rtol=0, atol=1e-12) and c[0, 1] == pytest.approx(1.0)
    assert np.isnan(c[2]).all() and np.isnan(c[:, 2]).all()                  # the constant row has no variance
    # disjoint time ranges add
    a, b = x[:, :1], x[:, 1:]
    ga = gram.Gram(1, torch.from_numpy(a.sum(1)), torch.from_numpy(a.sum(1)), torch.from_numpy(a @ a.T), True)
    gb = gram.Gram(3, torch.from_numpy(b.sum(1)), torch.from_numpy(b.sum(1)), torch.from_numpy(b @ b.T), True)
    both = ga + gb
    assert both.n == 4 and torch.equal(both.gram, g.gram) and torch.equal(both.sum_a, g.sum_a) and both.symmetric
    cross = gram.Gram(4, g.sum_a, g.sum_b[:3], g.gram[:, :3])
    with pytest.raises(ValueError):
        cross.corr()
    with pytest.raises(ValueError):
        g + cross
    # a leading lag axis
    lag = gram.Gram([4, 2], torch.stack([g.sum_a, g.sum_a]), torch.stack([g.sum_b, g.sum_b]), torch.stack([g.gram, g.gram]))
    assert tuple(lag.cov().shape) == (2, 4, 4) and np.allclose(lag.cov()[0].numpy(), np.cov(x), rtol=0, atol=1e-12)


def test_host_matrices_and_bad_arguments_are_refused(monkeypatch):
    monkeypatch.setattr(_ingest, "lib", lambda: pytest.fail("the library was loaded"))
    host = np.zeros((3, 100), np.uint8)
    for x in (host, torch.from_numpy(host)):
        with pytest.raises(ValueError, match="no CPU path"):
            gram.gram(x)
    with pytest.raises(ValueError):
        gram.gram(torch.from_numpy(host), lag=-1)
    with pytest.raises(ValueError):
        gram.gram(torch.from_numpy(host), lag=[])
    from muahuff import container_io as cio
    with pytest.raises(ValueError, match="no CPU path"):
        cio.decompress_gram(host)
    for kw in (dict(start=0, stop=10, bin=0), dict(start=0, stop=10, bin=4097), dict(start=5, stop=3), dict(start=0, stop=101),
               dict(start=3, stop=50, bin=5), dict(start=-1, stop=5)):
        with pytest.raises(ValueError):
            gram.gram_args(kw["start"], kw["stop"], kw.get("bin"), 100)
    assert gram.gram_args(10, 57, 5, 100) == (10, 5, 9) and gram.gram_args(3, 50, None, 100) == (3, 1, 47)
    assert gram.batches(10, 4, 12) == [(0, 3), (3, 3), (6, 3), (9, 1)] and gram.batches(10, 4, 1) == [(i, 1) for i in range(10)]
