"""Trial-aligned windows without a GPU (mhi_windows, include/muahuff_ingest.h; windows.py): the ABI's three descriptions
agree, every argument error comes back before a pointer is used -- with the text tests/windows_check.cpp prints, which is
csrc/mh_windows_layout.hpp built alone under AddressSanitizer + UBSan -- the tiles of every form cover a window's bins
exactly once, the capped grid follows its rule, the host planner agrees with brute force, and the Python entry points
refuse what they cannot do before anything is loaded."""
import ctypes as ct
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _ingest, _lib, windows
from muahuff import container_io as cio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "windows_check.cpp")
STACK, SUM = 0, 1
CH = muahuff.CHUNK


@pytest.fixture(scope="module", autouse=True)
def built():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()


def test_header_map_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "muahuff_ingest.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhi_\w+)\s*\(", code))
    assert declared == set(_ingest.PROTOTYPES) and "mhi_windows" in declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _ingest.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.split()[-1].startswith("mhi_")}
    assert exported == declared
    args = re.search(r"\bmhi_windows\s*\(([^)]*)\)", code).group(1)
    assert len(args.split(",")) == len(_ingest.PROTOTYPES["mhi_windows"][1]) == 20
    assert "#define MHI_WIN_STACK 0u" in hdr and "#define MHI_WIN_SUM   1u" in hdr
    assert (_ingest.WIN_STACK, _ingest.WIN_SUM) == (STACK, SUM)
    build = importlib.import_module("hardware-efficient-mua-compression_amd.build")
    assert {"csrc/mh_windows.hpp", "csrc/mh_windows_layout.hpp"} <= set(build.INGEST_HEADERS)
    assert _ingest.lib().mhi_version() == 103
    assert muahuff.windows is windows


# ---- argument errors ---------------------------------------------------------------------------------------------------
ORDER = ("inp", "row_stride", "rows", "cols", "win_off", "win_idx", "n_win", "n_out", "W", "r", "mode", "out", "out_bits",
         "out_win_stride", "out_row_stride", "sumsq", "sq_row_stride", "accumulate", "bad")
POINTERS = ("inp", "win_off", "win_idx", "out", "sumsq", "bad")


def _args(**over):
    """mhi_windows' arguments with host stand-ins for the device buffers (kept alive in the first item)"""
    keep = {k: np.zeros(4096, np.uint64) for k in POINTERS}
    a = dict(row_stride=128, rows=3, cols=100, n_win=5, n_out=5, W=10, r=2, mode=STACK, out_bits=8, out_win_stride=64,
             out_row_stride=16, sq_row_stride=0, accumulate=0)
    for k, v in keep.items():
        a[k] = v.ctypes.data + (-v.ctypes.data) % 16
    a["sumsq"] = 0
    a["win_idx"] = 0
    shift = {k[:-6]: over.pop(k) for k in list(over) if k.endswith("_shift")}
    for k, v in over.items():
        a[k] = (keep[k].ctypes.data + (-keep[k].ctypes.data) % 16 if v == "given" else 0 if v is None else v) if k in POINTERS else v
    for k, s in shift.items():
        a[k] += s
    return keep, a


def _call(a):
    L = _ingest.lib()
    vals = [ct.c_void_p(a[k]) if k in POINTERS else a[k] for k in ORDER]
    rc = L.mhi_windows(*vals, None)
    return rc, L.mhi_last_error().decode()


T32 = 1 << 32
SUM_OK = dict(mode=SUM, out_bits=32, out_row_stride=64)
BAD = [dict(inp=None), dict(out=None), dict(bad=None), dict(win_off=None),
       dict(mode=2), dict(mode=7),
       dict(out_bits=16), dict(out_bits=0), dict(out_bits=64), dict(SUM_OK, out_bits=8), dict(SUM_OK, out_bits=16),
       dict(sumsq="given"), dict(accumulate=1), dict(SUM_OK, accumulate=2),
       dict(out_bits=32, out_shift=2), dict(out_bits=32, out_row_stride=18), dict(out_bits=32, out_win_stride=66),
       dict(SUM_OK, out_shift=1), dict(SUM_OK, out_row_stride=6),
       dict(SUM_OK, sumsq="given", sumsq_shift=4, sq_row_stride=64), dict(SUM_OK, sumsq="given", sq_row_stride=60),
       dict(rows=0), dict(cols=0), dict(W=0), dict(r=0),
       dict(W=T32, cols=T32 + 5), dict(W=T32 + 7, cols=T32 + 9), dict(r=T32), dict(n_win=T32),
       dict(row_stride=99), dict(row_stride=0),
       dict(SUM_OK, n_win=-(-T32 // (255 * 2)), r=2),                 # the first refused n_win: n * 255 * 2 >= 2^32
       dict(SUM_OK, n_win=-(-T32 // (255 * 10)), r=64, W=10),         # ... min(r, W) = W
       dict(SUM_OK, n_win=T32 - 1, r=1),
       dict(rows=1 << 62, row_stride=1 << 40)]
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items())   # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=_ids)
def test_argument_errors_come_before_any_device_work(bad):
    keep, a = _args(**bad)
    rc, msg = _call(a)
    del keep
    assert rc == _lib.ERR_ARG and "mhi_windows" in msg, (rc, msg)


def _line(a):
    return "check " + " ".join(str(a[k]) for k in ORDER) + "\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("windows") / "windows_check_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def _run(exe_path, text):
    r = subprocess.run([exe_path], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


# arguments on the accepted side of every bound: the check program says "ok" (the library would launch: not called here)
GOOD = [dict(), dict(out_bits=32), dict(win_idx="given"), dict(SUM_OK), dict(SUM_OK, sumsq="given", sq_row_stride=64),
        dict(SUM_OK, accumulate=1), dict(n_win=0, win_off=None), dict(SUM_OK, n_win=0, win_off=None),
        dict(W=T32 - 1, cols=T32 + 5, row_stride=T32 + 5), dict(r=T32 - 1), dict(n_win=T32 - 1), dict(row_stride=100), dict(rows=1, row_stride=0),
        dict(SUM_OK, n_win=-(-T32 // (255 * 2)) - 1, r=2),            # the last accepted n_win
        dict(SUM_OK, n_win=-(-T32 // (255 * 10)) - 1, r=64, W=10),
        dict(SUM_OK, n_win=T32 - 1, r=1, accumulate=1),               # with accumulate the caller owns the bound
        dict(out_bits=8, out_shift=1, out_row_stride=7, out_win_stride=3)]


def test_the_check_program_and_the_library_give_the_same_codes_and_messages(exe):
    cases = [_args(**b) for b in BAD]
    lines = _run(exe, "".join(_line(a) for _k, a in cases))
    assert len(lines) == len(BAD)
    for (keep, a), ln, b in zip(cases, lines, BAD):
        rc, msg = _call(a)
        assert ln == "error %d %s" % (rc, msg) and rc == _lib.ERR_ARG, (b, ln, msg)
    good = [_args(**g) for g in GOOD]
    assert _run(exe, "".join(_line(a) for _k, a in good)) == ["ok"] * len(GOOD)
    assert -(-T32 // 510) * 510 >= T32 > (-(-T32 // 510) - 1) * 510       # the two n_win above straddle the bound


def _layout(mode, rows, W, r, n_win):
    """mh_windows_layout.hpp's rule, restated"""
    nb = -(-W // r)
    form, tile_bins = (0, 16) if r == 1 else (1, 1024 // r) if r <= 64 else (2, 1)
    tiles = -(-nb // tile_bins)
    items = (n_win if mode == STACK else 1) * rows * tiles
    per = 256 if form == 0 else 4
    return [form, nb, tile_bins, tiles, items, per, min(-(-items // per), 4096), 4096]


def test_layout_around_every_form_switch_and_the_grid_cap(exe):
    around = lambda x: [x - 1, x, x + 1]     # noqa: E731
    grid = []
    for W in [1, 15, 16, 17, 64, 1000, 1023, 1024, 1025, 4099, 2 ** 20 + 3, T32 - 1]:
        for r in sorted({1, 2, 3, 5, 15, 16, 17, 50, 63, 64, 65, 66, 1023, 1024, 1025, 4096, W, min(W + 1, T32 - 1), T32 - 1}):
            for mode, rows, n_win in ((STACK, 3, 7), (SUM, 70, 300), (STACK, 1, 0), (SUM, 1, 0)):
                grid.append((mode, rows, W, r, n_win))
    # on both sides of the cap: 4096 workgroups of 256 lanes (r == 1) or of 4 waves
    for n_win in around(4096 * 256 // 70) + around(4096 * 256):
        grid.append((STACK, 70 if n_win < 10 ** 5 else 1, 16, 1, n_win))
    for n_win in around(4096 * 4 // 2) + [500, 30000]:
        grid += [(STACK, 2, 17, 2, n_win), (STACK, 2, 700, 100, n_win)]
    for rows in around(4096 * 256 // 63) + around(4096 * 4):
        grid += [(SUM, rows, 1000, 1, 3), (SUM, rows, 17, 2, 3), (SUM, rows, 66, 65, 3)]
    lines = _run(exe, "".join("layout %d %d %d %d %d\n" % g for g in grid))
    assert len(lines) == len(grid) > 500
    capped = 0
    for g, ln in zip(grid, lines):
        got = [int(v) for v in ln.split()]
        assert got == _layout(*g), (g, got)
        capped += got[4] > 4096 * got[5]
    assert capped > 10
    # the shapes tests/test_gpu_windows.py uses to cross the cap do cross it
    assert _layout(STACK, 70, 1, 1, 15000)[4] > 4096 * 256 and _layout(STACK, 70, 17, 2, 300)[4] > 4096 * 4
    assert _layout(STACK, 70, 700, 100, 40)[4] > 4096 * 4
    assert _layout(SUM, 17000, 1000, 1, 2)[4] > 4096 * 256 and _layout(SUM, 17000, 17, 2, 2)[4] > 4096 * 4
    assert _layout(SUM, 17000, 66, 65, 2)[4] > 4096 * 4


# ---- the planner -------------------------------------------------------------------------------------------------------
def _check_plan(starts, W, T, join, budget):
    plan = windows.plan_spans(starts, W, T, join, budget)
    n = len(starts)
    assert sorted(plan.order.tolist()) == list(range(n))
    s = np.asarray(starts)[plan.order]
    assert (np.diff(s) >= 0).all()
    rec = (np.arange(T) * 2654435761 % 251).astype(np.uint8)
    seen, prev = 0, None
    for bt in plan.batches:
        assert budget is None or bt.cols <= budget                                   # no batch is over budget
        assert bt.first == seen and len(bt.offsets) == bt.last - bt.first > 0
        lens = bt.spans[:, 1] - bt.spans[:, 0]
        assert (lens >= W).all() and bt.cols == lens.sum()
        assert np.array_equal(bt.base, np.concatenate([[0], np.cumsum(lens)[:-1]]))
        scratch = np.concatenate([rec[a:b] for a, b in bt.spans])                    # the matrix cut by the plan
        inside = np.zeros(bt.last - bt.first, int)
        for j, ((a, b), early) in enumerate(zip(bt.spans.tolist(), bt.early.tolist())):
            assert 0 <= a < b <= T
            if prev is not None:
                assert a >= prev[0]                                                  # ascending
                if not prev[2]:
                    assert a > prev[1] + join                                        # disjoint, and not joinable
                else:
                    assert a <= prev[1] + join and a + W - prev[0] > budget          # only the budget closes a span early
            prev = (a, b, early)
            w = s[bt.first:bt.last]
            mine = (bt.offsets >= bt.base[j]) & (bt.offsets < bt.base[j] + (b - a))
            assert ((w[mine] >= a) & (w[mine] + W <= b)).all() and w[mine].min() == a and w[mine].max() + W == b
            inside += mine
        assert (inside == 1).all()                                                   # every window in exactly one span
        for k in range(bt.first, bt.last):
            o = bt.offsets[k - bt.first]
            assert np.array_equal(scratch[o:o + W], rec[s[k]:s[k] + W])
        seen = bt.last
    assert seen == n
    # brute force: the spans without a budget are the connected runs of the join rule
    if budget is None:
        want, a, b = [], s[0], s[0] + W
        for st in s[1:]:
            if st <= b + join:
                b = st + W
            else:
                want.append((a, b))
                a, b = st, st + W
        want.append((a, b))
        got = [tuple(sp) for bt in plan.batches for sp in bt.spans.tolist()]
        assert got == [(int(x), int(y)) for x, y in want] and len(plan.batches) == 1
    return plan


def test_plan_spans_against_brute_force():
    rng = np.random.RandomState(5)
    early = many = 0
    for trial in range(200):
        W = int(rng.choice([1, 7, 100, 1000]))
        join = int(rng.choice([0, 1, 50, 3000, CH]))
        T = int(rng.choice([W, W + 1, 5000, 300000]))
        n = int(rng.choice([1, 2, 5, 40, 200]))
        starts = rng.randint(0, T - W + 1, n)
        if trial % 3 == 0 and T > 5 * (W + join) + 8:     # touching windows; gaps of join - 1, join and join + 1
            base = int(rng.randint(0, T - 5 * (W + join) - 7))
            a = base + W
            made = [base, base, a]
            for gap in (join - 1, join, join + 1):
                made.append(made[-1] + W + max(gap, 0))
            starts = np.concatenate([starts, made])
        starts = rng.permutation(starts)
        _check_plan(starts, W, T, join, None)
        budget = int(rng.choice([W, W + 1, 2 * W + 3, 10 * W, 20000]))
        plan = _check_plan(starts, W, T, join, budget)
        early += sum(int(bt.early.sum()) for bt in plan.batches)
        many += len(plan.batches) > 1
    assert early > 50 and many > 50
    # the gap rule on both sides, spelled out
    spans = lambda st, j: [tuple(x) for bt in windows.plan_spans(st, 10, 10 ** 6, j).batches for x in bt.spans.tolist()]   # noqa: E731
    assert spans([0, 10 + 99], 100) == [(0, 119)] and spans([0, 10 + 100], 100) == [(0, 120)]
    assert spans([0, 10 + 101], 100) == [(0, 10), (111, 121)]
    assert spans([5, 10 + CH + 5], CH) == [(5, CH + 25)] and spans([5, 10 + CH + 6], CH) == [(5, 15), (CH + 16, CH + 26)]
    assert windows.plan_spans(np.zeros(0, np.int64), 10, 100).batches == []


def test_plan_spans_refuses():
    with pytest.raises(ValueError, match="wider than the budget"):
        windows.plan_spans([0, 5], 100, 1000, budget=99)
    windows.plan_spans([0, 5], 100, 1000, budget=100)
    with pytest.raises(ValueError, match=r"window 1: \[901, 1001\)"):
        windows.plan_spans([0, 901], 100, 1000)
    with pytest.raises(ValueError, match="window 0"):
        windows.plan_spans([-1, 5], 100, 1000)
    with pytest.raises(ValueError):
        windows.plan_spans([0.5], 100, 1000)


# ---- the Python entry points refuse before anything is loaded ---------------------------------------------------------
class _NoSource:
    """a stand-in for a Compressed: the argument rules come before any of it is read"""
    ch_len = np.array([1000, 400], np.uint64)

    @property
    def header(self):
        raise AssertionError("the source was read before the arguments were checked")


def test_host_matrices_and_bad_arguments_are_refused(monkeypatch):
    monkeypatch.setattr(_ingest, "lib", lambda: pytest.fail("the library was loaded"))
    host = np.zeros((3, 100), np.uint8)
    for x in (host, torch.from_numpy(host)):
        with pytest.raises(ValueError, match="no CPU path"):
            windows.gather(x, [0, 5], 10)
        with pytest.raises(ValueError, match="no CPU path"):
            windows.psth(x, [0, 5], 10, moments=2)
        with pytest.raises(ValueError, match="no CPU path"):
            cio.decompress_windows(x, [50], 10, 10)
    src = _NoSource()
    for kw in (dict(pre=-1, post=5), dict(pre=5, post=-1), dict(pre=0, post=0), dict(pre=5, post=5, bin=0),
               dict(pre=5, post=5, bin=4097), dict(pre=5, post=5, reduce="mean"), dict(pre=5, post=5, moments=3),
               dict(pre=5, post=5, reduce="sum", bin=4096, triggers=[500] * 900000)):
        trig = kw.pop("triggers", [500])
        with pytest.raises(ValueError):
            cio.decompress_windows(src, trig, **kw)
    with pytest.raises(ValueError, match="trigger 4:"):
        cio.decompress_windows(src, [500, 4], 5, 5)
    with pytest.raises(ValueError, match="trigger 996:"):
        cio.decompress_windows(src, [500, 995, 996], 5, 5)


def test_read_windows_checks_its_arguments_before_it_reads(tmp_path):
    """archive.Reader.read_windows on an archive of oracle-encoded blocks: nothing is read for a refused call"""
    from muahuff import archive
    from tests import helpers
    from tests.test_host_archive import LENS, SC, C, S, _block
    path = str(tmp_path / "a.mua")
    with archive.create(path, C, S=S, sclv_rows=helpers.sclv_tables()[S], seg_chunks=SC) as w:
        for k, Tb in enumerate(LENS[:2]):
            w.append_compressed(_block(Tb, seed=k))
    with archive.open(path) as rd:
        before = rd.bytes_read
        for kw in (dict(pre=-1, post=5), dict(pre=0, post=0), dict(pre=5, post=5, bin=0), dict(pre=5, post=5, bin=4097),
                   dict(pre=5, post=5, reduce="mean"), dict(pre=5, post=5, moments=0)):
            with pytest.raises(ValueError):
                rd.read_windows([100], **kw)
        with pytest.raises(ValueError, match="trigger 3:"):
            rd.read_windows([100, 3], 5, 5)
        with pytest.raises(ValueError, match="trigger %d:" % (rd.T - 4)):
            rd.read_windows([100, rd.T - 5, rd.T - 4], 5, 5)
        with pytest.raises(IndexError):
            rd.read_windows([100], 5, 5, channels=[rd.C])
        assert rd.bytes_read == before
