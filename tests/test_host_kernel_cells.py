"""The table of codec kernel cells (tests/kernel_cells.py) against the shipped code object, the host planner and the
library's kernel selection (csrc/mh_select.hpp, run by tests/planner_check.cpp --cells).  Runs without a GPU: a kernel
instance added to libmuahuff.so fails here until it gets a cell, a cell whose kernel is no longer shipped fails as
well, a cell whose plans no longer land on its kernel fails before any GPU run, and so does a launch whose dynamic-LDS
request changes."""
import os
import re
import subprocess

import pytest

from tests import kernel_cells as kc
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def code_object_symbols(tmp_path, pattern):
    """demangled names of the kernels in the gfx950 code object of libmuahuff.so whose symbol matches `pattern`"""
    from muahuff import _lib
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("no ROCm LLVM tools here")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([tools[0], "--dump-section", ".hip_fatbin=" + fat, _lib.SO], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    table = subprocess.run([tools[2], "-t", co], check=True, capture_output=True, text=True).stdout
    # kernel entry points are the function symbols (their descriptors are the ".kd" objects)
    mangled = sorted({ln.split()[-1] for ln in table.splitlines() if " F " in ln and re.search(pattern, ln)})
    if not mangled:
        return set()
    names = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", check=True, capture_output=True,
                           text=True).stdout.split("\n")[:len(mangled)]
    return {n.strip() for n in names}


def test_shipped_codec_instances_are_exactly_the_42_cells(tmp_path):
    shipped = set()
    for n in code_object_symbols(tmp_path, r"k_(en|de)code2"):
        m = re.fullmatch(r"void (mh::k_(?:en|de)code2w?<[^>]*>)\(mh::(?:Enc|Dec)2Args\)", n)
        assert m, n
        shipped.add(m.group(1))
    cells = [c.symbol for c in kc.CELLS]
    assert len(cells) == len(set(cells)), "one cell per kernel instance"
    assert (len(kc.ENCODER_CELLS), len(kc.DECODER_CELLS), len(kc.PACKED_DECODER_CELLS)) == (24, 8, 10)
    assert len(shipped) == 42
    assert set(cells) == shipped, dict(without_cell=sorted(shipped - set(cells)), not_shipped=sorted(set(cells) - shipped))


def test_cell_symbols_name_their_task_form_and_input():
    for c in kc.CELLS:
        assert ("2w<" in c.symbol) == c.wave, c.symbol
        # the last template argument: PK (packed input) of an encoder, PO (packed output) of a decoder
        last = int(c.symbol.rstrip(">").split(",")[-1])
        assert last == (0 if c.input_bits == 8 else c.input_bits), c.symbol
        for k in c.cases:
            if c.input_bits == 2:
                assert k.S <= 4, (c.symbol, k.S)
            if c.decoder and c.input_bits != 8:   # mh_decode_packed: 2 bits for S <= 4, 4 bits for S >= 5
                assert c.input_bits == (2 if k.S <= 4 else 4), (c.symbol, k.S)
            if not c.decoder and c.input_bits == 8:
                pb = int(c.symbol.split("<")[1].split(",")[1])
                assert pb == (3 if k.S <= 8 else 4), (c.symbol, k.S)


def planned(exe, lines):  # noqa: F811  (a path here, the fixture's value)
    """planner_check --cells over `lines`: per case (maxlen, wave, W, [(instance name, dynamic-LDS bytes), ...]) as the
    library's selection (csrc/mh_select.hpp) gives them -- encoder, decoder (("-", 0): mh_decode_packed refuses the
    plan) and, for byte plans, k_decode_range and k_decode_rebin"""
    r = subprocess.run([exe, "--cells"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    out = []
    for g in got:
        f = g.split("|")
        maxlen, wave, W = (int(v) for v in f[0].split())
        out.append((maxlen, wave, W, [(f[i], int(f[i + 1])) for i in range(1, len(f), 2)]))
    return out


def _line(lens, S, h, mode, rows, sc, input_bits, window=3):
    return "%d %d %d %d %d %d %d %d  %s  %s" % (len(lens), S, h, mode, window, len(rows), sc, input_bits,
                                                " ".join(map(str, lens)), " ".join(str(v) for r in rows for v in r))


@pytest.fixture(scope="module")
def cell_plans(exe):  # noqa: F811
    """each case x layout of each cell through the library's selection, once for the module"""
    want = [(c, k, lens, sc) for c in kc.CELLS for k in c.cases for lens, sc in c.layouts]
    lines = [_line(lens, k.S, 0 if c in kc.PACKED_DECODER_CELLS else 6, c.mode, k.rows, sc, c.input_bits)
             for c, k, lens, sc in want]
    return list(zip(want, planned(exe, lines)))


def test_every_cell_lands_where_the_table_says(cell_plans):
    """Each case x layout of each cell through the host planner and the library's own selection (--cells): maxlen, the
    task form and, for decoder cells, W; the instance the selection names is the cell's symbol, for decoder and encoder
    cells alike, and so are its K and NR.  Packed decoder cells are planned as StreamDecoder plans its blocks, without
    a calibration window (h = 0)."""
    for (c, k, lens, sc), (maxlen, wave, W, picks) in cell_plans:
        tag = (c.symbol, k.S, k.rows, lens, sc)
        assert maxlen == k.maxlen, tag
        assert wave == int(c.wave), tag
        assert len(picks) == (4 if c.input_bits == 8 else 2), tag
        if c.decoder:
            assert W == k.W, tag
            assert picks[1][0] == c.symbol, tag
            K, _m, NR = (int(v) for v in picks[1][0].split("<")[1].split(", ")[:3])
            want_K, _m, want_NR = (int(v) for v in c.symbol.split("<")[1].split(", ")[:3])
            assert (K, NR) == (want_K, want_NR), tag
        else:
            assert picks[0][0] == c.symbol, tag


def test_every_launch_leaves_three_workgroups_per_cu(cell_plans):
    """every dynamic-LDS request of every case x layout of every cell: within the 64 KiB no launch has to raise, and at
    least 3 workgroups of it fit the 160 KiB of a CU"""
    for (c, k, lens, sc), (_l, _w, _W, picks) in cell_plans:
        for name, lds in picks:
            if name != "-":
                assert 0 < lds <= 65536 and 160 * 1024 // lds >= 3, (c.symbol, k.S, lens, sc, name, lds)


def test_launch_sizes(exe):  # noqa: F811
    """The dynamic-LDS bytes of the launches, pinned: the decoders' table + staging per rung and W, the 41 KiB floor of
    the byte-output four-symbol decoder and of the short-code byte-input encoder from 16384 workgroup tasks on (3
    workgroups per CU; none for packed output / input), k_decode_rebin's row buffers."""
    wg, wave = kc.WG_LAYOUTS[0], kc.WAVE_LAYOUTS[0]
    R = kc.R

    def one(layout, S, L, input_bits=8, h=6):
        (_l, _w, W, picks), = planned(exe, [_line(layout[0], S, h, 1, R[(S, L)], layout[1], input_bits)])
        return W, dict(picks)

    for S, L, W_want in ((3, 2, 8), (2, 1, 4)):
        W, picks = one(wg, S, L)
        assert W == W_want and picks["mh::k_decode2<4, 4, 17, 1, false, 0>"] == 41984
    W, picks = one(wg, 3, 2)
    assert picks["mh::k_decode_range<4, 4, 17, 1, false>"] == 41984
    assert picks["mh::k_decode_rebin<4, 4, 17, 1, false, true>"] == 41984
    W, picks = one(wg, 3, 2, input_bits=2, h=0)
    assert W == 8 and picks["mh::k_decode2<4, 4, 17, 1, false, 2>"] == 23040
    W, picks = one(wg, 4, 3)
    assert W == 6 and picks["mh::k_decode2<2, 2, 25, 2, false, 0>"] == 29440
    W, picks = one(wg, 6, 5)
    assert W == 10 and picks["mh::k_decode2<2, 2, 32, 0, false, 0>"] == 37376
    assert picks["mh::k_decode_rebin<2, 2, 32, 0, false, true>"] == 42560
    W, picks = one(wg, 7, 6)
    assert W == 10 and picks["mh::k_decode2<2, 2, 31, 2, true, 0>"] == 37376
    W, picks = one(wave, 6, 5)
    assert picks["mh::k_decode2w<1, 2, 36, 2, false, true, 0>"] == 38912
    W, picks = one(wave, 3, 2)
    assert W == 8 and picks["mh::k_decode2w<4, 4, 17, 1, false, false, 0>"] == 30720
    # the encoder's floor: equal-length channels of four one-chunk segments are one workgroup task each
    for ntask, want in ((16383, 17920), (16384, 41984)):
        _W, picks = one(((4 * kc.CHUNK,) * ntask, 1), 3, 2)
        assert picks["mh::k_encode2<0, 3, 0>"] == want, ntask
        _W, picks = one(((4 * kc.CHUNK,) * ntask, 1), 3, 2, input_bits=2, h=0)
        assert picks["mh::k_encode2<0, 4, 2>"] == 17920, ntask
