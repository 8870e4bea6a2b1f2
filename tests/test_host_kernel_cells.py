"""The table of codec kernel cells (tests/kernel_cells.py) against the shipped code object and the host planner.
Runs without a GPU: a kernel instance added to libmuahuff.so fails here until it gets a cell, a cell whose kernel
is no longer shipped fails as well, and a cell whose plans no longer land on its kernel fails before any GPU run."""
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


def test_every_cell_lands_where_the_table_says(exe):  # noqa: F811
    """Each case x layout of each cell through the host planner (--cells): maxlen and the task form; decoder cells
    also W, dec_K, dec_NR and the instance dispatch_decode picks from them.  Packed decoder cells are planned as
    StreamDecoder plans its blocks, without a calibration window (h = 0)."""
    lines, want = [], []
    for c in kc.CELLS:
        for k in c.cases:
            for lens, sc in c.layouts:
                rows = " ".join(str(v) for r in k.rows for v in r)
                h = 0 if c in kc.PACKED_DECODER_CELLS else 6
                lines.append("%d %d %d %d 3 %d %d %d  %s  %s" % (len(lens), k.S, h, c.mode, len(k.rows), sc, c.input_bits,
                                                                " ".join(map(str, lens)), rows))
                want.append((c, k, lens, sc))
    r = subprocess.run([exe, "--cells"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, (c, k, lens, sc) in zip(got, want):
        maxlen, wave, W, dec_K, dec_NR = (int(v) for v in g.split())
        tag = (c.symbol, k.S, k.rows, lens, sc)
        assert maxlen == k.maxlen, tag
        assert wave == int(c.wave), tag
        if c.decoder:
            assert (W, dec_K, dec_NR) == (k.W, k.dec_K, k.dec_NR), tag
            po = 0 if c.input_bits == 8 else c.input_bits
            assert kc.decoder_symbol(po, c.wave, maxlen, W) == c.symbol, tag
