"""The receiving side of the stream path without a GPU: the C ABI of mh_decode_packed / mh_interleave_packed and the
set of packed-output decoder instances (k_decpk / k_decpkw) the shipped code object holds, each with the plans that
land on it according to the host planner.

Dispatch (dispatch_decode_packed, csrc/muahuff.hip) picks the output width from S -- 2 bits for S <= 4, 4 bits for
S >= 5 -- and then makes dispatch_decode's choice from maxlen L, the task form and the table width W.  S >= 5 needs a
codeword of at least 3 bits, S <= 4 has none longer than 3, so ten instances are reachable and nothing else is built."""
import os
import re
import subprocess

import pytest

from tests import kernel_cells as kc
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")

R53 = ((2, 2, 2, 3, 3),)   # S = 5 with maxlen 3: the shortest code a 4-bit plan can have


def _c(S, L, rows=None, **dec):
    return kc.Case(S, rows or kc.R[(S, L)], L, **dec)


class PackedCell:
    def __init__(self, symbol, wave, po, cases):
        self.symbol, self.wave, self.po, self.cases = symbol, wave, po, tuple(cases)
        self.layouts = kc.WAVE_LAYOUTS if wave else kc.WG_LAYOUTS


# (symbol, task form, output bits, cases with the planner's W / dec_K / dec_NR)
PACKED_CELLS = (
    # 2-bit pieces (S <= 4): the four-symbol table for L <= 2, the pair table for L = 3
    PackedCell("mh::k_decpk<4, 4, 17, 1, false, 2>", False, 2,
               [_c(3, 2, W=8, dec_K=4, dec_NR=32), _c(2, 1, W=4, dec_K=4, dec_NR=32), _c(4, 2, W=8, dec_K=4, dec_NR=32)]),
    PackedCell("mh::k_decpk<2, 2, 25, 2, false, 2>", False, 2, [_c(4, 3, W=6, dec_K=2, dec_NR=32)]),
    PackedCell("mh::k_decpkw<4, 4, 17, 1, false, false, 2>", True, 2,
               [_c(3, 2, W=8, dec_K=4, dec_NR=32), _c(2, 1, W=4, dec_K=4, dec_NR=32), _c(4, 2, W=8, dec_K=4, dec_NR=32)]),
    PackedCell("mh::k_decpkw<2, 2, 25, 2, false, false, 2>", True, 2, [_c(4, 3, W=6, dec_K=2, dec_NR=32)]),
    # 4-bit pieces (S >= 5)
    PackedCell("mh::k_decpk<2, 2, 25, 2, false, 4>", False, 4,
               [_c(5, 3, R53, W=6, dec_K=2, dec_NR=32), _c(8, 3, W=6, dec_K=2, dec_NR=32)]),
    PackedCell("mh::k_decpk<2, 2, 32, 0, false, 4>", False, 4,      # L = 5 is the last with W = 2L
               [_c(5, 4, W=8, dec_K=2, dec_NR=32), _c(9, 4, W=8, dec_K=2, dec_NR=32), _c(6, 5, W=10, dec_K=2, dec_NR=32)]),
    PackedCell("mh::k_decpk<2, 2, 31, 2, true, 4>", False, 4,       # hybrid pair table from L = 6
               [_c(7, 6, W=10, dec_K=2, dec_NR=31), _c(10, 9, W=10, dec_K=2, dec_NR=31)]),
    PackedCell("mh::k_decpkw<2, 2, 25, 2, false, false, 4>", True, 4,
               [_c(5, 3, R53, W=6, dec_K=2, dec_NR=32), _c(8, 3, W=6, dec_K=2, dec_NR=32)]),
    PackedCell("mh::k_decpkw<2, 2, 32, 0, false, false, 4>", True, 4,  # L = 4 is the last with W = 2L
               [_c(5, 4, W=8, dec_K=2, dec_NR=32), _c(10, 4, W=8, dec_K=2, dec_NR=32)]),
    PackedCell("mh::k_decpkw<1, 2, 36, 2, false, true, 4>", True, 4,   # one-symbol pairs from L = 5
               [_c(6, 5, W=8, dec_K=2, dec_NR=31), _c(10, 9, W=9, dec_K=2, dec_NR=31)]),
)


def _code_object_symbols(tmp_path, pattern):
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
    mangled = sorted({ln.split()[-1] for ln in table.splitlines() if " F " in ln and re.search(pattern, ln)})
    if not mangled:
        return set()
    names = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", check=True, capture_output=True,
                           text=True).stdout.split("\n")[:len(mangled)]
    return {n.strip() for n in names}


def test_header_declares_the_receive_side_with_the_binding_prototypes():
    from muahuff import _lib
    hdr = open(os.path.join(ROOT, "include", "muahuff.h")).read()
    ctype = {"mh_plan*": "p", "constuint32_t*": "p", "constuint64_t*": "p", "constuint8_t*": "p", "uint8_t*": "p",
             "void*": "p", "uint64_t": "u64", "uint32_t": "u32"}
    py = {_lib.ct.c_void_p: "p", _lib.ct.c_uint64: "u64", _lib.ct.c_uint32: "u32"}
    for name in ("mh_decode_packed", "mh_interleave_packed"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\);" % name, hdr)
        assert m, name + " is not declared in include/muahuff.h"
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        kinds = []
        for a in args:
            kinds.append(ctype[re.match(r"(.*?[\s*])\w+$", a).group(1).replace(" ", "")])
        assert name in _lib.PROTOTYPES
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is _lib.ct.c_int
        assert [py[a] for a in argtypes] == kinds, (name, kinds)


def test_shipped_packed_decoders_are_exactly_the_cells(tmp_path):
    shipped = _code_object_symbols(tmp_path, r"k_decpk")
    want = {"void %s(mh::DecPkArgs)" % c.symbol for c in PACKED_CELLS}
    assert len(want) == len(PACKED_CELLS) == 10
    assert shipped == want, dict(without_cell=sorted(shipped - want), not_shipped=sorted(want - shipped))
    for name in shipped:                 # tests/test_host_kernel_cells.py counts k_(en|de)code2 symbols: not these
        assert not re.search(r"k_(en|de)code2", name), name
    assert _code_object_symbols(tmp_path, r"k_interleave_p") == {
        "void mh::k_interleave_p<%d>(unsigned char const*, unsigned long const*, unsigned long, unsigned int, "
        "unsigned int, unsigned long, unsigned int, unsigned char*)" % b for b in (2, 4)}


def _dispatch(po, wave, L, W):
    """dispatch_decode_packed (csrc/muahuff.hip) in Python: the instance a packed plan launches"""
    if po == 2:
        if wave:
            return "mh::k_decpkw<4, 4, 17, 1, false, false, 2>" if L <= 2 else "mh::k_decpkw<2, 2, 25, 2, false, false, 2>"
        return "mh::k_decpk<4, 4, 17, 1, false, 2>" if L <= 2 else "mh::k_decpk<2, 2, 25, 2, false, 2>"
    if wave:
        if L == 3:
            return "mh::k_decpkw<2, 2, 25, 2, false, false, 4>"
        return "mh::k_decpkw<2, 2, 32, 0, false, false, 4>" if W >= 2 * L else "mh::k_decpkw<1, 2, 36, 2, false, true, 4>"
    if L == 3:
        return "mh::k_decpk<2, 2, 25, 2, false, 4>"
    return "mh::k_decpk<2, 2, 32, 0, false, 4>" if W >= 2 * L else "mh::k_decpk<2, 2, 31, 2, true, 4>"


def test_every_packed_cell_lands_where_the_table_says(exe):  # noqa: F811
    """Each case x layout of each cell through the host planner with the cell's packed input_bits (planner_check
    --cells): maxlen, task form, W, dec_K, dec_NR, and the instance dispatch picks from them."""
    lines, want = [], []
    for c in PACKED_CELLS:
        for k in c.cases:
            assert (2 if k.S <= 4 else 4) == c.po, (c.symbol, k.S)
            for lens, sc in c.layouts:
                rows = " ".join(str(v) for r in k.rows for v in r)
                lines.append("%d %d 0 1 3 %d %d %d  %s  %s" % (len(lens), k.S, len(k.rows), sc, c.po,
                                                              " ".join(map(str, lens)), rows))
                want.append((c, k, lens, sc))
    r = subprocess.run([exe, "--cells"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, (c, k, lens, sc) in zip(got, want):
        maxlen, wave, W, dec_K, dec_NR = (int(v) for v in g.split())
        tag = (c.symbol, k.S, k.rows, lens, sc)
        assert maxlen == k.maxlen and wave == int(c.wave), tag
        assert (W, dec_K, dec_NR) == (k.W, k.dec_K, k.dec_NR), tag
        assert _dispatch(c.po, bool(wave), maxlen, W) == c.symbol, tag


def test_every_reachable_packed_plan_has_a_cell(exe):  # noqa: F811
    """All SCLV tables of S = 2..10 (every row and the whole table), both task forms: the instance dispatch picks is
    one of the cells -- a plan that could reach an unbuilt instance fails here."""
    from tests import helpers
    symbols = {c.symbol for c in PACKED_CELLS}
    tabs = helpers.sclv_tables()
    lines, meta = [], []
    for S in range(2, 11):
        po = 2 if S <= 4 else 4
        for rows in [[r] for r in tabs[S]] + [list(tabs[S])]:
            for lens, sc in (kc.WAVE_LAYOUTS[0], kc.WG_LAYOUTS[0]):
                flat = " ".join(str(int(v)) for r in rows for v in r)
                lines.append("%d %d 0 1 3 %d %d %d  %s  %s" % (len(lens), S, len(rows), sc, po, " ".join(map(str, lens)), flat))
                meta.append((S, po))
    r = subprocess.run([exe, "--cells"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = set()
    for g, (S, po) in zip(r.stdout.splitlines(), meta):
        maxlen, wave, W, _k, _nr = (int(v) for v in g.split())
        sym = _dispatch(po, bool(wave), maxlen, W)
        assert sym in symbols, (S, maxlen, wave, W)
        seen.add(sym)
    assert len(seen) >= 8
