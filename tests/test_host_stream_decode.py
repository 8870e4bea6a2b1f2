"""The receiving side of the stream path without a GPU: the C ABI of mh_decode_packed / mh_interleave_packed, the
k_interleave_p instances, and that every plan mh_decode_packed accepts lands on a shipped decoder.  The packed
decoders themselves are cells of tests/kernel_cells.py (k_decode2 / k_decode2w with PO = 2 / 4), pinned and placed
with the others by tests/test_host_kernel_cells.py.

mh_decode_packed picks the output width from S -- 2 bits for S <= 4, 4 bits for S >= 5 -- and then makes
mh_decode's choice (dec_pick, csrc/mh_select.hpp) from maxlen L, the task form and the table width W.  S >= 5 needs a codeword of
at least 3 bits, S <= 4 has none longer than 3, so ten instances are reachable and nothing else is built."""
import os
import re

from tests import kernel_cells as kc
from tests.test_host_kernel_cells import code_object_symbols, planned
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_shipped_packed_interleavers(tmp_path):
    assert code_object_symbols(tmp_path, r"k_interleave_p") == {
        "void mh::k_interleave_p<%d>(unsigned char const*, unsigned long const*, unsigned long, unsigned int, "
        "unsigned int, unsigned long, unsigned int, unsigned char*)" % b for b in (2, 4)}


def test_every_reachable_packed_plan_has_a_cell(exe):  # noqa: F811
    """All SCLV tables of S = 2..10 (every row and the whole table), both task forms: the instance the library's
    selection names (planner_check --cells) is one of the cells -- a plan that could reach an unbuilt instance fails
    here."""
    from tests import helpers
    symbols = {c.symbol for c in kc.PACKED_DECODER_CELLS}
    tabs = helpers.sclv_tables()
    lines, meta = [], []
    for S in range(2, 11):
        po = 2 if S <= 4 else 4
        for rows in [[r] for r in tabs[S]] + [list(tabs[S])]:
            for lens, sc in (kc.WAVE_LAYOUTS[0], kc.WG_LAYOUTS[0]):
                flat = " ".join(str(int(v)) for r in rows for v in r)
                lines.append("%d %d 0 1 3 %d %d %d  %s  %s" % (len(lens), S, len(rows), sc, po, " ".join(map(str, lens)), flat))
                meta.append((S, po))
    seen = set()
    for (maxlen, wave, W, picks), (S, po) in zip(planned(exe, lines), meta):
        sym = picks[1][0]
        assert sym in symbols, (S, maxlen, wave, W)
        seen.add(sym)
    assert len(seen) >= 8
