"""mh_measure on packed plans, the part that needs no GPU: the header documents it, the NULL check is still in front,
and the feature added no exported function (tests/async_table.py still names every symbol)."""
import os
import re
import subprocess

from muahuff import _lib
from tests import async_table as at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "muahuff.h")).read()


def _comment_before(hdr, decl):
    """the block comment that ends right in front of `decl`"""
    end = hdr.index(decl)
    start = hdr.rindex("/*", 0, end)
    return " ".join(hdr[start:end].split())


def test_header_documents_measure_on_packed_plans():
    hdr = _header()
    packed = _comment_before(hdr, "int mh_plan_create_packed(")
    measure = _comment_before(hdr, "int mh_measure(")
    assert "only mh_encode_preset reads" not in packed
    assert not re.search(r"mh_measure,\s*mh_encode\s+and\s+mh_decode return MH_ERR_ARG", packed)
    assert "mh_measure" in packed and "mh_encode and mh_decode return MH_ERR_ARG" in packed
    assert "packed plan" in measure.lower() and "mh_deinterleave_packed" in measure
    assert "#define MH_VERSION 103 " in hdr
    additions = hdr[hdr.index("Additions within 0.1.3"):hdr.index("/* ---- error codes")]
    assert re.search(r"mh_measure\s+-- .*packed", additions)


def test_measure_null_plan_is_still_an_argument_error():
    L = _lib.lib()
    assert L.mh_measure(None, None, None, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert b"mh_measure" in L.mh_last_error()


def test_symbol_set_is_unchanged():
    assert len(at.CLASS) == 34
    assert set(_lib.PROTOTYPES) == set(at.CLASS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO], check=True, capture_output=True, text=True).stdout
    exported = sorted(line.split()[-1] for line in nm.splitlines() if line.strip())
    assert exported == sorted(at.CLASS), sorted(set(exported) ^ set(at.CLASS))
    assert at.CLASS["mh_measure"] == at.CAPTURABLE
