"""The build recipe without a GPU and without a compiler: the header lists that decide whether a library is stale are what
its source reaches through #include "...", and touching a header marks the libraries that reach it and no others."""
import importlib
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hardware-efficient-mua-compression_amd"
build = importlib.import_module(PKG + ".build")
NAMES = ["muahuff"] + ["muahuff_" + n for n in ("ingest", "wiener", "cascade", "smooth", "sweep", "kalman", "lstm")]


def _closure(source):
    """every #include "..." target below `source`, as paths relative to the package directory: a walk of its own"""
    here = os.path.join(ROOT, PKG)
    seen, stack = set(), [source]
    while stack:
        f = stack.pop()
        for inc in re.findall(r'#\s*include\s*"([^"]+)"', open(os.path.join(here, f)).read()):
            tried = [os.path.normpath(os.path.join(d, inc)) for d in (os.path.dirname(f), "csrc", "../include")]
            hit = [p for p in tried if os.path.exists(os.path.join(here, p))]
            assert hit, inc
            if hit[0] not in seen:
                seen.add(hit[0])
                stack.append(hit[0])
    return seen


def test_every_header_list_is_what_the_source_reaches():
    assert [row[0] for row in build.LIBRARIES] == NAMES
    lists = [build.HEADERS, build.INGEST_HEADERS, build.WIENER_HEADERS, build.CASCADE_HEADERS, build.SMOOTH_HEADERS,
             build.SWEEP_HEADERS, build.KALMAN_HEADERS, build.LSTM_HEADERS]
    for (name, source, exports, public), listed in zip(build.LIBRARIES, lists):
        assert listed == build.headers(name) and len(set(listed)) == len(listed)
        assert _closure(source) | {exports, public} == set(listed), name
        assert "csrc/mh_abi.hpp" in listed and "csrc/mh_msg.hpp" in listed and "../include/muahuff.h" in listed
        for f in [source] + listed:
            assert os.path.isfile(os.path.join(ROOT, PKG, f)), f
    assert "csrc/mh_rows.hpp" in build.KALMAN_HEADERS and "csrc/mh_rows.hpp" not in build.HEADERS


def test_touching_a_header_marks_the_libraries_that_reach_it_and_no_others(tmp_path, monkeypatch):
    pkg = tmp_path / PKG
    shutil.copytree(os.path.join(ROOT, PKG, "csrc"), pkg / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    for d in (pkg / "csrc", tmp_path / "include"):
        for f in d.iterdir():
            os.utime(f, (1000, 1000))
    monkeypatch.setattr(build, "HERE", str(pkg))
    monkeypatch.setattr(build.subprocess, "check_call", lambda *a, **k: pytest.fail("the staleness test compiles nothing"))
    assert all(build.stale(n) for n in NAMES)                     # no library yet
    for n in NAMES:
        (pkg / ("lib%s.so" % n)).write_bytes(b"")
        os.utime(pkg / ("lib%s.so" % n), (2000, 2000))
    assert not any(build.stale(n) for n in NAMES) and not build.stale()
    assert build.build_kalman() == str(pkg / "libmuahuff_kalman.so")  # fresh: returned as it is
    companions = set(NAMES[1:])
    for header, reach in (("csrc/mh_msg.hpp", set(NAMES)), ("csrc/mh_rows.hpp", companions),
                          ("csrc/mh_kalman_layout.hpp", {"muahuff_kalman"}),
                          ("csrc/mh_wiener_layout.hpp", {"muahuff_wiener", "muahuff_sweep"}),
                          ("csrc/mh_gram_layout.hpp", {"muahuff_ingest", "muahuff_sweep"}),
                          ("csrc/exports_lstm.map", {"muahuff_lstm"}), ("../include/muahuff_smooth.h", {"muahuff_smooth"}),
                          ("csrc/mh_cascade.hip", {"muahuff_cascade"})):
        os.utime(pkg / header, (3000, 3000))
        assert {n for n in NAMES if build.stale(n)} == reach, header
        assert reach == {row[0] for row in build.LIBRARIES if header in _closure(row[1]) | set(row[1:])}, header
        os.utime(pkg / header, (1000, 1000))
    assert not any(build.stale(n) for n in NAMES)
