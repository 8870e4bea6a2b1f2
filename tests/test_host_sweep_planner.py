"""The planner of mh_sweep_create (csrc/mh_sweep_planner.hpp: breakpoints, slots and histogram tiles of a sweep handle,
and csrc/mh_plan_arena.hpp's layout of them) as a host program under AddressSanitizer + UBSan, against a NumPy
restatement of include/muahuff.h's text: per channel the 2 * nh + 1 intervals between the SORTED breakpoints
0, c_h = min(2^h, T), min(c_h + T // 2, T) for every h, and T; each interval cut into tiles of 131072 samples.
Runs without a GPU."""
import os
import subprocess

import numpy as np

from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

TILE = 131072
LENS = [1, 5, 63, 64, 65, 131072, 131073, 300001]
BITS = [[6], [2, 6, 10], [6, 6], [30], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 17, 18, 30]]


def _run(exe_path, text):
    r = subprocess.run([exe_path, "--sweep"], input=text, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def _restated(lens, bits):
    """(bounds [C, ni + 1], slot lengths [C, ni], tiles [(channel, slot, start, n)])"""
    bounds = np.array([sorted([0, T] + [b for h in bits for b in (min(2 ** h, T), min(min(2 ** h, T) + T // 2, T))]) for T in lens],
                      dtype=np.uint64)
    ni = 2 * len(bits) + 1
    tiles = []
    for c in range(len(lens)):
        for j in range(ni):
            lo, hi = int(bounds[c, j]), int(bounds[c, j + 1])
            tiles += [(c, c * ni + j, first, min(TILE, hi - first)) for first in range(lo, hi, TILE)]
    return bounds, np.diff(bounds.astype(np.int64), axis=1), tiles


def test_sweep_layout_under_sanitizers_matches_the_header_text(exe):  # noqa: F811
    cases = [(LENS, b) for b in BITS] + [(LENS[::-1], [2, 6, 10])] + [([T], [6, 17]) for T in LENS]
    text = "\n".join("%d %d %s  %s" % (len(lens), len(b), " ".join(map(str, b)), " ".join(map(str, lens))) for lens, b in cases)
    lines = iter(_run(exe, text + "\n"))
    for lens, b in cases:
        bounds, slot_len, tiles = _restated(lens, b)
        C, ni = len(lens), 2 * len(b) + 1
        tag, got_ni, nt, t_bytes, s_bytes = next(lines).split()
        assert tag == "W" and int(got_ni) == ni and int(nt) == len(tiles), (lens, b)
        # six tables and one histogram of 16 64-bit counters per slot, each on a multiple of 256 bytes
        pad = lambda n: (max(n, 1) + 255) // 256 * 256    # noqa: E731
        assert int(t_bytes) == pad(8 * C) + 3 * pad(4 * len(tiles)) + pad(8 * len(tiles)) + pad(8 * C * ni)
        assert int(s_bytes) == pad(C * ni * 16 * 8)
        assert np.array_equal(np.array(next(lines).split()[1:], np.uint64).reshape(C, ni + 1), bounds)
        assert np.array_equal(np.array(next(lines).split()[1:], np.int64).reshape(C, ni), slot_len)
        got = [tuple(int(v) for v in next(lines).split()[1:]) for _ in tiles]
        assert got == tiles, (lens, b)
        assert slot_len.sum() == sum(lens) == sum(t[3] for t in tiles)     # the slots of a channel cover it once
    assert next(lines, None) is None
    # [6, 6] repeats every breakpoint: empty intervals, no tile for them
    _, slot_len, tiles = _restated(LENS, [6, 6])
    assert (slot_len == 0).any() and all(t[3] > 0 for t in tiles)


def test_sweep_planner_refuses_bad_arguments_under_sanitizers(exe):  # noqa: F811
    bad = ["2 0  5 6",                                   # nh = 0
           "2 17 " + " ".join(["6"] * 17) + "  5 6",     # nh = 17
           "2 2 6 31  5 6",                              # hist_bits = 31
           "3 1 6  5 0 6",                               # a channel without bins
           "0 1 6"]                                      # C = 0
    assert _run(exe, "\n".join(bad) + "\n") == ["error -1", "error -1", "error -1", "error -2", "error -1"]
