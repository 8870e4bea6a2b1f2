"""The capped launch grids of the two libraries (csrc/mh_launch.hpp: what muahuff.hip and mh_ingest.hip launch) read back
off-device: planner_check --geometry prints the grid and the derived kernel arguments of one launch per line, under
AddressSanitizer + UBSan, and every rule is restated here in Python -- at the shapes tests/test_gpu_launch_caps.py,
tests/test_gpu_bin_events_spans.py, tests/test_gpu_checksum.py and tests/test_gpu_ingest_trips.py run on the device, and at the edges of each cap.
DESIGN.md ("Capped launch grids") is the table of the rules.  Runs without a GPU."""
import os
import subprocess

from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

YMAX, XMAX = 65535, 2 ** 31 - 1
C_BIG = 2 * YMAX + 3
ERR_ARG = -1


def _ceil(a, b):
    return -(-a // b)


def _clamp(n, cap):
    return max(1, min(n, cap))


def _run(exe_path, lines):
    r = subprocess.run([exe_path, "--geometry"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


def _ints(rec, name):
    assert rec[0] == name and rec[1] != "error", rec
    return [int(v) for v in rec[1:]]


def _refused(rec, name, word):
    assert rec[:3] == [name, "error", str(ERR_ARG)] and word in " ".join(rec[3:]), rec


# ---- mh_rebin ------------------------------------------------------------------------------------------------------
def _rebin(max_len, C, r):
    y = min(C, YMAX)                                     # one grid row per channel, ch += gridDim.y
    if r < 4:                                            # k_rebin2: tiles of 32768 // r bins, at most 4096 of them in x
        return [_clamp(_ceil(_ceil(max_len, r), 32768 // r), 4096), y]
    g = 1 if r % 4 == 0 else 2 if r % 2 == 0 else 4      # k_rebin3: units of g bins = u dwords
    u = g * r // 4
    upt = 8192 // u                                      # units of a tile of at most 32 KiB ...
    if upt >= 256:
        upt -= upt % 256                                 # ... in whole passes of 256 threads
    return [_clamp(_ceil(_ceil(max_len, upt * u * 4), 4), YMAX), y, g, u, upt, 4]


def _long_len(r):                                        # test_gpu_launch_caps.py: 4096 + 2 tiles of k_rebin2
    return ((4096 + 1) * (32768 // r) + (32768 // r) // 3) * r + 16


def test_rebin_grids(exe):  # noqa: F811
    shapes = [(300, C_BIG, r) for r in (2, 3, 5, 7, 100)] + [(_long_len(3), 3, 3), (_long_len(1), 3, 1)]
    shapes += [(32768 * 4096, 1, 1), (32768 * 4096 + 1, 1, 1), (0, 1, 2), (1, YMAX, 3), (1, YMAX + 1, 3)]      # x and y caps of k_rebin2
    shapes += [(4 * 32768 * YMAX, 1, 4), (4 * 32768 * YMAX + 1, 1, 4), (10 ** 7, 1024, 4096), (10 ** 7, 1024, 6), (0, 5, 4)]
    got = _run(exe, ["rebin %d %d %d" % s for s in shapes])
    for s, rec in zip(shapes, got):
        assert _ints(rec, "rebin") == _rebin(*s), s
    assert _ints(got[0], "rebin")[1] == YMAX and _ints(got[5], "rebin")[0] == 4096 < _ceil(_ceil(_long_len(3), 3), 32768 // 3)
    assert [_ints(got[i], "rebin")[0] for i in (7, 8, 12, 13)] == [4096, 4096, YMAX, YMAX]


# ---- mh_synth_poisson ----------------------------------------------------------------------------------------------
def test_synth_grids(exe):  # noqa: F811
    shapes = [(4096 * 4096 + 5 * 4096 + 7, 6), (40, C_BIG), (4096 * 4096, 1), (4096 * 4095 + 1, 1), (4096 * 4095, 1), (0, 1), (1, YMAX)]
    got = _run(exe, ["synth %d %d" % s for s in shapes])
    for (max_len, C), rec in zip(shapes, got):
        assert _ints(rec, "synth") == [_clamp(_ceil(max_len, 256 * 16), 4096), min(C, YMAX)], (max_len, C)
    assert [_ints(r, "synth")[0] for r in got[:5]] == [4096, 1, 4096, 4096, 4095]


# ---- the zero fills of mh_decode_range / mh_decode_rebin -------------------------------------------------------------
def test_fill_grids(exe):  # noqa: F811
    range_stop = 1024 * 16384 + 3 * 4096 + 5             # test_gpu_launch_caps.py: RANGE_STOP, REBIN_STOP / REBIN_R
    shapes = [(512, 256 * 16 * 4, 2 * YMAX + 2), (range_stop - 100, 256 * 16 * 4, 3), (1024 * 4096 + 3 * 256 + 5 - 25, 256 * 16, 3),
              (1024 * 4096, 4096, YMAX), (1024 * 4096 + 1, 4096, YMAX + 1), (0, 4096, 1), (77, 4096, 0)]
    got = _run(exe, ["fills %d %d %d" % s for s in shapes])
    for (max_fill, per_block, nfill), rec in zip(shapes, got):
        launches = [min(YMAX, nfill - f) for f in range(0, nfill, YMAX)]          # the next launch takes the next 65535 records
        assert _ints(rec, "fills") == [_clamp(_ceil(max_fill, per_block), 1024)] + launches, (max_fill, per_block, nfill)
    assert _ints(got[0], "fills") == [1, YMAX, YMAX, 2] and _ints(got[1], "fills")[0] == 1024 and _ints(got[6], "fills") == [1]


# ---- the four transposing calls --------------------------------------------------------------------------------------
def test_transposed_grids(exe):  # noqa: F811
    def grid(T, C, tpw):
        strips = _ceil(C, 128)
        return min(_ceil(_ceil(T, 256), tpw), XMAX // strips) * strips     # strips x visits in one dimension, the visits capped

    shapes = [(1, YMAX * 128, 4), (1, 1, 4), (10 ** 7, 1024, 4), (10 ** 7, 1024, 2), (256 * 4 * 40000, YMAX * 128, 4),
              (2 ** 64 - 1, 1, 2), (256 * 4 * XMAX, 1, 4), (256 * 4 * XMAX + 1, 1, 4), (0, 128, 4)]
    got = _run(exe, ["transposed %d %d %d" % s for s in shapes + [(1, YMAX * 128 + 1, 4), (10 ** 7, 2 ** 32 - 1, 2)]])
    for s, rec in zip(shapes, got):
        assert _ints(rec, "transposed") == [grid(*s)], s
    assert _ints(got[0], "transposed") == [YMAX]                         # 65535 strips are accepted ...
    _refused(got[-2], "transposed", "too large")                        # ... 65536 are not
    _refused(got[-1], "transposed", "too large")
    assert _ints(got[4], "transposed") == [(XMAX // YMAX) * YMAX] and 40000 > XMAX // YMAX     # the visits are capped
    assert [_ints(got[i], "transposed")[0] for i in (5, 6, 7)] == [XMAX] * 3                  # clamped to 2^31 - 1


# ---- mh_power_draws, mh_reduce_rows; mh_compact ------------------------------------------------------------------------
def test_per_item_and_compact_grids(exe):  # noqa: F811
    ns = [1, 256, 257, XMAX * 256]
    got = _run(exe, ["items %d" % n for n in ns + [XMAX * 256 + 1, 2 ** 64 - 1]])
    for n, rec in zip(ns, got):
        assert _ints(rec, "items") == [_ceil(n, 256)]
    _refused(got[-2], "items", "too many items for one launch")
    _refused(got[-1], "items", "too many")
    nsegs = [0, 1, 4, 5, 2048, 2049, 4096, 4097, 0xFFFFFFF0]
    for nseg, rec in zip(nsegs, _run(exe, ["compact %d" % n for n in nsegs])):
        blocks = _ceil(nseg, 2048)                       # up to one block of 2048 segments every wave scans for itself
        assert _ints(rec, "compact") == [int(blocks <= 1), blocks, max(1, _ceil(nseg, 4))], nseg


# ---- mhi_bin_events ----------------------------------------------------------------------------------------------------
def _bin(C, T, period):
    nch = _ceil(T, 16384)

    def groups(span):
        return C * _ceil(nch, span)
    # 8 chunks per workgroup, fewer (down to 1) while that leaves less than 4096 workgroups ...
    span = next((s for s in (8, 4, 2, 1) if groups(s) >= 4096), 1)
    if groups(span) > XMAX:                              # ... more when C x spans does not fit one grid dimension
        span = min(2 ** k for k in range(4, 64) if groups(2 ** k) <= XMAX)
    return [groups(span), nch, span, _ceil(nch, span), 0 if period == 1 else 1 if period < 2 ** 18 else 2]


def test_bin_events_spans_and_division(exe):  # noqa: F811
    CH = 16384
    shapes = [(1, 8 * 4096 * CH, 1), (1, (8 * 4096 - 8) * CH, 1), (1, (8 * 4096 - 8) * CH + 1, 1),     # span 8 | 4 | 8
              (1, (4 * 4096 - 4) * CH, 2), (1, (2 * 4096 - 2) * CH - CH + 1, 2 ** 18 - 1), (3, 10 * CH, 2 ** 18), (4096, 1, 2 ** 40),
              (4095, 1, 7), (4095, CH + 1, 7), (512, 8 * 8 * CH, 1), (512, (8 * 8 - 1) * CH, 1),
              (XMAX, 8 * CH, 1), (XMAX, 8 * CH + 1, 1), (65536, 8 * 32768 * CH, 1), (65536, (8 * 32768 - 8) * CH, 1),
              (65536, 8 * 32768 * CH * 5, 1), (XMAX, 2 ** 45, 3)]
    got = _run(exe, ["bin_events %d %d %d" % s for s in shapes + [(2 ** 31, 1, 1), (2 ** 32 - 1, 10 ** 9, 1)]])
    for s, rec in zip(shapes, got):
        assert _ints(rec, "bin_events") == _bin(*s), s
        assert 1 <= _ints(rec, "bin_events")[0] <= XMAX
    spans = [_ints(rec, "bin_events")[2] for rec in got[:len(shapes)]]
    assert spans[:6] == [8, 4, 8, 2, 1, 1] and {1, 2, 4, 8, 16} <= set(spans) and max(spans) > 16
    assert [_ints(rec, "bin_events")[4] for rec in got[3:6]] == [1, 1, 2] and _ints(got[0], "bin_events")[4] == 0
    # both sides of 4096 and of 2^31 - 1 workgroups at eight chunks each
    assert _bin(*shapes[0])[0] == 4096 and 8 * 4096 - 8 == 8 * 4095
    assert _bin(*shapes[11])[:3] == [XMAX, 8, 8] and _bin(*shapes[12])[:3] == [XMAX, 9, 16]
    assert _bin(*shapes[13])[2] == 16 and _bin(*shapes[14])[2] == 8
    # more channels than one grid dimension holds fit at no span
    _refused(got[-2], "bin_events", "C=2147483648")
    _refused(got[-1], "bin_events", "C=4294967295")


# ---- mhi_excess_apply --------------------------------------------------------------------------------------------------
def test_excess_apply_grids(exe):  # noqa: F811
    # r == 1 (k_excess_apply1): x = at most 64 workgroups of 256 threads over the LIST's entries, y = one grid row per
    # output row up to 65535.  Both sides of each cap, and the shapes of tests/test_gpu_ingest_trips.py
    ones = [(1, 1), (256, 1), (257, 1), (63 * 256, 7), (64 * 256, 7), (64 * 256 + 1, 7), (65 * 256, 7), (1000, YMAX - 1), (1000, YMAX),
            (1000, YMAX + 1), (12000, C_BIG), (90000, 3), (2 ** 40, 2 ** 40), (2 ** 64 - 1, 2 ** 64 - 1)]
    got = _run(exe, ["excess_apply1 %d %d" % s for s in ones])
    for (n_entries, n_rows), rec in zip(ones, got):
        assert _ints(rec, "excess_apply1") == [min(_ceil(n_entries, 256), 64), min(n_rows, YMAX)], (n_entries, n_rows)
    assert [_ints(r, "excess_apply1")[0] for r in got[:7]] == [1, 1, 2, 63, 64, 64, 64]
    assert [_ints(r, "excess_apply1")[1] for r in got[7:11]] == [YMAX - 1, YMAX, YMAX, YMAX]
    # r > 1 (k_excess_apply): a thread per run of 32 elements of a row, at most 2^20 workgroups of 256 threads
    cap = 2 ** 20
    jobs = [(1, 1), (3, 625), (256, 1), (257, 1), (cap * 256 - 1, 1), (cap * 256, 1), (cap * 256 + 1, 1), (cap, 256), (cap + 1, 256),
            (2 ** 28 + 1000, 1), (2 ** 31, 2 ** 31), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)]
    got = _run(exe, ["excess_apply %d %d" % s for s in jobs])
    for (n_rows, runs), rec in zip(jobs, got):
        assert _ints(rec, "excess_apply") == [min(_ceil(n_rows * runs, 256), cap)], (n_rows, runs)
    assert [_ints(r, "excess_apply")[0] for r in got[:10]] == [1, 8, 1, 2, cap, cap, cap, cap, cap, cap]
    assert _ceil(cap * 256 - 1, 256) == cap and _ceil((cap - 1) * 256 + 1, 256) == cap
    assert _ints(_run(exe, ["excess_apply %d 1" % ((cap - 1) * 256)])[0], "excess_apply") == [cap - 1]


# ---- mhi_seg_crc32, the chunk-stride rule ------------------------------------------------------------------------------
def test_seg_crc32_grid_and_chunk_stride_rule(exe):  # noqa: F811
    ns = [1, 4, 5, 2047 * 4, 2048 * 4 - 3, 2048 * 4, 2048 * 4 + 1, 2049 * 4, 3 * 8192 + 5, 2 ** 64 - 1]
    got = _run(exe, ["seg_crc32 %d" % n for n in ns])
    for n, rec in zip(ns, got):
        assert _ints(rec, "seg_crc32") == [min(_ceil(n, 4), 2048)], n        # workgroups of 4 segments, at most 2048
    assert [_ints(r, "seg_crc32")[0] for r in got[3:8]] == [2047, 2048, 2048, 2048, 2048]
    strides = [(0, 8), (0, 2), (4096, 8), (4096, 2), (4096 + 8, 2), (4096 + 16, 2), (2048, 2), (4096, 4), (8192, 4), (2 ** 64 - 16, 4)]
    for (stride, bits), rec in zip(strides, _run(exe, ["chunk_stride %d %d" % s for s in strides])):
        ok = stride == 0 or (bits != 8 and stride % 16 == 0 and stride >= 16384 * bits // 8)      # include/muahuff.h
        assert _ints(rec, "chunk_stride") == [int(ok)], (stride, bits)
