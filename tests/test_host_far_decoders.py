"""The table of tests/far_decoders.py without a GPU.  For every case:

  (a) the terms that CROSSING names for it -- stated here, case by case, so that a later edit cannot shrink a case into
      irrelevance -- are the terms that cross 2^32: every access through such an argument is formed by a term that, cut
      modulo 2^32, lands elsewhere, and at least one of them lies past 2^32;
  (b) every address the call can form lies inside the arena and inside a window that the GPU test compares whole: with every
      term in full, and again with each term cut modulo 2^32 (the stride, the index * stride product, the product scaled to
      bytes) singly, and the whole sum cut.  A kernel that narrows any of them therefore cannot fault;
  (c) a far input and each of its aliases differ before the call; a far output is changed by the call and its alias is
      another address; every true region is disjoint from its aliases;
  (d) the layout meets the entry point's own argument rules, and the decoys give another result (each Setup lists them).

Then the table as a whole -- every entry point listed in DESIGN.md has its far values, its far products and its far column
-- the shapes of the five whole-length cases, and the argument rules about strides the cases rely on, through the check
programs of the five host tests (tests/*_check.cpp, the layout headers built alone under AddressSanitizer + UBSan): two rows
2^48 - 8 bytes apart are accepted everywhere; 2^48 is refused where the header says so (muahuff_smooth.h,
muahuff_kalman.h).  muahuff_wiener.h, muahuff_cascade.h and muahuff_sweep.h document no upper bound on a stride, and their
check functions have none: with at most 65536 rows any stride below 2^48 keeps every product inside 64 bits."""
import os
import re

import numpy as np
import pytest

from tests import far_decoders as fd
from tests import far_offsets as fo

IDS = [c.id for c in fd.CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The arguments whose terms cross 2^32, case by case.  A stride case crosses through the argument it is named after (in
# place: through both, which are one stride); a far-column case through the ranges, on every operand that is indexed by
# the column in elements wider than a byte.
CROSSING = {}
for _row, _args in (("xty", ("x_row_stride", "y_row_stride")), ("fir", ("x_row_stride", "out_row_stride")),
                    ("moments", ("p_row_stride", "y_row_stride")), ("box_f32", ("in_row_stride", "out_row_stride")),
                    ("xty_clips", ("x_row_stride", "y_row_stride")), ("project", ("x_row_stride", "v_row_stride"))):
    for _k in ("value", "product"):
        for _a in _args:
            CROSSING["%s-%s-%s" % (_row, _a, _k)] = {_a}
for _row, _args in (("polyval", ("p_row_stride", "out_row_stride")), ("scan", ("v_row_stride", "out_row_stride"))):
    for _k in ("value", "product"):
        for _a in _args:
            CROSSING["%s-%s-%s" % (_row, _a, _k)] = {_a}
        CROSSING["%s-in place-%s" % (_row, _k)] = set(_args)
CROSSING.update({"box-x_row_stride": {"x_row_stride"}, "box-out_row_stride": {"out_row_stride (lo)", "out_row_stride (hi)"},
                 "gram_clips": {"x_row_stride"}, "moments": {"ranges (p)", "ranges (y)"}, "xty_clips": {"ranges (y)"},
                 "scan-1": {"ranges (v)", "ranges (out)"}, "scan2-2": {"ranges (v)", "ranges (out)"}})


@pytest.fixture(scope="module")
def setups():
    return {}


def _setup(setups, case):
    if case.id not in setups:
        setups[case.id] = case.setup()
    return setups[case.id]


def _size(case):
    return fo.ARENA_BYTES if case.arena == "A" else fd.ARENA2_BYTES


def test_the_arena_is_the_one_of_far_offsets():
    assert fo.ARENA_BYTES == 2 ** 32 + 2 ** 28 and fd.ARENA_F32 * 4 == fd.ARENA_F64 * 8 == fo.ARENA_BYTES and fo.SLACK < 2 ** 31
    assert fd.ARENA2_BYTES == 2 * fo.ARENA_BYTES
    assert fd.Image is fo.Image and fd.Access is fo.Access and fd.Term is fo.Term and fd.Setup is fo.Setup      # imported, not copied
    # the extras of the far strides are longer than any row, so the alias of the last row lies behind row 0
    longest = max(a.nbytes for c in fd.CASES if c.kind in ("value", "product") for a in c.setup().accesses)
    assert longest < min(fd.EX1, fd.EX4, fd.EX8, fd.EX16) and fd.EX1 % 2 == 1 and fd.EX4 % 4 == 0 and fd.EX8 % 8 == 0 and fd.EX16 % 16 == 0


def test_ids_are_unique_and_every_case_states_what_crosses():
    assert len(set(IDS)) == len(IDS)
    assert set(CROSSING) == set(IDS), set(CROSSING) ^ set(IDS)


@pytest.mark.parametrize("case", fd.CASES, ids=IDS)
def test_a_the_stated_terms_cross(setups, case):
    s = _setup(setups, case)
    assert s.pre.size == _size(case) and s.crossing, case.id
    for what, value, unit in s.crossing:
        assert unit == "bytes" and value >= fo.FAR, (what, value)
    crossing = {a.arg for a in s.accesses if a.aliases()}
    assert crossing == CROSSING[case.id], (case.id, crossing)
    for arg in crossing:
        accs = [a for a in s.accesses if a.arg == arg]
        assert any(a.full >= fo.FAR for a in accs), (arg, "no access through it is far")
        last = max(accs, key=lambda a: a.full)
        cut = [t for t in last.terms if t.cuts() != {t.value}]
        assert cut and all(t.value >= fo.FAR for t in cut), (arg, last.terms)      # the term itself, not a sum of small ones
        if case.kind == "value":
            assert all(t.index == 1 and t.stride >= fo.FAR for t in cut)
        elif case.kind == "product":
            assert all(t.index == 2 and t.stride * t.scale < fo.FAR for t in cut)
        else:                                                   # a far column: an element index below 2^32 whose byte offset is not
            col = [t for t in cut if t.stride == 1]
            assert col and all(t.index < fo.FAR and t.scale in (4, 8) for t in col)


@pytest.mark.parametrize("case", fd.CASES, ids=IDS)
def test_b_every_address_cut_or_not_stays_inside_the_arena(setups, case):
    s = _setup(setups, case)
    cut = 0
    for acc in s.accesses:
        for a in [acc.full] + acc.aliases():
            assert 0 <= a and a + acc.nbytes <= s.pre.size, (acc.arg, hex(a))
            assert s.pre.get(a, acc.nbytes) is not None and s.post.get(a, acc.nbytes) is not None, (acc.arg, hex(a), "not compared")
        cut += len(acc.aliases())
    assert cut > 0
    assert s.pre.nbytes() < 8 << 20 and [w[0] for w in s.pre.wins] == [w[0] for w in s.post.wins]      # kilobytes, not the arena
    for lo, buf, _m in s.pre.wins:
        assert 0 <= lo and lo + buf.size <= s.pre.size


@pytest.mark.parametrize("case", fd.CASES, ids=IDS)
def test_c_a_region_and_its_alias_are_apart_and_differ(setups, case):
    s = _setup(setups, case)
    true = [(a.full, a.full + a.nbytes) for a in s.accesses if a.nbytes]
    for acc in s.accesses:
        if not acc.nbytes:
            continue
        here = s.pre.get(acc.full, acc.nbytes)
        for a in acc.aliases():
            # the alias of a region touches no true region of the case: what a cut reads is a decoy, what it writes is canary
            assert all(a + acc.nbytes <= lo or hi <= a for lo, hi in true), (acc.arg, hex(acc.full), hex(a))
            if acc.role == "in":
                assert not np.array_equal(here, s.pre.get(a, acc.nbytes)), (acc.arg, hex(acc.full), hex(a))
            elif not any(o.role == "in" and o.full <= acc.full and acc.full + acc.nbytes <= o.full + o.nbytes for o in s.accesses):
                assert (s.pre.get(a, acc.nbytes) == fo.CANARY).all(), (acc.arg, hex(a), "no canary at the alias of an output")
        if acc.role == "out" and acc.aliases():
            assert not np.array_equal(s.post.get(acc.full, acc.nbytes), here), (acc.arg, hex(acc.full), "the call changes nothing here")
    # canary around every written row: PAD bytes on either side that no region of the case covers
    for acc in s.accesses:
        if acc.role != "out" or any(o.role == "in" and o.full <= acc.full and acc.full + acc.nbytes <= o.full + o.nbytes for o in s.accesses):
            continue
        for a in (acc.full - 16, acc.full + acc.nbytes):
            edge = s.post.get(a, 16)
            free = np.array([not any(lo <= a + i < hi for lo, hi in true) for i in range(16)])      # (adjacent ranges touch)
            assert edge is not None and (edge[free] == fo.CANARY).all(), (acc.arg, hex(a))


@pytest.mark.parametrize("case", fd.CASES, ids=IDS)
def test_d_the_layout_meets_the_argument_rules(setups, case):
    s = _setup(setups, case)
    assert s.rules
    for rule, holds in s.rules:
        assert holds, (case.id, rule)


def test_every_entry_point_has_its_far_values_its_far_products_and_its_far_column():
    kinds = {}
    for c in fd.CASES:
        kinds.setdefault((c.entry, c.far), set()).add(c.kind)
    both = {"value", "product"}
    for entry, operands in (("mhw_xty", ("x_row_stride", "y_row_stride")), ("mhw_fir", ("x_row_stride", "out_row_stride")),
                            ("mhc_moments", ("p_row_stride", "y_row_stride")), ("mhc_polyval", ("p_row_stride", "out_row_stride", "in place")),
                            ("mhs_box_f32", ("in_row_stride", "out_row_stride")), ("mhq_xty_clips", ("x_row_stride", "y_row_stride")),
                            ("mhk_project", ("x_row_stride", "v_row_stride")), ("mhk_scan", ("v_row_stride", "out_row_stride", "in place"))):
        for op in operands:
            assert kinds[(entry, op)] == both, (entry, op)
    # the calls that take ranges have their far column in the table, the others over the whole length
    for entry in ("mhc_moments", "mhq_xty_clips", "mhk_scan"):
        assert kinds[(entry, "ranges")] == {"column"}
    assert set(fd.WHOLE) == {"mhw_xty", "mhw_fir", "mhc_polyval", "mhs_box_f32", "mhk_project"}
    # the far products that tests/test_gpu_box.py and tests/test_gpu_sweep.py lack
    assert kinds[("mhs_box", "x_row_stride")] == kinds[("mhs_box", "out_row_stride")] == kinds[("mhq_gram_clips", "x_row_stride")] == {"product"}
    # mhk_scan's far column with k = 1 and k = 2, in place, 3 * 512 + 9 steps, n_gain 5
    assert [c.args for c in fd.CASES if c.entry == "mhk_scan" and c.kind == "column"] == [(1,), (2,)]
    assert fd.SCAN_STEPS == 3 * 512 + 9 and fd.SCAN_GAINS == 5


def test_the_whole_length_shapes_pass_2_32_by_a_tile_and_a_ragged_end():
    from tests import test_host_box as hb
    from tests import test_host_cascade as hc
    from tests import test_host_kalman as hk
    from tests import test_host_wiener as hw
    # the layout mirrors of the host tests are the constants of the table
    assert (fd.XTY_RUN, fd.MOM_RUN, fd.BOX_TILE, fd.PROJ_TILE, fd.SCAN_TILE) == (hw.RUN, hc.RUN, hb.TILE_COLS, hk.PROJ_TILE, hk.TILE)
    assert hw.TILE_COLS == fd.FIR_TILE and hw.layout(1, 2 * (fd.FIR_TILE - 1), 2, 1)[7:9] == [fd.FIR_TILE - 1, 2]      # lags 2: 511 outputs a tile
    unit = {"mhw_xty": fd.XTY_RUN, "mhw_fir": fd.FIR_TILE - 1, "mhc_polyval": fd.POLY_TILE, "mhs_box_f32": fd.BOXF_TILE, "mhk_project": fd.PROJ_TILE}
    for entry, (cols, elem, need, _what) in fd.WHOLE.items():
        first = fo.FAR // elem                                      # the column whose byte offset is 2^32
        assert first + unit[entry] < cols < first + 2 * unit[entry] and (cols - first) % unit[entry] not in (0, 1), entry
        assert cols % 4 != 0 and cols * elem <= fo.ARENA_BYTES and fo.ARENA_BYTES - cols * elem > 1 << 20      # a tail that keeps its canary
        assert need >= fo.ARENA_BYTES + (4 << 30) and fd.WHOLE_CHUNK <= 1 << 26
    assert fd.WHOLE["mhs_box_f32"][2] >= 2 * fo.ARENA_BYTES         # its input is a second buffer of the same size


# ---- the argument rules about strides, through the check programs of the five host tests ------------------------------------
from tests import test_host_box as hb  # noqa: E402
from tests import test_host_cascade as hc  # noqa: E402
from tests import test_host_kalman as hk  # noqa: E402
from tests import test_host_sweep as hs  # noqa: E402
from tests import test_host_wiener as hw  # noqa: E402

wiener_exe, cascade_exe, box_exe, sweep_exe, kalman_exe = hw.exe, hc.exe, hb.exe, hs.exe, hk.exe
T48 = 1 << 48


def test_wiener_cascade_and_sweep_take_two_rows_2_48_less_8_apart(wiener_exe, cascade_exe, sweep_exe):
    top = T48 - 8
    lines = [hw._line("xty", hw.XTY, hw._args(hw.XTY, rows=2, x_row_stride=top, scratch_bytes=2 * 5 * 2 * 8)[1]),
             hw._line("xty", hw.XTY, hw._args(hw.XTY, k=2, y_row_stride=top)[1]),
             hw._line("fir", hw.FIR, hw._args(hw.FIR, rows=2, x_row_stride=top)[1]),
             hw._line("fir", hw.FIR, hw._args(hw.FIR, k=2, out_row_stride=top, out=1 << 60)[1])]
    assert hw._run(wiener_exe, "".join(lines)) == ["ok"] * 4
    lines = [hc._line("mom", hc.MOM, hc._args(hc.MOM, k=2, p_row_stride=top)[1]),
             hc._line("mom", hc.MOM, hc._args(hc.MOM, k=2, y_row_stride=top)[1]),
             hc._line("poly", hc.POLY, hc._poly_args(k=2, p_row_stride=top, out=1 << 60)[1]),
             hc._line("poly", hc.POLY, hc._poly_args(k=2, out_row_stride=top, out=1 << 60)[1]),
             hc._line("poly", hc.POLY, hc._poly_args(k=2, p_row_stride=top, out_row_stride=top, out="p", coef=1 << 50)[1])]
    assert hc._run(cascade_exe, "".join(lines)) == ["ok"] * 5
    lines = [hs._line(hs.GRAM, hs._args(hs.GRAM, rows=2, x_row_stride=top)[1]),
             hs._line(hs.XTY, hs._args(hs.XTY, rows=2, x_row_stride=top)[1]),
             hs._line(hs.XTY, hs._args(hs.XTY, k=2, y_row_stride=top)[1])]
    assert hs._run(sweep_exe, "".join(lines)) == ["ok"] * 3
    # their headers document no upper bound on a stride; if one is added, its refusal belongs here
    for name in ("muahuff_wiener.h", "muahuff_cascade.h", "muahuff_sweep.h"):
        assert "2^48" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_smooth_and_kalman_take_2_48_less_8_and_refuse_2_48(box_exe, kalman_exe):
    top = T48 - 8
    good = [hb._line("box", hb.BOX, hb._args(hb.BOX, rows=2, x_row_stride=top, lo=1 << 60, hi=1 << 61)[1]),
            hb._line("box", hb.BOX, hb._args(hb.BOX, rows=2, out_row_stride=T48 - 16, lo=1 << 60, hi=1 << 61)[1]),
            hb._line("boxf", hb.BOXF, hb._boxf_args(k=2, in_row_stride=top, out=1 << 60, bias=1 << 61)[1]),
            hb._line("boxf", hb.BOXF, hb._boxf_args(k=2, out_row_stride=top, out=1 << 60, bias=1 << 61)[1])]
    bad = [hb._line("box", hb.BOX, hb._args(hb.BOX, rows=2, x_row_stride=T48, lo=1 << 60, hi=1 << 61)[1]),
           hb._line("box", hb.BOX, hb._args(hb.BOX, rows=2, out_row_stride=T48, lo=1 << 60, hi=1 << 61)[1]),
           hb._line("boxf", hb.BOXF, hb._boxf_args(k=2, in_row_stride=T48, out=1 << 60, bias=1 << 61)[1]),
           hb._line("boxf", hb.BOXF, hb._boxf_args(k=2, out_row_stride=T48, out=1 << 60, bias=1 << 61)[1])]
    got = hb._run(box_exe, "".join(good + bad))
    assert got[:4] == ["ok"] * 4, got
    assert all(re.match(r"error -?\d+ mhs_box(_f32)?: .*not below 2\^48", ln) for ln in got[4:]) and len(got) == 8, got
    good = [hk._line(hk.PROJECT, hk._args(hk.PROJECT, rows=2, x_row_stride=top, v=1 << 60)[1]),
            hk._line(hk.PROJECT, hk._args(hk.PROJECT, k=2, v_row_stride=top, v=1 << 60)[1]),
            hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, v_row_stride=top, v=1 << 60)[1]),
            hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, out_row_stride=top, out=1 << 60)[1]),
            hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, v_row_stride=top, out_row_stride=top, v=1 << 60, out="v")[1])]
    bad = [hk._line(hk.PROJECT, hk._args(hk.PROJECT, rows=2, x_row_stride=T48, v=1 << 60)[1]),
           hk._line(hk.PROJECT, hk._args(hk.PROJECT, k=2, v_row_stride=T48, v=1 << 60)[1]),
           hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, v_row_stride=T48, v=1 << 60)[1]),
           hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, out_row_stride=T48, out=1 << 60)[1])]
    got = hk._run(kalman_exe, "".join(good + bad))
    assert got[:5] == ["ok"] * 5, got
    assert all(re.match(r"error -?\d+ mhk_(project|scan): .*2\^48", ln) for ln in got[5:]) and len(got) == 9, got
    for name in ("muahuff_smooth.h", "muahuff_kalman.h"):
        assert "2^48 or more" in open(os.path.join(ROOT, "include", name)).read(), name


def test_the_check_programs_take_the_strides_of_the_table(wiener_exe, cascade_exe, box_exe, sweep_exe, kalman_exe):
    """the far strides themselves, with the shapes of the cases, pass every argument check"""
    for kind in ("value", "product"):
        n, s1 = fd._stride(kind, fd.EX1)
        _n, s4 = fd._stride(kind, fd.EX4, 4)
        _n, s8 = fd._stride(kind, fd.EX8, 8)
        _n, s16 = fd._stride(kind, fd.EX16, 16)
        need = n * fd.XTY_LAGS * 2 * 8
        lines = [hw._line("xty", hw.XTY, hw._args(hw.XTY, rows=n, cols=fd.XTY_COLS, lags=fd.XTY_LAGS, x_row_stride=s1, y_row_stride=4 * fd.XTY_COLS + 12, scratch_bytes=need)[1]),
                 hw._line("xty", hw.XTY, hw._args(hw.XTY, rows=2, k=n, cols=fd.XTY_COLS, lags=fd.XTY_LAGS, x_row_stride=fd.XTY_COLS + 39, y_row_stride=s4, scratch_bytes=need)[1]),
                 hw._line("fir", hw.FIR, hw._args(hw.FIR, rows=n, cols=fd.FIR_COLS, lags=fd.FIR_LAGS, x_row_stride=s1, out_row_stride=4 * fd.FIR_COLS + 12)[1]),
                 hw._line("fir", hw.FIR, hw._args(hw.FIR, rows=2, k=n, cols=fd.FIR_COLS, lags=fd.FIR_LAGS, x_row_stride=fd.FIR_COLS + 39, out_row_stride=s4, out=1 << 60)[1])]
        assert hw._run(wiener_exe, "".join(lines)) == ["ok"] * 4, kind
        lines = [hc._line("poly", hc.POLY, hc._poly_args(k=n, cols=fd.POLY_COLS, p_row_stride=s4, out_row_stride=s4, out="p", coef=1 << 50)[1]),
                 hc._line("mom", hc.MOM, hc._args(hc.MOM, k=n, cols=2053, p_row_stride=s4, y_row_stride=4 * 2053 + 12, values=(3, 1000, 1000, 2053),
                                                  scratch_bytes=hc._need(2053, n, 2, 2), degree=2)[1])]
        assert hc._run(cascade_exe, "".join(lines)) == ["ok"] * 2, kind
        lines = [hk._line(hk.PROJECT, hk._args(hk.PROJECT, rows=n, cols=fd.PROJ_COLS, x_row_stride=s1, v_row_stride=8 * fd.PROJ_COLS + 40, v=1 << 60)[1]),
                 hk._line(hk.SCAN, hk._args(hk.SCAN, k=n, cols=1594, v_row_stride=s8, out_row_stride=s8, v=1 << 60, out="v",
                                            ranges=[(2, 40), (40, 40 + fd.SCAN_STEPS + 1)], n_gain=fd.SCAN_GAINS)[1])]
        assert hk._run(kalman_exe, "".join(lines)) == ["ok"] * 2, kind
        lines = [hb._line("boxf", hb.BOXF, hb._boxf_args(k=n, cols=fd.BOXF_COLS, window=fd.BOXF_WINDOW, in_row_stride=s4, out_row_stride=4 * fd.BOXF_COLS + 12,
                                                          out=1 << 60, bias=1 << 61)[1])]
        if kind == "product":
            lines += [hb._line("box", hb.BOX, hb._args(hb.BOX, rows=n, cols=fd.BOX_COLS, window=fd.BOX_WINDOW, x_row_stride=s1, out_row_stride=3920, lo=1 << 60, hi=1 << 61)[1]),
                      hb._line("box", hb.BOX, hb._args(hb.BOX, rows=n, cols=fd.BOX_COLS, window=fd.BOX_WINDOW, x_row_stride=fd.BOX_COLS + 86, out_row_stride=s16,
                                                       lo=1 << 60, hi=(1 << 60) + 0x100000)[1])]
        assert hb._run(box_exe, "".join(lines)) == ["ok"] * len(lines), kind
        lines = [hs._line(hs.GRAM, hs._args(hs.GRAM, rows=n, cols=300, lags=3, x_row_stride=s1, ranges=[(2, 150), (150, 300)], clips=[2, 39])[1]),
                 hs._line(hs.XTY, hs._args(hs.XTY, rows=2, k=n, cols=400, lags=3, lead=2, x_row_stride=437, y_row_stride=s4,
                                           ranges=[(2, 150), (150, 150), (190, 398)], clips=[2, 39])[1])]
        assert hs._run(sweep_exe, "".join(lines)) == ["ok"] * 2, kind
    # the far columns: cols just under the arena's element count, ranges past column 2^30 / 2^29
    cols = fd.ARENA_F32 - (1 << 18)
    a0 = (1 << 30) + 0x1003
    ln = hc._line("mom", hc.MOM, hc._args(hc.MOM, k=1, cols=cols, p_row_stride=0, y_row_stride=0, degree=2,
                                          values=(a0, a0 + 301, a0 + 0x2000, a0 + 0x2000 + 2 * fd.MOM_RUN + 77), scratch_bytes=hc._need(cols, 1, 2, 2))[1])
    assert hc._run(cascade_exe, ln) == ["ok"]
    cols, a0 = fd.ARENA_F64 - 16, (1 << 29) + 0x803
    ranges = [(a0, a0 + 40), (a0 + 0x1000, a0 + 0x1000 + fd.SCAN_STEPS + 1)]
    lines = [hk._line(hk.SCAN, hk._args(hk.SCAN, k=1, cols=cols, v_row_stride=0, out_row_stride=0, v=1 << 60, out="v", ranges=ranges, n_gain=5)[1]),
             hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, cols=cols, v_row_stride=fo.ARENA_BYTES, out_row_stride=fo.ARENA_BYTES, v=1 << 60, out="v",
                                        ranges=ranges, n_gain=5)[1]),
             # ... and why k = 2 takes an arena of its own: a second row less than 8 * cols bytes behind the first is refused
             hk._line(hk.SCAN, hk._args(hk.SCAN, k=2, cols=cols, v_row_stride=fo.ARENA_BYTES - 136, out_row_stride=fo.ARENA_BYTES - 136, v=1 << 60, out="v",
                                        ranges=ranges, n_gain=5)[1])]
    got = hk._run(kalman_exe, "".join(lines))
    assert got[:2] == ["ok", "ok"] and got[2].startswith("error") and "mhk_scan:" in got[2], got
