"""The table of tests/far_offsets.py without a GPU.  For every case:

  (a) the named quantity crosses 2^32 -- in bytes, and in words for the arena-W cases;
  (b) every address the call can form lies inside the arena and inside a window that the GPU test compares whole: with
      every offset, stride and product in full, and again with each one cut modulo 2^32 (the stride, the index * stride
      product, the product scaled to bytes, the whole sum).  A kernel that narrows any of them therefore cannot fault;
  (c) a far input and each of its aliases differ before the call; a far output is changed by the call (the yardstick's
      image differs from the canary, or from the values a += call starts from) and its alias is another address;
  (d) the layout meets the entry point's own argument rules (each Setup lists them).

Then the table as a whole: every row of the issue's table is there, every strided argument comes as far value and as far
product, and the windows of a case stay small -- no host array of arena size is ever built.

The two host-only builders that take a pitch or a stride without a change to their command line get the same far values:
the work-list printer of tests/planner_check.cpp (out_pitch of mh_decode_range / mh_decode_rebin) and
tests/windows_check.cpp (the strides of mhi_windows)."""
import numpy as np
import pytest

from tests import far_offsets as fo

IDS = [c.id for c in fo.CASES]


@pytest.fixture(scope="module")
def setups():
    return {}


def _setup(setups, case):
    if case.id not in setups:
        setups[case.id] = case.setup()
    return setups[case.id]


def test_the_arenas_are_what_the_layout_needs():
    assert fo.ARENA_BYTES == 2 ** 32 + 2 ** 28 and fo.ARENA_W_BYTES == 4 * (2 ** 32 + 2 ** 26) and fo.HEADROOM == 2 * 2 ** 30
    assert fo.SLACK < 2 ** 31          # d < 2^31: a signed and an unsigned cut give the same alias


def test_ids_are_unique_and_every_row_is_there():
    assert len(set(IDS)) == len(IDS)
    rows = {c.row for c in fo.CASES}
    assert rows >= {"rebin", "transpose", "synth", "sweep", "analysis", "crc", "unbin", "excess", "apply", "windows", "gram"}, rows


@pytest.mark.parametrize("case", fo.CASES, ids=IDS)
def test_a_the_named_quantity_crosses(setups, case):
    s = _setup(setups, case)
    assert s.arena == case.arena and s.pre.size == (fo.ARENA_BYTES if case.arena == "A" else fo.ARENA_W_BYTES)
    assert s.crossing, case.id
    for what, value, unit in s.crossing:
        assert unit in ("bytes", "words") and value >= fo.FAR, (what, value, unit)
    if case.arena == "W":
        assert any(unit == "words" for _w, _v, unit in s.crossing)
    assert any(a.full >= fo.FAR for a in s.accesses), "no access of the case is far"


@pytest.mark.parametrize("case", fo.CASES, ids=IDS)
def test_b_every_address_cut_or_not_stays_inside_the_arena(setups, case):
    s = _setup(setups, case)
    cut = 0
    for acc in s.accesses:
        for a in [acc.full] + acc.aliases():
            assert 0 <= a and a + acc.nbytes <= s.pre.size, (acc.arg, hex(a))
            assert s.pre.get(a, acc.nbytes) is not None and s.post.get(a, acc.nbytes) is not None, (acc.arg, hex(a), "not compared")
        cut += len(acc.aliases())
    assert cut > 0
    # the windows, nothing else, are ever on the host
    assert s.pre.nbytes() < 64 << 20 and [w[0] for w in s.pre.wins] == [w[0] for w in s.post.wins]
    for lo, buf, _m in s.pre.wins:
        assert 0 <= lo and lo + buf.size <= s.pre.size


@pytest.mark.parametrize("case", fo.CASES, ids=IDS)
def test_c_a_region_and_its_alias_differ(setups, case):
    s = _setup(setups, case)
    for acc in s.accesses:
        if not acc.nbytes:
            continue
        true = s.pre.get(acc.full, acc.nbytes)
        for a in acc.aliases():
            assert a != acc.full
            if acc.role == "in":
                assert not np.array_equal(true, s.pre.get(a, acc.nbytes)), (acc.arg, hex(acc.full), hex(a))
        if acc.role == "out" and acc.aliases():
            assert not np.array_equal(s.post.get(acc.full, acc.nbytes), true), (acc.arg, hex(acc.full), "the call changes nothing here")


@pytest.mark.parametrize("case", fo.CASES, ids=IDS)
def test_d_the_layout_meets_the_argument_rules(setups, case):
    s = _setup(setups, case)
    for rule, holds in s.rules:
        assert holds, (case.id, rule)


def test_strided_arguments_come_as_far_value_and_as_far_product():
    kinds = {}
    for c in fo.CASES:
        if c.kind in ("value", "product"):
            kinds.setdefault((c.entry, c.far.split(" (")[0]), set()).add(c.kind)
    assert kinds
    # chunk_stride has a lower bound only as a product (a chunk-blocked buffer of several chunks) and col_stride with three
    # elements likewise: a far value times index 2 lies behind the arena
    only_product = {"chunk_stride", "col_stride"}
    for (entry, far), k in kinds.items():
        assert k == {"value", "product"} or (far.split()[0] in only_product and k == {"product"}), (entry, far, k)


# ---- the host-only builders that take the far argument as it is -----------------------------------------------------------
from tests import helpers  # noqa: E402
from tests import test_host_gram as hg  # noqa: E402
from tests import test_host_windows as hw  # noqa: E402
from tests import test_host_worklist as wl  # noqa: E402
from tests import test_planner_sanitized as ps  # noqa: E402

plan_exe = ps.exe          # fixture: tests/planner_check.cpp under AddressSanitizer + UBSan
win_exe = hw.exe           # fixture: tests/windows_check.cpp, likewise
gram_exe = hg.exe          # fixture: tests/gram_check.cpp, likewise


def _rc(idx, pitch, n_sel, width):
    """element idx of a pitched result -> (row, column), inside the row's `width` elements"""
    row, col = divmod(int(idx), pitch)
    assert 0 <= row < n_sel and 0 <= col < width, (idx, pitch, row, col)
    return row, col


def _sparse_range(head, rec, seg, arr, w0, w1, sel, t0, t1, pitch):
    """wl._execute_range without the n_sel * pitch host buffer: one array per row"""
    wl._check_layout(head, rec, 48, False)
    ln = t1 - t0
    buf, cnt = np.full((len(sel), ln), 0xA5, np.uint8), np.zeros((len(sel), ln), np.int32)
    for dst, sg, skip, _ncnk, _n, lo, hi, _scr in rec["T"]:
        row, col = _rc(dst + lo, pitch, len(sel), ln)
        c = sel[row]
        src = wl._task_source(sg, skip, seg, w0, c)
        assert col + (hi - lo) <= ln and col + t0 == src + lo          # sample t lands on byte t - t0 of its row
        buf[row, col:col + hi - lo] = arr[c][src + lo:src + hi]
        cnt[row, col:col + hi - lo] += 1
    for off, n in rec["F"]:
        row, col = _rc(off, pitch, len(sel), ln)
        assert col + n <= ln
        buf[row, col:col + n] = 0
        cnt[row, col:col + n] += 1
    assert (cnt == 1).all()
    for i, c in enumerate(sel):
        assert np.array_equal(buf[i], wl._expected_row(arr, w0, w1, c, t0, t1)), (i, c)


def _sparse_rebin(head, rec, seg, arr, w0, w1, sel, t0, t1, r, pitch):
    """wl._execute_rebin likewise: direct writes, side slots with their fix records, fills -- every bin exactly once"""
    nside = wl._check_layout(head, rec, 64, True)
    nb = (t1 - t0 + r - 1) // r
    out, once = np.full((len(sel), nb), -1, np.int64), np.zeros((len(sel), nb), np.int32)
    side, users = np.zeros(nside, np.int64), [[] for _ in range(nside)]
    for dst, sg, skip, _n, lo, hi, ph, jfirst, jlast, head_, tail in rec["T"]:
        row, _col = _rc(dst + jfirst, pitch, len(sel), nb)
        c = sel[row]
        src = wl._task_source(sg, skip, seg, w0, c)
        assert jfirst == (ph + lo) // r and jlast == (ph + hi - 1) // r
        assert dst + (ph + lo) // r - row * pitch == (src + lo - t0) // r
        cuts = np.arange((jfirst + 1) * r - ph, hi, r)
        sums = np.add.reduceat(arr[c][src + lo:src + hi].astype(np.int64), np.concatenate([[0], cuts - lo]))
        to_out = np.ones(len(sums), bool)
        for j, slot in ((jfirst, head_), (jlast, tail)):
            if slot != wl.NO_SLOT and to_out[j - jfirst]:
                side[slot] += sums[j - jfirst]
                users[slot].append(dst + j)
                to_out[j - jfirst] = False
        for k in np.nonzero(to_out)[0]:
            rr, cc = _rc(dst + jfirst + k, pitch, len(sel), nb)
            assert rr == row
            out[rr, cc] = sums[k]
            once[rr, cc] += 1
    for off, slot in rec["X"]:
        rr, cc = _rc(off, pitch, len(sel), nb)
        assert all(at == off for at in users[slot])
        out[rr, cc] = side[slot]
        once[rr, cc] += 1
    for off, n in rec["F"]:
        rr, cc = _rc(off, pitch, len(sel), nb)
        assert cc + n <= nb
        out[rr, cc:cc + n] = 0
        once[rr, cc:cc + n] += 1
    assert (once == 1).all()
    for i, c in enumerate(sel):
        y = wl._expected_row(arr, w0, w1, c, t0, t1).astype(np.int64)
        assert np.array_equal(out[i], np.add.reduceat(y, np.arange(0, t1 - t0, r))), (i, c)


def test_the_work_list_builder_takes_the_far_pitches(plan_exe):
    """tests/planner_check.cpp --worklist with the out_pitch of the "range" cases: every dst, fix and fill offset is a
    64-bit element index row * pitch + column, executed here row by row against the slice and its bin sums"""
    from muahuff import container_io as cio
    lens, sc = fo.CODEC_LAYOUTS["wg"]
    lens = list(lens)
    S, h, window = wl.S, fo.CODEC_H, 3
    tab = helpers.sclv_tables()[S]
    case = "%d %d %d 1 %d %d %d  %s  %s" % (len(lens), S, h, window, len(tab), sc, " ".join(map(str, lens)),
                                             " ".join(str(int(v)) for v in tab.ravel()))
    t0, t1, r = fo.RANGE_T0, fo.RANGE_T1, fo.RANGE_R
    shapes = [([1, 0], 0, fo.FAR + 37), ([0, 1, 0], 0, (1 << 31) + 4099), ([1, 0], r, fo.FAR + 37), ([0, 1, 0], r, (1 << 31) + 4099),
              ([1, 0], r, (1 << 30) + 9), ([0, 1, 0], r, (1 << 29) + 1025)]          # the last two: elements of 4 bytes
    pitches = {c.args[:2]: c.setup().accesses for c in fo.CASES if c.row == "range" and c.arena == "A"}
    for what, k, (sel, rr, pitch) in zip(("range", "range", "rebin8", "rebin8", "rebin32", "rebin32"), ("value", "product") * 3, shapes):
        acc = [a for a in pitches[(what, k)] if a.arg == "out_pitch"]
        assert len(acc) == len(sel) and acc[1].terms[0].stride == pitch, (what, k)      # the table's own pitches
    qs = ["%d %s %d %d %d %d" % (len(sel), " ".join(map(str, sel)), t0, t1, rr, pitch) for sel, rr, pitch in shapes]
    rng = np.random.RandomState(3)
    arr = [rng.randint(0, S, size=n).astype(np.uint8) for n in lens]
    w0, w1 = (x.astype(np.int64) for x in cio.window_bounds(lens, h, window))
    (seg, lists), = wl._run(plan_exe, [(case, qs)])
    for (head, rec), (sel, rr, pitch) in zip(lists, shapes):
        e = 4 if pitch in ((1 << 30) + 9, (1 << 29) + 1025) else 1
        assert (len(sel) - 1) * pitch * e >= fo.FAR             # the last row's elements are written: the executors check every one
        if rr == 0:
            _sparse_range(head, rec, seg, arr, w0, w1, sel, t0, t1, pitch)
        else:
            _sparse_rebin(head, rec, seg, arr, w0, w1, sel, t0, t1, rr, pitch)


def test_the_gram_check_program_takes_the_far_strides(gram_exe):
    """tests/gram_check.cpp: the argument check accepts the strides of the "gram" cases, in both forms and with
    accumulate 0 and 1"""
    lines, n = "", 0
    near_a, near_b = fo.GRAM_COLS + 5, fo.GRAM_COLS + 9
    for kind in ("value", "product"):
        rows, rs, gs = fo._gram_strides(kind)
        assert (rs >= fo.FAR) == (gs >= fo.FAR) == (kind == "value") and (rows - 1) * rs >= fo.FAR and (rows - 1) * gs >= fo.FAR
        for over in (dict(a_rows=rows, a_row_stride=rs, b_rows=fo.GRAM_NEAR, b_row_stride=near_b, gram_row_stride=8 * (fo.GRAM_NEAR + 1)),
                     dict(a_rows=fo.GRAM_NEAR, a_row_stride=near_a, b_rows=rows, b_row_stride=rs, gram_row_stride=8 * (rows + 1)),
                     dict(a_rows=rows, a_row_stride=near_a, b_rows=fo.GRAM_NEAR, b_row_stride=near_b, gram_row_stride=gs),
                     dict(hg.SYM, a_rows=rows, a_row_stride=rs, gram_row_stride=8 * (rows + 1)),
                     dict(hg.SYM, a_rows=rows, a_row_stride=near_a, gram_row_stride=gs)):
            for acc in (0, 1):
                odd = dict(a_shift=1) if "b" in over else dict(a_shift=1, b_shift=3)          # (b stays NULL in the symmetric form)
                _keep, a = hg._args(cols=fo.GRAM_COLS, accumulate=acc, **odd, **over)
                lines += hg._line(a)
                n += 1
    assert hg._run(gram_exe, lines) == ["ok"] * n
    # the table's own strides are these
    cases = {c.args: c.setup() for c in fo.CASES if c.row == "gram" and c.kind != "offset"}
    for (far, kind, _form, _acc), s in cases.items():
        rows, rs, gs = fo._gram_strides(kind)
        strides = {t.stride for a in s.accesses if a.arg == far for t in a.terms}
        assert (gs if far == "gram_row_stride" else rs) in strides and len([a for a in s.accesses if a.arg == far]) >= rows, (far, kind)


def test_the_windows_check_program_takes_the_far_strides(win_exe):
    """tests/windows_check.cpp: the argument check accepts the strides of the "windows" cases, and the layout of their
    three forms is the restated rule"""
    lines, n = "", 0
    for kind in ("value", "product"):
        rows, rs, o4, o8 = fo._win_strides(kind)
        for W, r in fo.WIN_FORMS:
            nb = fo.ceil_div(W, r)
            for over in (dict(mode=hw.STACK, out_bits=8, out_win_stride=nb + 20, out_row_stride=o4 + 1, n_win=fo.WIN_N, n_out=fo.WIN_N),
                         dict(mode=hw.STACK, out_bits=32, out_win_stride=4 * nb + 20, out_row_stride=o4, n_win=fo.WIN_N, n_out=fo.WIN_N),
                         dict(mode=hw.STACK, out_bits=32, out_win_stride=o4, out_row_stride=4 * nb + 12, n_win=rows, n_out=rows),
                         dict(mode=hw.SUM, out_bits=32, out_row_stride=o4, sumsq="given", sq_row_stride=o8, n_win=fo.WIN_N, n_out=0)):
                _keep, a = hw._args(row_stride=rs, rows=rows, cols=fo.WIN_COLS, W=W, r=r,
                                    win_idx="given" if over["mode"] == hw.STACK else None, **over)
                lines += hw._line(a)
                n += 1
    assert hw._run(win_exe, lines) == ["ok"] * n
    grid = [(mode, rows, W, r, nw) for W, r in fo.WIN_FORMS
            for mode, rows, nw in ((hw.STACK, 2, fo.WIN_N), (hw.STACK, 3, 3), (hw.SUM, 3, fo.WIN_N))]
    got = hw._run(win_exe, "".join("layout %d %d %d %d %d\n" % g for g in grid))
    assert [[int(v) for v in ln.split()] for ln in got] == [hw._layout(*g) for g in grid]
    assert {hw._layout(*g)[0] for g in grid} == {0, 1, 2}                 # one case per form
