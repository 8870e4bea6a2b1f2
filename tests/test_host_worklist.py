"""The work lists of mh_decode_range and mh_decode_rebin (csrc/mh_worklist.hpp -- every address the range kernels
write is decided there) without a GPU: tests/planner_check.cpp --worklist builds them under AddressSanitizer + UBSan
and prints the records, and each list is then executed as a program, in NumPy, against random per-channel arrays:
sample x of a task is channel sample w0 + seg_first + skip * CHUNK + x.  The range list must reproduce the zero-extended
slice and write every byte of a row exactly once; the re-bin list, routed as RebinSink::emit routes (side slot for the
first bin with `head`, for the last with `tail`, else a direct write), then fixed and filled, must reproduce
np.add.reduceat, every bin being exactly one of: zero-filled, written by one task, summed in one slot with one fix.

Bin factors: 1, 3, 5, 50, 4096, and one above the shortest head segment.  A bin of at most 4096 samples is shorter
than a chunk, and only the first and the last segment of a window can be shorter than a chunk, so such a bin meets at
most two tasks; the slot chain across three tasks is driven here with r = 20000 on one-chunk segments (beyond what
mh_decode_rebin accepts: the builder itself has no such limit)."""
import os
import subprocess

import numpy as np
import pytest

import muahuff
from muahuff import container_io as cio
from tests import helpers
from tests.test_host_range_decode import _boundaries
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

CH = muahuff.CHUNK
S = 3
NO_SLOT = 0xFFFFFFFF
# the layouts of test_range_segments_follow_the_planner_directory: (h, seg_chunks, lens)
LAYOUTS = ((2, 1, [16 * CH + 1000, 50000, 20 * CH + 3, 5]), (3, 2, [40 * CH + 7, 16 * CH, 3, 70001]),
           (6, 3, [33 * CH + 100, 64, 65, 16 * CH + 64 + 5]))
RS = (1, 3, 5, 50, 4096)
R_THREE_TASKS = 20000
N_THINNED = 16   # boundary pairs kept per (layout, window, revision), of the cross product


def _channels(lens):
    rng = np.random.RandomState(len(lens) + sum(lens) % 1000)
    return [rng.randint(0, S, size=n).astype(np.uint8) for n in lens]


CHANNELS = {i: _channels(lens) for i, (_, _, lens) in enumerate(LAYOUTS)}


def _up16(x):
    return (x + 15) & ~15


def _queries(h, sc, lens, window, seg, rng):
    """[(kinds, sel, t0, t1)]: the required kinds of range first, then a fixed-seed sample of the boundary pairs and a
    few random ranges; sel repeats a channel and names the layout's shortest one (outside most ranges)"""
    w0, w1 = (x.astype(np.int64) for x in cio.window_bounds(lens, h, window))
    T = max(lens)
    short = int(np.argmin(lens))
    long_ = int(np.argmax(w1 - w0))
    other = [c for c in range(len(lens)) if c not in (short, long_)]
    sels = ([long_, short, long_, other[0]], [other[1], long_, short], [short], [long_, other[0], other[0], other[1]])
    ids = np.nonzero(seg["ch"] == long_)[0]
    mid = int(ids[len(ids) // 2])
    a0 = int(w0[long_]) + int(seg["first"][mid])
    need = [("one_chunk", a0 + 5, a0 + 1005),                       # inside chunk 0 of a middle segment
            ("segment_boundary", a0 - 7, a0 + 9),                   # the last samples of one segment, the first of the next
            ("window_ends", 0, T),                                  # starts at or before every window, ends behind every one
            ("no_window", int(w1[short]), int(w1[short]) + 40)]     # behind the shortest channel's window
    pts = _boundaries(lens, h, window, sc)
    pairs = [(a, b) for a in pts[::3] for b in pts[::5] if a < b]
    keep = rng.choice(len(pairs), size=min(N_THINNED, len(pairs)), replace=False)
    more = [pairs[i] for i in sorted(keep)]
    more += [tuple(sorted(int(x) for x in rng.randint(0, T + 1, size=2))) for _ in range(4)]
    out = [(kind, sels[0], a, b) for kind, a, b in need]
    out += [("", sels[i % len(sels)], a, b) for i, (a, b) in enumerate(more) if a < b]
    return out


def _kinds_seen(sel, t0, t1, lens, h, window, seg):
    """which of the kinds a query must cover it does cover, from the directory"""
    w0, w1 = (x.astype(np.int64) for x in cio.window_bounds(lens, h, window))
    seen = set()
    for c in sel:
        a, b = max(t0, int(w0[c])), min(t1, int(w1[c]))
        if a >= b:
            seen.add("no_window")
            continue
        if t0 <= w0[c] and t1 >= w1[c] and (t1 > w1[c] or t0 < w0[c]):
            seen.add("window_ends")
        ids = np.nonzero(seg["ch"] == c)[0]
        hit = [s for s in ids if seg["first"][s] < b - w0[c] and seg["first"][s] + seg["n"][s] > a - w0[c]]
        if len(hit) > 1:
            seen.add("segment_boundary")
        elif (a - w0[c] - seg["first"][hit[0]]) // CH == (b - 1 - w0[c] - seg["first"][hit[0]]) // CH:
            seen.add("one_chunk")
    return seen


def _run(exe_path, plans):
    """plans: [(case line, [query lines])] -> per plan (directory, [parsed list per query])"""
    text = "".join("%s\n%d\n%s\n" % (case, len(qs), "\n".join(qs)) for case, qs in plans)
    r = subprocess.run([exe_path, "--worklist"], input=text, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    pos, out = 0, []
    for _, qs in plans:
        assert lines[pos].split()[0] == "D"
        seg = {name: np.array(lines[pos + 1 + k].split(), dtype=np.int64) for k, name in enumerate(("ch", "first", "n"))}
        assert len(seg["ch"]) == int(lines[pos].split()[1])
        pos += 4
        lists = []
        for q in qs:
            head = [int(v) for v in lines[pos].split()[1:]]
            pos += 1
            rec = {}
            for key, cnt, width in zip("TWXF", head[:4], (11 if q.split()[-2] != "0" else 8, 3, 2, 2)):
                rows = [lines[pos + i].split() for i in range(cnt)]
                assert all(row[0] == key and len(row) == width + 1 for row in rows)
                rec[key] = np.array([[int(v) for v in row[1:]] for row in rows], dtype=np.int64).reshape(cnt, width)
                pos += cnt
            lists.append((head, rec))
        out.append((seg, lists))
    assert pos == len(lines)
    return out


def _check_layout(head, rec, task_bytes, has_fix):
    """section offsets and counts of the packed blob; the workgroup records partition the tasks in order"""
    ntask, nwg, nfix, nfill, naux, max_fill, o_wg, o_fix, o_fill, size = head
    assert o_wg == _up16(ntask * task_bytes) and o_fix == o_wg + _up16(nwg * 16) and o_fill == o_fix + _up16(nfix * 16)
    assert size == o_fill + nfill * 16 and o_wg % 16 == 0 and o_fix % 16 == 0 and o_fill % 16 == 0
    assert has_fix or nfix == 0
    F = rec["F"]
    assert nfill == 0 or F[:, 1].min() > 0                 # no empty fill record
    assert max_fill == (int(F[:, 1].max()) if nfill else 0)
    nxt = 0
    for task0, n, _ in rec["W"]:
        assert task0 == nxt and 1 <= n <= 4
        nxt += n
    assert nxt == ntask
    return naux


def _task_source(t_seg, t_skip, seg, w0, c):
    assert seg["ch"][t_seg] == c
    return int(w0[c]) + int(seg["first"][t_seg]) + int(t_skip) * CH


def _expected_row(arr, w0, w1, c, t0, t1):
    y = np.zeros(t1 - t0, np.uint8)
    a, b = max(t0, int(w0[c])), min(t1, int(w1[c]))
    if a < b:
        y[a - t0:b - t0] = arr[c][a:b]
    return y


def _execute_range(head, rec, seg, arr, w0, w1, sel, t0, t1, pitch):
    nscr = _check_layout(head, rec, 48, False)
    n_sel, ln = len(sel), t1 - t0
    buf = np.full(n_sel * pitch, 0xA5, np.uint8)
    cnt = np.zeros(n_sel * pitch, np.int32)
    T = rec["T"]
    rows, cut = [], []
    for dst, sg, skip, ncnk, n, lo, hi, scr in T:
        row = (dst + lo) // pitch
        rows.append(row)
        assert 0 <= row < n_sel
        c = sel[row]
        src = _task_source(sg, skip, seg, w0, c)
        assert lo < CH and lo < hi <= n and hi > (ncnk - 1) * CH and ncnk >= 1
        assert n == min(seg["n"][sg] - skip * CH, ncnk * CH)
        assert row * pitch <= dst + lo and dst + hi <= row * pitch + ln     # nothing outside the row
        assert dst + lo - row * pitch + t0 == src + lo                      # sample t lands on byte t - t0 of the row
        buf[dst + lo:dst + hi] = arr[c][src + lo:src + hi]
        cnt[dst + lo:dst + hi] += 1
        if lo > 0 or hi < n:
            cut.append(scr)
    assert len(set(cut)) == len(cut) == nscr and all(0 <= s < nscr for s in cut)
    for task0, n, ch in rec["W"]:
        assert len({rows[task0 + k] for k in range(n)}) == 1 and sel[rows[task0]] == ch
    for off, n in rec["F"]:
        row = off // pitch
        assert row * pitch <= off and off + n <= row * pitch + ln
        buf[off:off + n] = 0
        cnt[off:off + n] += 1
    buf, cnt = buf.reshape(n_sel, pitch), cnt.reshape(n_sel, pitch)
    assert (cnt[:, :ln] == 1).all() and (cnt[:, ln:] == 0).all() and (buf[:, ln:] == 0xA5).all()
    for i, c in enumerate(sel):
        assert np.array_equal(buf[i, :ln], _expected_row(arr, w0, w1, c, t0, t1)), (i, c)


def _execute_rebin(head, rec, seg, arr, w0, w1, sel, t0, t1, r, pitch):
    """-> the largest number of tasks that share one side slot"""
    nside = _check_layout(head, rec, 64, True)
    n_sel, nb = len(sel), (t1 - t0 + r - 1) // r
    out = np.full(n_sel * pitch, -1, np.int64)
    direct = np.zeros(n_sel * pitch, np.int32)
    fixed = np.zeros(n_sel * pitch, np.int32)
    filled = np.zeros(n_sel * pitch, np.int32)
    side = np.zeros(nside, np.int64)
    users = [[] for _ in range(nside)]         # (task, element of `out` its bin is) per slot
    rows = []
    for k, (dst, sg, skip, n, lo, hi, ph, jfirst, jlast, head_, tail) in enumerate(rec["T"]):
        row = (dst + jfirst) // pitch
        rows.append(row)
        assert 0 <= row < n_sel
        c = sel[row]
        src = _task_source(sg, skip, seg, w0, c)
        assert lo < CH and lo < hi <= n and ph < r
        assert n == min(seg["n"][sg] - skip * CH, ((hi - 1) // CH + 1) * CH)
        assert jfirst == (ph + lo) // r and jlast == (ph + hi - 1) // r
        # sample x lies in bin (t - t0) // r of the row
        assert dst + (ph + lo) // r - row * pitch == (src + lo - t0) // r
        cuts = np.arange((jfirst + 1) * r - ph, hi, r)              # first samples of the bins behind jfirst
        sums = np.add.reduceat(arr[c][src + lo:src + hi].astype(np.int64), np.concatenate([[0], cuts - lo]))
        assert len(sums) == jlast - jfirst + 1
        to_out = np.ones(len(sums), bool)
        for j, slot in ((jfirst, head_), (jlast, tail)):            # RebinSink::emit: head before tail
            if slot != NO_SLOT and to_out[j - jfirst]:
                assert 0 <= slot < nside
                side[slot] += sums[j - jfirst]
                users[slot].append((k, dst + j))
                to_out[j - jfirst] = False
        idx = dst + jfirst + np.nonzero(to_out)[0]
        if idx.size:
            assert row * pitch <= idx[0] and idx[-1] < row * pitch + nb     # no direct write outside the row
        out[idx] = sums[to_out]
        direct[idx] += 1
    for task0, n, ch in rec["W"]:
        assert len({rows[task0 + k] for k in range(n)}) == 1 and sel[rows[task0]] == ch
    X = rec["X"]
    assert sorted(X[:, 1].tolist()) == list(range(nside))           # one fix record per slot, slots distinct
    for off, slot in X:
        row = off // pitch
        assert row * pitch <= off < row * pitch + nb
        assert len(users[slot]) >= 2 and all(at == off for _, at in users[slot])   # one bin, several tasks
        tasks = [k for k, _ in users[slot]]
        assert tasks == list(range(tasks[0], tasks[0] + len(tasks)))
        out[off] = side[slot]
        fixed[off] += 1
    for off, n in rec["F"]:
        row = off // pitch
        assert row * pitch <= off and off + n <= row * pitch + nb
        out[off:off + n] = 0
        filled[off:off + n] += 1
    once = (direct + fixed + filled).reshape(n_sel, pitch)
    assert (once[:, :nb] == 1).all() and (once[:, nb:] == 0).all()
    out = out.reshape(n_sel, pitch)
    assert (out[:, nb:] == -1).all()
    for i, c in enumerate(sel):
        y = _expected_row(arr, w0, w1, c, t0, t1).astype(np.int64)
        assert np.array_equal(out[i, :nb], np.add.reduceat(y, np.arange(0, t1 - t0, r))), (i, c, r)
    return max((len(u) for u in users), default=0)


@pytest.mark.parametrize("rev", [2, 3])
@pytest.mark.parametrize("window", [0, 1, 2, 3])
def test_work_lists_execute_to_the_slice_and_its_bin_sums(exe, rev, window):  # noqa: F811
    rng = np.random.RandomState(100 * rev + window)
    tab = helpers.sclv_tables()[S]
    wflag = window | (muahuff._lib.WIN_REV2_SEGMENTS if rev == 2 else 0)
    # the directory first (no queries), to place the required ranges on it
    cases = ["%d %d %d 1 %d %d %d  %s  %s" % (len(lens), S, h, wflag, len(tab), sc, " ".join(map(str, lens)),
                                               " ".join(str(int(v)) for v in tab.ravel())) for h, sc, lens in LAYOUTS]
    segs = [seg for seg, _ in _run(exe, [(case, []) for case in cases])]
    plans, meta = [], []
    for k, (h, sc, lens) in enumerate(LAYOUTS):
        w0, w1 = cio.window_bounds(lens, h, window)
        heads = [int(n) for s, n in enumerate(segs[k]["n"]) if segs[k]["first"][s] == 0 and n < CH and
                 (w1 - w0)[segs[k]["ch"][s]] >= 16 * CH]
        r_head = min(heads) + 1 if heads else 125      # above the shortest head segment (no heads: above any possible one)
        qs, info = [], []
        for i, (kind, sel, a, b) in enumerate(_queries(h, sc, lens, window, segs[k], rng)):
            binned = [RS[i % len(RS)], RS[(i + 2) % len(RS)]] + ([r_head] if i % 3 == 0 else [])
            if sc == 1 and (kind == "window_ends" or i % 5 == 0):
                binned.append(R_THREE_TASKS)
            for r in [0] + binned:
                t0 = a - a % r if r else a
                row = (b - t0 + r - 1) // r if r else b - t0
                pitch = row + 13 if i % 2 else row
                qs.append("%d %s %d %d %d %d" % (len(sel), " ".join(map(str, sel)), t0, b, r, pitch))
                info.append((kind, sel, t0, b, r, pitch))
        plans.append((cases[k], qs))
        meta.append(info)
    shared = 0
    for k, ((seg, lists), info) in enumerate(zip(_run(exe, plans), meta)):
        h, sc, lens = LAYOUTS[k]
        assert all(np.array_equal(seg[name], segs[k][name]) for name in seg)
        w0, w1 = cio.window_bounds(lens, h, window)
        seen = set()
        for (head, rec), (kind, sel, t0, t1, r, pitch) in zip(lists, info):
            got = _kinds_seen(sel, t0, t1, lens, h, window, seg)
            assert r or not kind or kind in got, (kind, sel, t0, t1)    # (a binned query starts at a multiple of r)
            seen |= got
            if r == 0:
                _execute_range(head, rec, seg, CHANNELS[k], w0, w1, sel, t0, t1, pitch)
            else:
                n = _execute_rebin(head, rec, seg, CHANNELS[k], w0, w1, sel, t0, t1, r, pitch)
                assert n <= 2 or r > 4096
                shared = max(shared, n)
        assert seen == {"one_chunk", "segment_boundary", "window_ends", "no_window"}, (k, seen)
    assert shared >= 3      # r = 20000 on one-chunk segments: one bin, three tasks, one slot
