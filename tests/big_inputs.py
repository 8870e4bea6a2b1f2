"""Indices that pass 2^32 because of the AMOUNT of data one call handles -- tests/far_offsets.py crosses it in strides,
pitches and offset tables over a few KiB; here the ingest kernels get the data.  One table, two users:
tests/test_host_big_inputs.py (no GPU: every builder at a small crossing point against a brute-force NumPy model) and
tests/test_gpu_big_inputs.py (the calls themselves at 2^32).

A builder takes the crossing point FAR (2^32 on the GPU, 2^16 on the host) and returns a Built:

  shape     the few numbers of the call
  inputs    what the buffers hold, in a form a device can expand without a host copy: a short period to repeat, a
            constant fill, a list of planted (index, value) entries
  expect    the result in closed form, from those same few numbers: small tables as arrays, large outputs as functions
            of an index array
  cut       the same, as the call would return it if the named index were taken modulo FAR.  Every case plants a decoy
            at the alias (true index - FAR), or leaves canary where a cut index never arrives, so expect != cut
  accesses  the large buffers with their true far indices, for the no-fault rule: a true index, its unsigned cut and its
            sign-extended cut all lie inside the allocation (a buffer that is walked through [2^31, 2^32) starts LEAD =
            2^31 bytes inside its allocation, canary in front)
  peak      device bytes the GPU test holds at the worst moment

Nothing here calls the library under test.

Not built, and said so in DESIGN.md: win_split's other callers (the SUM form, the staged and the wave kernels) reach 2^32
items only by walking tens of GB; they share the one function that `windows-many-items` runs through the lane form."""
import math
from collections import namedtuple

import numpy as np

CANARY = 0xA5
CAN64 = int(np.frombuffer(bytes([CANARY]) * 8, np.int64)[0])
LEAD = 1 << 31
TILE = 16384                 # mh_unbin_layout.hpp: kUnbinTile
GROUP = 1024                 # kUnbinGroup
PERM = ((np.arange(256) * 167 + 13) % 256).astype(np.uint8)       # every value 0 .. 255 once
PERM_SUM = 255 * 128
ORIGIN, PERIOD, PHASE = 1000, 3, 1

Access = namedtuple("Access", "buf elem lead body base idx")       # bytes; idx: element indices from `base`
Built = namedtuple("Built", "shape inputs expect cut accesses peak")
Case = namedtuple("Case", "id entry crosses shape build")


P = 4099                     # the pattern period, and the data behind FAR
D = 1037                     # FAR + D is planted: below 2^31, so a signed and an unsigned cut give the same alias


def up16(x):
    return (x + 15) & ~15


def _perm_cum(shift):
    return np.concatenate([[0], np.cumsum(np.roll(PERM, -shift).astype(np.int64))])


def perm_range_sum(shift, a, b):
    """sum of PERM[(j + shift) % 256] over a <= j < b"""
    cum = _perm_cum(shift)
    at = lambda x: (x // 256) * PERM_SUM + int(cum[x % 256])       # noqa: E731
    return at(b) - at(a)


# ---- unbin-far-out -------------------------------------------------------------------------------------------------------
def unbin_far_out(far):
    unit = far // 8                               # out_ticks passes byte FAR at element FAR / 8
    reps = -(-(unit + P) // (3 * PERM_SUM))
    cols, E = 256 * reps, reps * PERM_SUM
    total = 3 * E
    shifts = [0, 5, 10]
    cums = [_perm_cum(s) for s in shifts]

    def ticks(e):
        e = np.asarray(e, np.int64)
        row, e2 = e // E, e % E
        q, r = e2 // PERM_SUM, e2 % PERM_SUM
        col = np.zeros_like(e)
        for i in range(3):
            col = np.where(row == i, np.searchsorted(cums[i], r, side="right") - 1, col)
        return ORIGIN + (q * 256 + col) * PERIOD + PHASE

    def cut_ticks(e):
        e = np.asarray(e, np.int64)
        last = e + unit * ((total - 1 - np.minimum(e, unit - 1)) // unit)          # the last event stored at e mod unit wins
        return np.where(e >= unit, CAN64, ticks(np.minimum(last, total - 1)))

    assert unit + P <= total
    ev_off = np.array([0, E, 2 * E, 3 * E], np.int64)
    body = 8 * (total + P)
    return Built(dict(rows=3, cols=cols, pitch=cols + 7, total=total, unit=unit, tail=P),
                 dict(kind="periodic rows", period=[np.roll(PERM, -s) for s in shifts], reps=reps),
                 dict(ev_off=ev_off, total=total, ticks=ticks, over=0),
                 dict(ev_off=ev_off, total=total, ticks=cut_ticks, over=0),
                 [Access("out_ticks", 8, LEAD, body, 0, [0, unit - 1, unit, total - 1])],
                 LEAD + body + 16 * E + 3 * 8 * 3 * cols + (1 << 28))


# ---- unbin-dense-group ----------------------------------------------------------------------------------------------------
def unbin_dense_group(far):
    tile = TILE if far == 1 << 32 else 16
    group = far // 256 // tile
    dense = tile * 255 * group                                       # 4 278 190 080 at 2^32
    assert far // 2 < dense < far
    cols = (group + 3) * tile
    s0 = dense + perm_range_sum(0, group * tile, cols)
    s1 = perm_range_sum(3, 0, cols)
    cap = max(far >> 16, 64)
    assert cap <= dense

    def ticks(e):
        return ORIGIN + (np.asarray(e, np.int64) // 255) * PERIOD + PHASE          # the first cap events: row 0, all 255

    def tables(first):
        ev = np.array([0, first, first + s1], np.int64)
        return dict(ev_off=ev, total=int(ev[2]), ticks=ticks, over=int(ev[2]) - cap)

    return Built(dict(rows=2, cols=cols, pitch=cols + 3, tile=tile, group=group, dense=dense, capacity=cap),
                 dict(kind="fill + periodic", fill=(0, 0, group * tile, 255), period=[PERM, np.roll(PERM, -3)]),
                 tables(s0), tables(s0 - far // 2),                  # the cut: the group's sum through 31 bits
                 [], 2 * (cols + 3) + (1 << 28))


# ---- the sparse un-binner cases --------------------------------------------------------------------------------------------
def _planted(far, n):
    """(index, count) in index order: FAR - 1, FAR, FAR + D, the last index, one in the middle, and a decoy at each alias"""
    p = [(0, 7), (D, 9), (n - 1 - far, 2), (far // 2 + 11, 8), (far - 1, 3), (far, 5), (far + D, 255), (n - 1, 4)]
    assert len({i for i, _c in p}) == len(p) and far + D < n - 1 and n - far < far // 2
    return sorted(p)


def _cut_planted(far, n, p):
    """what a read at index mod FAR sees: the entries below FAR, then the start of the buffer again up to n - FAR"""
    return [(i, c, i) for i, c in p if i < far] + [(i + far, c, i) for i, c in p if i + far < n]


def unbin_csr_long_row(far):
    cols = far + P
    rows = [_planted(far, cols), [(i, 256 - c) for i, c in _planted(far, cols)]]
    pitch = cols + 5

    def result(lists):
        """lists[row] = (column, count, column the tick is made from)"""
        t = [np.repeat([ORIGIN + j * PERIOD + PHASE for _i, _c, j in L], [c for _i, c, _j in L]).astype(np.int64) for L in lists]
        ev = np.array([0, t[0].size, t[0].size + t[1].size], np.int64)
        return dict(ev_off=ev, total=int(ev[2]), ticks=np.concatenate(t), over=0)

    return Built(dict(rows=2, cols=cols, pitch=pitch),
                 dict(kind="zeros + planted", planted=rows),
                 result([[(i, c, i) for i, c in r] for r in rows]), result([_cut_planted(far, cols, r) for r in rows]),
                 [Access("in row %d" % i, 1, LEAD, 2 * pitch, i * pitch, [j for j, _c in rows[i]]) for i in range(2)],
                 LEAD + 2 * pitch + (1 << 28))


def unbin_aer_big_block(far):
    cols = 1000
    rows = far // cols + 4           # the smallest block with three whole time steps behind FAR (FAR + 3 * cols + 7 is no
    n = rows * cols                  # multiple of cols)
    p = _planted(far, n)
    assert n >= far + 3 * cols + 7

    def result(L):
        cnt = [c for _i, c, _j in L]
        return dict(total=sum(cnt), over=0,
                    ticks=np.repeat([ORIGIN + (j // cols) * PERIOD + PHASE for _i, _c, j in L], cnt).astype(np.int64),
                    channels=np.repeat([j % cols for _i, _c, j in L], cnt).astype(np.int64))

    return Built(dict(rows=rows, cols=cols, n=n),
                 dict(kind="zeros + planted", planted=p),
                 result([(i, c, i) for i, c in p]), result(_cut_planted(far, n, p)),
                 [Access("in", 1, LEAD, n, 0, [i for i, _c in p])],
                 LEAD + n + (1 << 28))


# ---- aer-far-out -----------------------------------------------------------------------------------------------------------
AER_C = 3
AER_BASE = np.array([0, 1, 1, 0, 1, 0, 0], np.uint16)               # period 7: not cyclic in a wave's 64 pairs


def aer_pattern():
    """period 7 * 331 * 1009: channels 0 and 1 about half each, channel 2 one pair in 331, one pair in 1009 is >= C"""
    pat = np.tile(AER_BASE, 331 * 1009)
    pat[3::331] = 2
    bad = np.arange(5, pat.size, 1009)
    pat[bad] = 3 + (np.arange(bad.size) % 5)
    pat[5] = 0xFFFF
    return pat


def aer_far_out(far):
    unit = far // 8
    pat = aer_pattern()
    L = pat.size
    cum = [np.concatenate([[0], np.cumsum(pat == c, dtype=np.int64)]) for c in range(AER_C)]
    pos = [np.flatnonzero(pat == c).astype(np.int64) for c in range(AER_C)]
    count = lambda n, c: (n // L) * int(cum[c][L]) + int(cum[c][n % L])       # noqa: E731
    lo, hi = unit, 2 * unit                                          # the smallest n whose channel 2 starts behind unit
    while lo < hi:
        mid = (lo + hi) // 2
        if count(mid, 0) + count(mid, 1) >= unit + 1:
            hi = mid
        else:
            lo = mid + 1
    n = -(-(lo + P) // 3) * 3
    ev_off = np.cumsum([0] + [count(n, c) for c in range(AER_C)]).astype(np.int64)
    kept = int(ev_off[AER_C])
    assert ev_off[1] < unit < ev_off[2] < kept and n < far

    def run(c, k):
        """input index (= tick) of the k-th pair of channel c"""
        k = np.asarray(k, np.int64)
        return (k // pos[c].size) * L + pos[c][k % pos[c].size]

    def ticks(p):
        p = np.asarray(p, np.int64)
        out = np.zeros_like(p)
        for c in range(AER_C):
            m = (p >= ev_off[c]) & (p < ev_off[c + 1])
            out[m] = run(c, p[m] - ev_off[c])
        return out

    def cut_ticks(p):
        p = np.asarray(p, np.int64)
        last = p + unit * ((kept - 1 - np.minimum(p, unit - 1)) // unit)           # the last pair stored at p mod unit wins
        return np.where(p >= unit, CAN64, ticks(np.minimum(last, kept - 1)))

    body = 8 * (n + P)
    return Built(dict(n=n, C=AER_C, unit=unit, kept=kept, tail=P, L=L),
                 dict(kind="periodic", period=pat, positions=pos),
                 dict(ev_off=ev_off, dropped=n - kept, ticks=ticks, run=run),
                 dict(ev_off=ev_off, dropped=n - kept, ticks=cut_ticks, run=run),
                 [Access("out_ticks", 8, LEAD, body, 0, [0, unit - 1, unit, int(ev_off[2]), kept - 1])],
                 8 * n + LEAD + body + 2 * (n + L) + (1 << 29))            # the runs are compared after the inputs are freed


# ---- windows ---------------------------------------------------------------------------------------------------------------
WIN_W = 200
WIN_R = (1, 7, 100)
WIN_FORMS = ("stack8", "stack32idx", "sum")


def windows_far_offsets(far):
    d = D
    cols = far + 2 * P
    stride, W = cols + 13, WIN_W
    pat = np.random.RandomState(31).randint(0, 256, size=(2, P)).astype(np.uint8)
    offs = [5, P + 3, d, far // 2 + 17, far - W - 1, far - 100, far, far + 1, far + d, far + P + 11, far + 2 * P - W - 7, cols - W]
    idx = list(range(len(offs)))[::-1]
    assert sum(o >= far for o in offs) == 6 and max(offs) + W == cols and d + W <= P

    def val(i, c):
        c = np.asarray(c, np.int64)
        return np.where(c < 64, 255, pat[i][c % P]).astype(np.int64)

    def result(starts):
        win = np.array([[val(i, o + np.arange(W)) for i in range(2)] for o in starts])          # [12, 2, W]
        out = {}
        for r in WIN_R:
            sums = np.add.reduceat(win, np.arange(0, W, r), axis=2)
            by_slot = np.zeros_like(sums)
            by_slot[idx] = sums
            out["stack8", r] = np.minimum(sums, 255)
            out["stack32idx", r] = by_slot
            out["sum", r] = (sums.sum(0), (sums * sums).sum(0))
        return out

    return Built(dict(rows=2, cols=cols, stride=stride, W=W, n_win=len(offs)),
                 dict(kind="periodic rows + head", period=pat, head=(64, 255), win_off=offs, win_idx=idx),
                 result(offs), result([o % far for o in offs]),
                 [Access("in row %d" % i, 1, LEAD, 2 * stride, i * stride, offs + [o + W - 1 for o in offs]) for i in range(2)],
                 LEAD + 2 * stride + (1 << 28))


def windows_many_items(far):
    s = math.isqrt(far)
    rows, n_win, cols, pitch = s + 1, s, 257, 263
    items = rows * n_win

    def val(i, c):
        i, c = np.asarray(i, np.int64), np.asarray(c, np.int64)
        mix = i * (2 * c + 1) + (i >> 8) * (c + 1)
        return np.where(c == 0, i, np.where(c == 1, i >> 8, np.where(c == 2, i >> 16, mix))) & 255      # columns 0 .. 2 spell i

    def out(k, i):
        return val(i, np.asarray(k, np.int64) % cols)

    def cut_out(k, i):
        k, i = np.asarray(k, np.int64), np.asarray(i, np.int64)
        return np.where(k * rows + i >= far, CANARY, out(k, i))          # an item cut to 32 bits rewrites item - FAR

    assert s * s == far and items == far + s
    return Built(dict(rows=rows, n_win=n_win, cols=cols, pitch=pitch, W=1, r=1, items=items),
                 dict(kind="formula", val=val, win_off=lambda k: np.asarray(k, np.int64) % cols),
                 dict(out=out, bad=[0, -1]), dict(out=cut_out, bad=[0, -1]),
                 [Access("out", 1, LEAD, items, 0, [0, far - 1, far, items - 1])],
                 LEAD + items + items // 2 + rows * pitch * 9 + (1 << 28))


# ---- excess-cols-big-block -------------------------------------------------------------------------------------------------
EXC_THRESHOLD = 3


def excess_cols_big_block(far):
    C = 1024 + 3
    T = far // C + 6                 # the smallest block with five whole time steps behind FAR
    n, d = T * C, D
    p = sorted([(0, 9), (d, 200), (n - 1 - far, 77), (far // 2 + 11, 100), (far - 1, 4), (far, 255), (far + d, 10), (n - 1, 5)])
    assert n >= far + 5 * C and len({i for i, _v in p}) == len(p) and far + d < n - 1 and n - far < far // 2

    def result(L):
        """L = (flat index the entry stands for, value read)"""
        e = sorted((f % C, f // C, v - EXC_THRESHOLD) for f, v in L)
        off = np.concatenate([[0], np.cumsum(np.bincount([c for c, _t, _v in e], minlength=C))]).astype(np.int64)
        return dict(exc_off=off, total=len(e), over=0, pos=np.array([t for _c, t, _v in e], np.int64),
                    val=np.array([v for _c, _t, v in e], np.int64))

    return Built(dict(T=T, C=C, n=n, threshold=EXC_THRESHOLD),
                 dict(kind="zeros + planted", planted=p),
                 result(p), result([(i, v) for i, v, _j in _cut_planted(far, n, p)]),
                 [Access("in", 1, LEAD, n, 0, [i for i, _v in p])],
                 LEAD + n + 13 * C * (T // 512 + 1) + (1 << 28))


# ---- bin-long-channel ------------------------------------------------------------------------------------------------------
def bin_long_channel(far):
    d = D
    T = far + P
    runs = [[(3, 2), (far, 4), (T - 1, 1)],
            [(0, 1), (d, 2), (P - 1, 7), (far - 1, 300), (far, 2), (far + d, 1), (T - 1, 300)]]
    out_off = [0, up16(T) + 16]
    body = out_off[1] + T + 16
    ticks = [np.repeat([ORIGIN + b * PERIOD + b % PERIOD for b, _k in r], [k for _b, k in r]).astype(np.int64) for r in runs]
    ev_off = np.array([0, ticks[0].size, ticks[0].size + ticks[1].size], np.int64)

    def true(ch):
        return {b: min(k, 255) for b, k in runs[ch]}

    def cut(ch):
        """bin b >= FAR is stored at b - FAR: the tail overwrites [0, P), zeros included, and [FAR, T) keeps the canary"""
        t = true(ch)
        out = {b: v for b, v in t.items() if P <= b < far}
        out.update({b - far: v for b, v in t.items() if b >= far})
        return out

    return Built(dict(C=2, T=T, bits=8, origin=ORIGIN, period=PERIOD, out_off=out_off, body=body, tail=P),
                 dict(kind="planted runs", ticks=np.concatenate(ticks), ev_off=ev_off, runs=runs),
                 dict(bins=[true(0), true(1)], canary_from=T), dict(bins=[cut(0), cut(1)], canary_from=far),
                 [Access("out channel %d" % c, 1, LEAD, body, out_off[c], [b for b, _k in runs[c]]) for c in range(2)],
                 LEAD + body + 9 * (1 << 26) + (1 << 28))               # + one piece of the count as bool and as int64


CASES = [
    Case("unbin-far-out", "mhi_unbin_count / mhi_unbin_emit, CSR", "out_ticks past byte 2^32",
         "3 rows of a repeated 256-byte pattern, 2^29 + P events and more", unbin_far_out),
    Case("unbin-dense-group", "mhi_unbin_count / mhi_unbin_emit, CSR", "a group sum above 2^31, the scan's 16-bit halves at their largest",
         "2 rows of 1024 + 3 tiles, the first group all 255", unbin_dense_group),
    Case("unbin-csr-long-row", "mhi_unbin_count / mhi_unbin_emit, CSR", "a column >= 2^32 of one row",
         "2 rows of 2^32 + P columns of zeros with planted counts", unbin_csr_long_row),
    Case("unbin-aer-big-block", "mhi_unbin_count / mhi_unbin_emit, AER, 16- and 32-bit channels", "the flat element index >= 2^32 and f0 / cols",
         "cols = 1000, rows = 2^32 / 1000 + 4", unbin_aer_big_block),
    Case("aer-far-out", "mhi_aer_to_csr, 16-bit channels, C = 3", "positions >= 2^29",
         "n = 3 m pairs, channel 2 wholly behind byte 2^32 of out_ticks", aer_far_out),
    Case("windows-far-offsets", "mhi_windows: STACK 8-bit, STACK 32-bit with win_idx, SUM with sumsq; r = 1, 7, 100", "win_off >= 2^32",
         "2 rows of 2^32 + 2 P columns, 12 windows of 200", windows_far_offsets),
    Case("windows-many-items", "mhi_windows STACK 8-bit, r = 1, W = 1", "win_split's 64-bit branch: 2^32 + 65536 items",
         "65537 rows, 65536 windows", windows_many_items),
    Case("excess-cols-big-block", "mhi_excess_count / mhi_excess_emit, COLS", "t * C + c0 >= 2^32",
         "C = 1027, T = 2^32 / 1027 + 6", excess_cols_big_block),
    Case("bin-long-channel", "mhi_bin_events, 8 bits", "bin index and output byte >= 2^32",
         "C = 2, T = 2^32 + P bins, period 3", bin_long_channel),
]
BY_ID = {c.id: c for c in CASES}
