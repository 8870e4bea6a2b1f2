"""libmuahuff_ingest.so past the first trip of its loops: the single-workgroup scan that mhi_unbin_count and both forms of
mhi_excess_count share, and the capped grids of mhi_excess_apply.  Written against the ABI (include/muahuff_ingest.h)
with the harnesses of tests/test_gpu_unbin.py and tests/test_gpu_excess.py: ev_off / exc_off, total, over, the ticks or
(pos, val) sit in canary-framed buffers that are compared WHOLE, the scratch starts as garbage with a guard behind it,
the inputs are framed by 255s and start at odd bytes.

The rules, restated (the fixture checks the source text):
    scan    k_unbin_group_sum sums groups of 1024 pieces (kUnbinGroup: a piece is a tile of 16384 bytes of a CSR / ROWS row,
            or a cell of 512 time steps (kExcessTileT) of one channel of a COLS block).  k_unbin_scan (csrc/mh_unbin.hpp) is
            ONE workgroup of 1024 threads (kUnbinScanThreads) that walks the group sums in trips of 1024 groups and hands a
            `carry` from trip to trip: the second trip begins at piece TRIP = 2^20, the third at 2 * TRIP.
    apply   r == 1 (k_excess_apply1; excess_apply1_grid in csrc/mh_launch.hpp): x = min(ceil(n_entries / 256), 64),
            y = min(n_rows, 65535); the kernel strides i += gridDim.y and e += gridDim.x * 256.
            r > 1 (k_excess_apply; excess_apply_grid): min(ceil(n_rows * runs / 256), 2^20) workgroups over runs of 32
            elements; the kernel strides job += gridDim.x * 256.
The grid or the trip a call took cannot be read back from the device, so every case first asserts that its shape crosses
what it targets -- a coverage guard, never an expectation -- and that every trip holds entries.

Scan cases.  R3 = 2 * TRIP + 7 * 1024 + 5 pieces are 2056 groups: three trips, the last group of 5 pieces.  The inputs are
sparse (about 3 % counts of 1..3, about 2 % entries), with planted events or entries in pieces 0, TRIP - 1, TRIP,
2 * TRIP - 1, 2 * TRIP and the last one (those that exist).  The other 1023 pieces of group 1024 -- the first group of the
second trip -- are empty and group 1025 is not, so the base of piece TRIP and ev_off / exc_off there are exactly the carry
of the first trip, and the rest of the group sits at the carry plus the planted piece's count.  The yardstick is NumPy on
the input itself: np.nonzero in channel-major order, np.bincount for the index, np.repeat for the ticks.
With the carry dropped (`carry += all` removed) total, the entry behind the index and every base from piece TRIP on come
out too small: in every scan case `total` differs first in the order check() compares, then ev_off / exc_off from
channel (or row) TRIP / per_channel on, then the ticks / (pos, val), whose second-trip entries land on the first trip's.

(Seen once with such a build: all five scan cases fail at `total`, 0 against 1 991 081 in the largest CSR case.)

The r > 1 case past 2^20 workgroups takes 0.35 s on the MI355X and stays.  Out of reach: the AER form of the un-binner,
which shares the scan with the CSR form and reaches 2^20 tiles only with 16 GiB of input."""
import ctypes as ct
import importlib
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_excess as ex
from tests import test_gpu_unbin as ub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = ex.PAD
GROUP = 1024                      # pieces per group (kUnbinGroup)
SCAN = 1024                       # groups per trip of k_unbin_scan (kUnbinScanThreads)
TRIP = GROUP * SCAN               # pieces per trip
R3 = 2 * TRIP + 7 * GROUP + 5     # three trips; the last group holds 5 pieces
TILE, TILE_T = 16384, 512         # bytes of a CSR / ROWS tile, time steps of a COLS cell
YMAX = 65535                      # grid rows of k_excess_apply1 (kGridMaxY)
APPLY1_X = 64                     # its workgroups in x (kApply1MaxX)
APPLY_THREADS, APPLY_RUN = 256, 32
APPLY_MAX_BLOCKS = 1 << 20        # workgroups of k_excess_apply (kApplyMaxBlocks)
LEAD_BYTES, GAP = 65, 3           # a row input: 65 bytes of 255, then rows of `cols` bytes with 3 bytes of 255 between


@pytest.fixture(scope="module")
def mh():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()
    import muahuff
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    csrc = os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("mh_unbin_layout.hpp", "mh_unbin.hpp", "mh_excess_layout.hpp", "mh_launch.hpp")}
    assert "kUnbinGroup = 1024;" in text["mh_unbin_layout.hpp"] and "kUnbinScanThreads = 1024;" in text["mh_unbin.hpp"]
    assert "kExcessTileT = 512;" in text["mh_excess_layout.hpp"]             # the rules restated above are the headers'
    assert "kApplyRun = 32;" in text["mh_excess_layout.hpp"] and "kApplyThreads = 256;" in text["mh_excess_layout.hpp"]
    assert "kApplyMaxBlocks = 1u << 20;" in text["mh_excess_layout.hpp"]
    assert "kApply1MaxX = 64;" in text["mh_launch.hpp"] and "kGridMaxY = 65535;" in text["mh_launch.hpp"]
    return muahuff


def _ceil(a, b):
    return -(-a // b)


def _up16(n):
    return (n + 15) // 16 * 16


def scratch_of(pieces):
    """the scratch of `pieces` pieces (csrc/mh_unbin_layout.hpp, mh_excess_layout.hpp): u32 sums, u64 bases, u64 partials"""
    return _up16(4 * pieces) + _up16(8 * pieces) + _up16(8 * (_ceil(pieces, GROUP) + 1))


def planted(pieces):
    """the pieces on either side of every trip's edge, and the last one"""
    return sorted({p for p in (0, TRIP - 1, TRIP, 2 * TRIP - 1, 2 * TRIP, pieces - 1) if p < pieces})


def crosses(pieces, trips, per_piece):
    """the coverage guard of a scan case: more groups than trips - 1 trips hold, and entries in every trip"""
    groups = _ceil(pieces, GROUP)
    assert groups > (trips - 1) * SCAN and _ceil(groups, SCAN) == trips
    assert per_piece.size == pieces
    held = [int(per_piece[k * TRIP:(k + 1) * TRIP].sum()) for k in range(trips)]
    assert min(held) > 0, held
    for p in planted(pieces):
        assert per_piece[p] > 0, p
    if pieces > TRIP + GROUP:            # group 1024 is empty behind its first piece, group 1025 is not
        assert not per_piece[TRIP + 1:TRIP + GROUP].any() and per_piece[TRIP + GROUP:TRIP + 2 * GROUP].any()
    return held


class RowBlock:
    """x [rows, cols] inside a device buffer of 255s: row i begins at byte 65 + i * (cols + 3) -- an odd pitch, so the rows
    start at every offset modulo 16 -- with three bytes of 255 between the rows"""

    def __init__(self, x):
        rows, cols = x.shape
        pitch = cols + GAP
        assert pitch % 2 == 1
        body = np.full((rows, pitch), 255, np.uint8)
        body[:, :cols] = x
        host = np.concatenate([np.full(LEAD_BYTES, 255, np.uint8), body.reshape(-1), np.full(64, 255, np.uint8)])
        self.buf = torch.from_numpy(host).cuda()
        self.row_off = torch.from_numpy(LEAD_BYTES + np.arange(rows, dtype=np.int64) * pitch).cuda()
        self.rows, self.cols = rows, cols


def sparse(rng, n, rate, lo, hi, fill=None):
    """n bytes: `fill` (default zeros), about rate * n of them replaced by values in [lo, hi)"""
    x = np.zeros(n, np.uint8) if fill is None else np.tile(np.asarray(fill, np.uint8), n // len(fill) + 1)[:n]
    k = int(n * rate)
    x[rng.randint(0, n, k)] = rng.randint(lo, hi, k)
    return x


# ---- mhi_unbin_count + mhi_unbin_emit, CSR form ----------------------------------------------------------------------
def csr_yardstick(x, origin, period, phase):
    """x [rows, cols] uint8 -> (ticks uint64, ev_off uint64 [rows + 1], events per row)"""
    r, c = np.nonzero(x)                                             # row-major: channel-major, ascending in time
    k = x[r, c]
    ticks = np.repeat(np.uint64(origin + phase) + c.astype(np.uint64) * np.uint64(period), k)
    per_row = np.bincount(r, weights=k, minlength=x.shape[0]).astype(np.int64)
    off = np.zeros(x.shape[0] + 1, np.uint64)
    off[1:] = np.cumsum(per_row)
    return ticks, off, per_row


@pytest.mark.parametrize("rows,trips", [(R3, 3), (TRIP + 1, 2)], ids=["three_trips", "second_trip_of_one_piece"])
def test_unbin_csr_scan_carry(mh, rows, trips):
    cols = 16
    pieces = rows * _ceil(cols, TILE)                               # one tile per row
    assert pieces == rows and mh._ingest.unbin_scratch_bytes(ub.CSR, rows, cols) == scratch_of(pieces)
    rng = np.random.RandomState(rows % 1000)
    x = sparse(rng, rows * cols, 0.03, 1, 4).reshape(rows, cols)
    x[TRIP:TRIP + GROUP] = 0
    for p in planted(pieces):
        x[p, 0], x[p, cols - 1] = 2, 255                            # the first and the last byte of the row
    origin, period, phase = 1 << 40, 30, 7
    want, off, per_row = csr_yardstick(x, origin, period, phase)
    held = crosses(pieces, trips, per_row)
    assert int(off[TRIP]) == held[0] == int(x[:TRIP].sum(dtype=np.int64))        # ev_off[TRIP] is the first trip's carry
    assert 10 ** 6 / 2 < want.size < 10 ** 7
    inp = RowBlock(x)
    o = ub.Out(mh, ub.CSR, rows, cols, want.size)
    o.call(mh, inp.buf, inp.row_off, origin, period, phase)
    o.check(want, off, tag=("csr", rows))


# ---- mhi_excess_count + mhi_excess_emit ------------------------------------------------------------------------------
def test_excess_rows_scan_carry(mh):
    rows, cols, thr = R3, 16, 2
    pieces = rows * _ceil(cols, TILE)
    assert pieces == rows and mh._ingest.excess_scratch_bytes(ex.ROWS, rows, cols) == scratch_of(pieces)
    rng = np.random.RandomState(12)
    x = sparse(rng, rows * cols, 0.02, thr + 1, 256, fill=[0, 1, 2]).reshape(rows, cols)
    hi = rng.randint(1, cols + 1, rows).astype(np.int64)            # ragged windows [0, hi)
    x[TRIP:TRIP + GROUP] = 1
    for p in planted(pieces):
        hi[p] = cols - 3
        x[p, 0], x[p, cols - 4] = 255, thr + 1                      # the first and the last sample of the window
    inside = np.arange(cols)[None, :] < hi[:, None]
    x[~inside] = 255                                                # what a read behind the window would find
    r, c = np.nonzero((x > thr) & inside)
    per_row = np.bincount(r, minlength=rows)
    off = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int64)
    want = (off, c.astype(np.int64), x[r, c].astype(np.int64) - thr)
    held = crosses(pieces, 3, per_row)
    assert int(off[TRIP]) == held[0] and int(off[2 * TRIP]) == held[0] + held[1]
    assert 10 ** 5 < c.size < 10 ** 7
    inp = RowBlock(x)
    o = ex.Out(mh, ex.ROWS, rows, cols, c.size)
    o.call(mh, inp.buf, inp.row_off, None, torch.from_numpy(hi).cuda(), thr)
    torch.cuda.synchronize()
    o.check(want, tag="ROWS R3")


def cols_yardstick(X, thr):
    """X [T, C] uint8 time-major -> ((exc_off, pos, val), t, c of every entry in list order)"""
    t, c = np.nonzero(X > thr)
    order = np.argsort(c, kind="stable")                             # channel-major; t stays ascending inside a channel
    t, c = t[order], c[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=X.shape[1]))]).astype(np.int64)
    return (off, t.astype(np.int64), X[t, c].astype(np.int64) - thr), t, c


@pytest.mark.parametrize("T,C,trips", [(3, R3, 3), (TILE_T + 1, (1 << 19) + 512 + 3, 2)], ids=["one_cell_per_channel", "two_cells_per_channel"])
def test_excess_cols_scan_carry(mh, T, C, trips):
    thr = 2
    per_channel = _ceil(T, TILE_T)
    pieces = C * per_channel                                         # piece = channel * per_channel + time tile
    assert mh._ingest.excess_scratch_bytes(ex.COLS, T, C) == scratch_of(pieces)
    assert (per_channel, _ceil(C, ex.STRIP), _ceil(pieces, GROUP)) == ((1, 8221, 2056) if T == 3 else (2, 2051, 1026))
    rng = np.random.RandomState(T)
    X = sparse(rng, T * C, 0.02, thr + 1, 256, fill=[0, 1, 2]).reshape(T, C)
    X[:, TRIP // per_channel:(TRIP + GROUP) // per_channel] = 1
    for p in planted(pieces):
        ch, t0 = p // per_channel, p % per_channel * TILE_T
        X[t0, ch], X[min(t0 + TILE_T, T) - 1, ch] = thr + 1, 255    # the first and the last step of the cell (one and the same, perhaps)
    want, t, c = cols_yardstick(X, thr)
    held = crosses(pieces, trips, np.bincount(c * per_channel + t // TILE_T, minlength=pieces))
    assert int(want[0][TRIP // per_channel]) == held[0]              # exc_off at the second trip's first channel is the carry
    assert 10 ** 5 < t.size < 10 ** 7
    # the canary frame in front of the block makes its first byte odd-aligned for odd PAD
    buf = torch.full((PAD + T * C + PAD,), 255, dtype=torch.uint8, device="cuda")
    buf[PAD:PAD + T * C] = torch.from_numpy(X.reshape(-1)).cuda()
    o = ex.Out(mh, ex.COLS, T, C, t.size)
    o.call(mh, buf[PAD:], None, None, None, thr)
    torch.cuda.synchronize()
    o.check(want, tag="COLS %dx%d" % (T, C))


# ---- mhi_excess_apply across its caps --------------------------------------------------------------------------------
def channel_list(rng, K, T, rate, vmax, always=()):
    """a canonical list of K channels of T samples, entries at the samples `always` in every channel ->
    (exc_off, pos, val, channel of every entry)"""
    mask = rng.rand(K, T) < rate
    mask[:, list(always)] = True
    c, p = np.nonzero(mask)
    off = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=K))]).astype(np.int64)
    return off, p.astype(np.int64), rng.randint(1, vmax + 1, p.size), c


def apply_ref_rows_of_channels(base, pos, val, ch, sel, n_ch, start, stop, lead, bits):
    """ex.apply_ref for r == 1 where row i takes the whole list of channel sel[i], vectorised: np.add.at per channel"""
    add = np.zeros((n_ch, base.shape[1]), np.int64)
    keep = (pos >= start) & (pos < stop)
    np.add.at(add, (ch[keep], pos[keep] - start + lead), val[keep])
    out = base + add[sel]
    return np.minimum(out, 255) if bits == 8 else out


def compare_whole(tgt, want):
    got = tgt.buf.cpu().numpy()
    bad = np.nonzero(got != tgt.expect(want))[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]) - tgt.first, bad.size)


@pytest.mark.parametrize("layout", ["channel-major", "time-major"])
@pytest.mark.parametrize("bits", [8, 32])
def test_apply1_more_rows_than_grid_rows(mh, layout, bits):
    """r == 1 with 2 * 65535 + 3 rows: three trips of i += gridDim.y, the last of three rows"""
    n_rows, K, T = 2 * YMAX + 3, 1000, 40
    start, stop, lead = 9, 31, 2
    elements = stop - start + lead
    assert n_rows > YMAX and elements == 24
    rng = np.random.RandomState(bits)
    off, pos, val, ch = channel_list(rng, K, T, 0.3, 254, always=(start - 1, start, stop - 1, stop))      # [start, stop) cuts every channel
    sel = np.arange(n_rows) % K
    first, last = off[sel], off[sel + 1]
    tgt = ex.Target(layout, n_rows, elements, bits, rng)
    want = apply_ref_rows_of_channels(tgt.base, pos, val, ch, sel, K, start, stop, lead, bits)
    edge = np.array([0, YMAX - 1, YMAX, YMAX + 1, 2 * YMAX - 1, 2 * YMAX, n_rows - 1])
    assert (want[edge] != tgt.base[edge]).any(axis=1).all()          # the first and last row of every trip receive an entry
    assert np.array_equal(want[edge], ex.apply_ref(tgt.base[edge], pos, val, first[edge], last[edge], start, stop, 1, lead, bits))
    if bits == 8:                                                    # it does saturate
        assert (apply_ref_rows_of_channels(tgt.base, pos, val, ch, sel, K, start, stop, lead, 32) > 255).any()
    ex.run_apply(mh, tgt, pos, val, first, last, start, stop, 1, lead, bits)
    torch.cuda.synchronize()
    compare_whole(tgt, want)


@pytest.mark.parametrize("bits", [8, 32])
def test_apply1_a_row_of_more_entries_than_the_threads_of_a_grid_row(mh, bits):
    """r == 1, rows of about 30000 entries against 64 x 256 threads: e += gridDim.x * 256 runs twice"""
    C, T, start, stop = 3, 60100, 50, 60050
    rng = np.random.RandomState(40 + bits)
    off, pos, val = ex.sorted_list(rng, C, T, 0.5, 254)
    assert stop - start == 60000 and _ceil(len(pos), APPLY_THREADS) > APPLY1_X
    assert (np.diff(off) > APPLY1_X * APPLY_THREADS).all()          # every row, even cut to [start, stop), has more than 16384
    assert ((pos >= start) & (pos < stop))[off[0]:off[1]].sum() > APPLY1_X * APPLY_THREADS
    tgt = ex.Target("pitched", C, stop - start, bits, rng)
    want = ex.apply_ref(tgt.base, pos, val, off[:-1], off[1:], start, stop, 1, 0, bits)
    ex.run_apply(mh, tgt, pos, val, off[:-1], off[1:], start, stop, 1, 0, bits)
    torch.cuda.synchronize()
    compare_whole(tgt, want)


def test_apply_more_runs_than_the_capped_grid_holds(mh):
    """r = 2 with one element (one run) per row and 2^28 + 1000 rows: job += gridDim.x * 256 runs a second time for the
    last 1000 rows.  first / last and the expectation are built on the device (4.3 GB of indices, no host copy)."""
    n_rows, r, start, stop, lead = (1 << 28) + 1000, 2, 2, 4, 0
    elements = _ceil(stop - start + lead, r)
    runs = _ceil(elements, APPLY_RUN)
    assert elements == 1 and _ceil(n_rows * runs, APPLY_THREADS) > APPLY_MAX_BLOCKS
    K, T = 1000, 6
    assert (APPLY_MAX_BLOCKS * APPLY_THREADS) % K != 0               # a job and the one a stride behind it take different channels
    rng = np.random.RandomState(28)
    off, pos, val, ch = channel_list(rng, K, T, 0.5, 200)
    empty = np.diff(off) == 0
    assert empty.any() and not empty.all() and (pos < start).any() and (pos >= stop).any()
    keep = (pos >= start) & (pos < stop)
    add = np.zeros(K, np.int64)
    np.add.at(add, ch[keep], val[keep])                              # the one element of a row: its channel's entries at 2 and 3
    assert (add > 255).any() and (add == 0).any()
    d_off, d_add = torch.from_numpy(off).cuda(), torch.from_numpy(add.astype(np.int16)).cuda()
    sel = torch.arange(n_rows, dtype=torch.int64, device="cuda") % K
    first, last = d_off[sel], d_off[sel + 1]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(28)
    base = torch.randint(0, 4, (n_rows,), dtype=torch.uint8, device="cuda", generator=gen)
    want = (base.to(torch.int16) + d_add[sel]).clamp_(max=255).to(torch.uint8)
    del sel
    tail = slice(APPLY_MAX_BLOCKS * APPLY_THREADS, n_rows)            # the rows of the second pass
    assert bool((want[tail] != base[tail]).any())
    buf = torch.full((PAD + n_rows + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    buf[PAD:PAD + n_rows] = base
    d_pos = torch.from_numpy(pos.astype(np.uint32).view(np.int32)).cuda()
    d_val = torch.from_numpy(val.astype(np.uint8)).cuda()
    L = mh._ingest.lib()
    p = lambda t, skip=0: ct.c_void_p(t.data_ptr() + skip)   # noqa: E731
    rc = L.mhi_excess_apply(p(d_pos), p(d_val), len(pos), p(first), p(last), n_rows, start, stop, r, lead, p(buf, PAD), 8, 1, 1,
                            ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.mhi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[PAD:PAD + n_rows], want)
    assert bool((buf[:PAD] == 0x5A).all()) and bool((buf[PAD + n_rows:] == 0x5A).all())
