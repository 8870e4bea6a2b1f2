"""The launches of libmuahuff.so whose grid is capped, at shapes that cross the cap: the stride loop, the second launch
or the refusal that covers what the capped grid does not (the grids: csrc/mh_launch.hpp; DESIGN.md lists every capped launch).

    mh_rebin           more channels than 65535 grid rows (channel_rows; k_rebin2, k_rebin3);  a channel of more than 4096
                       tiles (rebin2_grid; k_rebin2)
    mh_synth_poisson   more channels than 65535 grid rows;  a channel of more than 4096 workgroups' samples (synth_grid; k_synth)
    mh_decode_range /  more than 65535 fill records: several launches (fill_grid_y);  one fill longer than what 1024
    mh_decode_rebin    workgroups zero in a pass (fill_grid_x; k_range_fill, k_rebin_fill)
    mh_deinterleave, mh_deinterleave_packed, mh_interleave, mh_interleave_packed   more than 65535 strips of 128 channels
                       are refused; 65535 strips are not (transposed_grid)

The grid a call launched cannot be read back from the device, so every test restates the rule it targets (its function
in csrc/mh_launch.hpp is named next to it) and asserts that its shape crosses it: a coverage guard, never an
expectation.  The functions themselves are read back off-device, at these shapes too, by
tests/test_host_launch_geometry.py.  When a rule changes in the header, the assertion here is the reminder to move the shape.

Every output lies in a buffer filled with a non-zero canary in front of, between and behind the channels or rows; the
WHOLE buffer is compared with the CPU reference, exactly.  A bin that no workgroup wrote shows as the canary.

Out of reach at test size: the x cap of k_rebin3 (65535 workgroups of 4 tiles of 32 KiB: a channel of more than 8 GiB).
Passing a max_len below the longest channel would reach it, but include/muahuff.h promises nothing for that.

Two shapes differ from a naive reading of their case, because mh_decode_range / mh_decode_rebin accept a range only up
to the plan's longest channel: the plan of 2 * 65535 + 3 short channels has ONE channel of 600 bins (its row is the only
one without a fill: 2 * 65535 + 2 fill records, launches of 65535, 65535 and 2), and the plan of three short channels
has a fourth that is as long as the query."""
import ctypes as ct

import numpy as np
import pytest
import torch

import oracle
from tests import helpers

pytestmark = pytest.mark.gpu

OC = oracle.c
YMAX = 65535                      # rows (y) of a grid
C_BIG = 2 * YMAX + 3              # three trips of a channel loop / three launches, the last one of three (two) only
EDGE_CH = (0, YMAX - 1, YMAX, YMAX + 1, 2 * YMAX - 1, 2 * YMAX, C_BIG - 1)    # first and last channel of every trip
TILE = 32768                      # kRebinTileBytes
CAN8, CAN32 = 0xA5, 0x5A5A5A5A
PAD = 64


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, container, synth  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    return muahuff


def _p(t):
    return ct.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _spread(counts):
    """channels of counts[c] elements laid end to end -> (channel, index inside its channel) of every element"""
    counts = np.asarray(counts, np.int64)
    ch = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    return ch, np.arange(int(counts.sum()), dtype=np.int64) - (np.cumsum(counts) - counts)[ch]


def _canary(shape, sat):
    """an output buffer of canaries: uint8 (saturating form) or int32"""
    return torch.full(shape, CAN8 if sat else CAN32, dtype=torch.uint8 if sat else torch.int32, device="cuda")


def _host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def _same(got, exp, tag):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (tag, got.shape, exp.shape, got.dtype, exp.dtype)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got.ravel() != exp.ravel())
        i = int(bad[0])
        pytest.fail("%r: %d of %d elements differ, the first at %d (row %d): got %#x, want %#x"
                    % (tag, bad.size, got.size, i, i // got.shape[-1], int(got.ravel()[i]), int(exp.ravel()[i])))


def _sums(x, r, sat):
    """np.add.reduceat over `x` in bins of r from element 0 (the last one may be cut)"""
    s = np.add.reduceat(x, np.arange(0, x.size, r, dtype=np.int64), dtype=np.uint32)
    return np.minimum(s, 255).astype(np.uint8) if sat else s


# ---- 1. mh_rebin, more channels than grid rows --------------------------------------------------------------------
R_MANY = (2, 3, 5, 7, 100)        # k_rebin2, k_rebin2, k_rebin3<., 5>, k_rebin3<., 0>, k_rebin3<., 100>


@pytest.mark.parametrize("r", R_MANY)
def test_rebin_more_channels_than_grid_rows(mh, r):
    C = C_BIG
    by = min(C, YMAX)                                   # channel_rows (mh_rebin): y = min(C, 65535)
    assert -(-C // by) == 3 and C - 2 * by == 3         # ch += gridDim.y: three trips, the last one of three workgroups
    rng = np.random.RandomState(100 + r)
    lens = rng.randint(1, 301, size=C).astype(np.int64)
    plant = (1, r - 1, r, r + 1, 299)
    for i, ch in enumerate(EDGE_CH):                    # every edge channel gets every planted length over the five r
        lens[ch] = plant[(i + R_MANY.index(r)) % len(plant)]
    assert lens.min() >= 1
    in_off, _, total = mh.container.layout(lens)
    in_off = in_off.astype(np.int64)
    host = rng.randint(0, 256, size=total + 16, dtype=np.uint8)     # the padding between channels is not zero either
    ch, j = _spread(lens)
    flat = host[in_off[ch] + j]                         # the channels end to end
    assert flat.max() == 255 and flat.min() == 0
    # reference: np.add.reduceat over `flat`, bin starts per channel
    nb = -(-lens // r)
    bch, bj = _spread(nb)
    exact = np.add.reduceat(flat, (np.cumsum(lens) - lens)[bch] + bj * r, dtype=np.uint32)
    assert exact.size == nb.sum() and (r < 3 or exact.max() > 255)
    gap = 1 + np.arange(C, dtype=np.int64) % 3          # canaries in front of every channel's bins
    out_off = PAD + np.cumsum(nb + gap) - nb
    size = int(out_off[-1] + nb[-1]) + PAD
    d_data, d_off, d_len, d_ooff = torch.from_numpy(host).cuda(), _dev(in_off), _dev(lens), _dev(out_off)
    for sat in (1, 0):
        out = _canary((size,), sat)
        mh._lib.check(mh._lib.lib().mh_rebin(_p(d_data), _p(d_off), _p(d_len), C, int(lens.max()), r, sat, _p(out),
                                             _p(d_ooff), None))
        exp = np.full(size, CAN8, np.uint8) if sat else np.full(size, CAN32, np.uint32)
        exp[out_off[bch] + bj] = np.minimum(exact, 255) if sat else exact
        _same(_host(out), exp, ("mh_rebin", r, sat))


# ---- 2. mh_rebin, one channel behind the tile clamp of k_rebin2 ---------------------------------------------------
def _long_len(r):
    """4096 + 2 tiles of k_rebin2, the last one cut, and 16 ragged bytes"""
    bins_per_tile = TILE // r
    return ((4096 + 1) * bins_per_tile + bins_per_tile // 3) * r + 16


SHORT = (5, 40000)                # behind the long channel: workgroups of a high blockIdx.x find nothing to do on them


@pytest.fixture(scope="module")
def long_channel():
    """random bytes for the long channel at offset 0 (as much as the longest case takes) and, behind them, for the two
    short ones: (host, device, offsets of the short channels)"""
    room = (max(_long_len(1), _long_len(3)) + 15) // 16 * 16 + 16
    offs = (room, room + 16)
    rng = np.random.RandomState(5)
    host = np.frombuffer(rng.bytes(offs[1] + SHORT[1] + 16), np.uint8)
    dev = torch.from_numpy(host.copy()).cuda()
    yield host, dev, offs
    del dev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("r,sat", [(3, 1), (3, 0), (1, 1)])     # r = 1 to uint32 is half a GiB and no other code path
def test_rebin_one_channel_behind_the_tile_clamp(mh, long_channel, r, sat):
    host, d_data, short_off = long_channel
    lens = np.array((_long_len(r),) + SHORT, np.int64)
    in_off = np.array((0,) + short_off, np.int64)
    assert in_off[1] >= lens[0]
    bins_per_tile = TILE // r                            # rebin2_grid (r < 4): x = ceil(ceil(max_len / r) / bins_per_tile)
    bx = -(-(-(-int(lens.max()) // r)) // bins_per_tile)
    assert bx == 4096 + 2 > 4096                         # ... clamped to 4096: b0 += gridDim.x * bins_per_tile, two tiles
    assert (-(-int(lens[0]) // r)) % bins_per_tile not in (0, bins_per_tile - 1) and lens[0] % 16   # the last tile is cut
    nb = -(-lens // r)
    assert nb[1] < bins_per_tile < nb[2] < 4096 * bins_per_tile
    out_off = PAD + np.cumsum(nb + 3) - nb
    size = int(out_off[-1] + nb[-1]) + PAD
    out = _canary((size,), sat)
    d_off, d_len, d_ooff = _dev(in_off), _dev(lens), _dev(out_off)
    mh._lib.check(mh._lib.lib().mh_rebin(_p(d_data), _p(d_off), _p(d_len), 3, int(lens.max()), r, sat, _p(out),
                                         _p(d_ooff), None))
    exp = np.full(size, CAN8, np.uint8) if sat else np.full(size, CAN32, np.uint32)
    for c in range(3):
        x = host[in_off[c]:in_off[c] + lens[c]]
        # bins of one byte are the bytes (no 134-million-entry index list for reduceat)
        exp[out_off[c]:out_off[c] + nb[c]] = x if r == 1 else _sums(x, r, sat)
    _same(_host(out), exp, ("mh_rebin", r, sat))


# ---- 3. mh_synth_poisson ------------------------------------------------------------------------------------------
def _synth(mh, lens, thr, seed):
    """mh_synth_poisson into a canary buffer laid out by container.layout with 16 more bytes in front of every channel
    (the layout leaves no gap behind a channel of a multiple of 16 bytes), against oracle.c.synth: the whole buffer"""
    lens = np.asarray(lens, np.int64)
    C = lens.size
    off, _, total = mh.container.layout(lens)
    off = off.astype(np.int64) + 16 * (1 + np.arange(C, dtype=np.int64))
    size = total + 16 * (C + 1) + PAD
    assert (off[1:] - (off + lens)[:-1] >= 16).all() and off[-1] + lens[-1] + PAD <= size
    buf = torch.full((size,), CAN8, dtype=torch.uint8, device="cuda")
    d_thr = torch.from_numpy(np.ascontiguousarray(thr, np.uint32).view(np.int32)).cuda()
    d_off, d_len = _dev(off), _dev(lens)
    mh._lib.check(mh._lib.lib().mh_synth_poisson(_p(buf), _p(d_off), _p(d_len), C, int(lens.max()), _p(d_thr), seed, None))
    want = OC.synth(off, lens, thr, seed, total=size, nthreads=8)
    edge = np.zeros(size + 1, np.int8)
    edge[off] = 1
    edge[off + lens] = -1
    inside = np.cumsum(edge[:size], dtype=np.int8) > 0
    assert inside.sum() == lens.sum()
    exp = np.where(inside, want, np.uint8(CAN8))
    _same(buf.cpu().numpy(), exp, ("mh_synth_poisson", C))
    return want[inside]


def test_synth_one_channel_behind_the_workgroup_clamp(mh):
    lens = [4096 * 4096 + 5 * 4096 + 7, 1, 15, 16, 17, 4097]
    bx = -(-max(lens) // (256 * 16))                     # synth_grid: x = ceil(max_len / 4096) ...
    assert bx == 4096 + 6 > 4096                         # ... clamped to 4096: pc += gridDim.x * 256, six workgroups, a cut piece
    thr = mh.synth.thresholds(mh.synth.channel_rates(len(lens), 0.3, 3.0))
    x = _synth(mh, lens, thr, 11)
    assert 0.2 < x.mean() < 4.0 and x.max() >= 5


def test_synth_more_channels_than_grid_rows(mh):
    C = C_BIG
    by = min(C, YMAX)                                    # channel_rows (mh_synth_poisson): y = min(C, 65535)
    assert -(-C // by) == 3 and C - 2 * by == 3          # ch += gridDim.y
    lens = np.random.RandomState(8).randint(1, 41, size=C)
    lens[list(EDGE_CH)] = (1, 15, 16, 17, 40, 33, 1)
    thr = mh.synth.thresholds(mh.synth.channel_rates(C, 0.3, 3.0))
    x = _synth(mh, lens, thr, 12)
    assert 0.2 < x.mean() < 4.0


# ---- 4 and 5. the zero fills of mh_decode_range and mh_decode_rebin ----------------------------------------------
_streams = {}


def _stream(mh, key, lens, S, rate):
    """channels of Poisson counts (lengths `lens`), a plan over them with whole-channel windows, and the GPU's own
    encode of them compacted to a dense stream: (plan, Encoded, the counts end to end); kept for the module under `key`"""
    if key not in _streams:
        lens = np.asarray(lens, np.int64)
        rng = np.random.default_rng(S + lens.size)
        flat = np.minimum(rng.poisson(rate, size=int(lens.sum())), 255).astype(np.uint8)
        assert (flat >= S).any()                                    # the decoder's clip at S - 1 shows
        off, ln, total = mh.container.layout(lens)
        host = np.zeros(total + 16, np.uint8)
        ch, j = _spread(lens)
        host[off.astype(np.int64)[ch] + j] = flat
        data = torch.from_numpy(host).cuda()
        plan = mh.codec.Plan(off, ln, S, 6, mh.MODE_APPROX, mh.WIN_FULL, helpers.sclv_tables()[S])
        d, _ = plan.compact(plan.encode(data))
        torch.cuda.synchronize()
        _streams[key] = (plan, d, flat, lens)
    return _streams[key]


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for plan, *_ in _streams.values():
        plan.close()
    _streams.clear()
    torch.cuda.empty_cache()


def _rows(flat, lens, S, a, b):
    """the reference: min(x, S - 1) of samples [a, b) of every channel, zero-extended"""
    ch, j = _spread(lens)
    keep = (j >= a) & (j < b)
    rows = np.zeros((lens.size, b - a), np.uint8)
    rows[ch[keep], j[keep] - a] = np.minimum(flat[keep], S - 1)
    return rows


def _framed(nrows, n, lead, trail, sat):
    """a canary buffer of nrows + 2 rows and its view of nrows x n behind `lead` canaries in rows 1 .. nrows"""
    buf = _canary((nrows + 2, lead + n + trail), sat)
    return buf, buf[1:-1, lead:lead + n]


def _check_framed(buf, rows, lead, tag):
    exp = np.full(tuple(buf.shape), CAN8 if rows.dtype == np.uint8 else CAN32, rows.dtype)
    exp[1:-1, lead:lead + rows.shape[1]] = rows
    _same(_host(buf), exp, tag)


def _range_and_rebin(plan, d, rows, a, b, r, tag):
    """mh_decode_range of [a, b) on all channels, then mh_decode_rebin of it with r to uint8 and int32: whole buffers"""
    C, n = rows.shape
    assert a % r == 0 and n % r == 0        # rows of whole bins: one reduceat runs over all of them
    buf, view = _framed(C, n, 7, 6, True)
    assert (view.data_ptr() + view.stride(0)) % 16        # row 1 starts off a 16-byte boundary
    plan.decode_range(d.payload, d.seg_off, d.peak, d.enc, None, a, b, out=view)
    assert plan.decode_ok()
    _check_framed(buf, rows, 7, tag + ("range",))
    del buf, view
    for sat in (True, False):
        buf, view = _framed(C, n // r, 3, 2, sat)
        plan.decode_rebin(d.payload, d.seg_off, d.peak, d.enc, None, a, b, r, saturate=sat, out=view)
        assert plan.decode_ok()
        _check_framed(buf, _sums(rows.ravel(), r, sat).reshape(C, n // r), 3, tag + ("rebin", sat))
        del buf, view


def _many_lens():
    lens = np.random.RandomState(21).randint(1, 401, size=C_BIG).astype(np.int64)
    lens[list(EDGE_CH)] = (1, 400, 255, 256, 257, 399, 1)
    lens[70000] = 600               # a range may reach as far as the longest channel: this one makes [., 512) a query
    return lens


@pytest.mark.parametrize("S,a,b", [(3, 0, 512), (3, 256, 512), (10, 0, 512)])
def test_fill_records_in_more_than_one_launch(mh, S, a, b):
    plan, d, flat, lens = _stream(mh, ("many", S), _many_lens(), S, 1.2 if S == 3 else 5.0)
    # walk_query (csrc/mh_worklist.hpp): one record for a row wholly behind its channel's end, one behind the data of a
    # row that ends inside the range; fill_grid_y: 65535 records per launch
    nfill = int((lens <= a).sum() + ((lens > a) & (lens < b)).sum())
    assert nfill == 2 * YMAX + 2 and -(-nfill // YMAX) == 3          # launches of 65535, 65535 and 2 records
    assert (lens <= a).sum() > (YMAX if a else -1) and (lens[YMAX:] > a).any()
    _range_and_rebin(plan, d, _rows(flat, lens, S, a, b), a, b, 4, (S, a, b))


RANGE_STOP = 1024 * 16384 + 3 * 4096 + 5
REBIN_R = 4
REBIN_STOP = REBIN_R * (1024 * 4096 + 3 * 256 + 5)
ONE_FILL_LENS = (100, 40000, 16384 + 64, RANGE_STOP + 11)    # the last one makes the ranges queries; it is decoded too


def test_one_range_fill_behind_the_workgroup_clamp(mh):
    plan, d, flat, lens = _stream(mh, "one", ONE_FILL_LENS, 3, 1.2)
    a, b = 0, RANGE_STOP
    max_fill = b - int(lens.min())
    nx = -(-max_fill // (256 * 16 * 4))                  # fill_grid_x(max_fill, 256 * 16 * 4) of mh_decode_range
    assert nx > 1024                                     # ... clamped to 1024: i += gridDim.x * 256 in k_range_fill
    assert 0 < -(-max_fill // 16) % (1024 * 256) <= 4 * 256      # the last pass is taken by a few workgroups only
    rows = _rows(flat, lens, 3, a, b)
    buf, view = _framed(len(lens), b - a, 7, 38, True)
    assert view.stride(0) % 16 and (view.data_ptr() + view.stride(0)) % 16     # byte-wise head and tail pieces of the fills
    plan.decode_range(d.payload, d.seg_off, d.peak, d.enc, None, a, b, out=view)
    assert plan.decode_ok()
    _check_framed(buf, rows, 7, ("range", a, b))


@pytest.mark.parametrize("sat", [True, False])
def test_one_rebin_fill_behind_the_workgroup_clamp(mh, sat):
    plan, d, flat, lens = _stream(mh, "one", ONE_FILL_LENS, 3, 1.2)
    a, b, r = 0, REBIN_STOP, REBIN_R
    nb = (b - a) // r
    max_fill = nb - -(-int(lens.min()) // r)
    nx = -(-max_fill // (256 * 16))                      # fill_grid_x(max_fill, 256 * 16) of mh_decode_rebin
    assert nx > 1024                                     # ... clamped to 1024: i += gridDim.x * 256 in k_rebin_fill
    assert 0 < max_fill % (1024 * 256) <= 4 * 256
    rows = _sums(_rows(flat, lens, 3, a, b).ravel(), r, sat).reshape(len(lens), nb)
    buf, view = _framed(len(lens), nb, 3, 2, sat)
    plan.decode_rebin(d.payload, d.seg_off, d.peak, d.enc, None, a, b, r, saturate=sat, out=view)
    assert plan.decode_ok()
    _check_framed(buf, rows, 3, ("rebin", sat))


# ---- 6. the layout calls refuse more than 65535 strips ------------------------------------------------------------
STRIP = 128                       # kTr2C: channels of a strip


def test_layout_calls_refuse_more_than_65535_strips(mh):
    lib, L = mh._lib.lib(), mh._lib
    T, C = 1, YMAX * STRIP + 1
    assert -(-C // STRIP) == YMAX + 1                    # transposed_grid: strips = ceil(C / 128); above 65535: MH_ERR_ARG (all four calls)
    # real buffers and offsets: a call that wrongly went ahead would stay inside them
    rng = np.random.RandomState(6)
    src = torch.from_numpy(rng.randint(0, 256, size=16 * C + PAD, dtype=np.uint8)).cuda()
    dst = torch.full((16 * C + PAD,), CAN8, dtype=torch.uint8, device="cuda")
    off1, off16 = _dev(np.arange(C)), _dev(16 * np.arange(C))
    calls = [("mh_deinterleave", lambda: lib.mh_deinterleave(_p(src), T, C, _p(dst), _p(off1), None)),
             ("mh_deinterleave_packed", lambda: lib.mh_deinterleave_packed(_p(src), T, C, 2, _p(dst), _p(off16), 0, None)),
             ("mh_deinterleave_packed", lambda: lib.mh_deinterleave_packed(_p(src), T, C, 4, _p(dst), _p(off16), 0, None)),
             ("mh_interleave", lambda: lib.mh_interleave(_p(src), _p(off1), T, C, _p(dst), None)),
             ("mh_interleave_packed", lambda: lib.mh_interleave_packed(_p(src), _p(off16), T, C, 2, 0, _p(dst), None)),
             ("mh_interleave_packed", lambda: lib.mh_interleave_packed(_p(src), _p(off16), T, C, 4, 0, _p(dst), None))]
    for name, call in calls:
        assert call() == L.ERR_ARG, name
        assert lib.mh_last_error().startswith(name.encode() + b":"), (name, lib.mh_last_error())
        torch.cuda.synchronize()
        assert bool((dst == CAN8).all()), name


def test_layout_calls_accept_65535_strips(mh):
    lib, L = mh._lib.lib(), mh._lib
    T, C = 1, YMAX * STRIP
    assert -(-C // STRIP) == YMAX                        # the largest accepted strip count
    x = np.random.RandomState(7).randint(0, 256, size=(T, C), dtype=np.uint8)
    off = PAD + 3 * np.arange(C, dtype=np.int64)         # two canaries between the one-byte channels
    d_x, d_off = torch.from_numpy(x).cuda(), _dev(off)
    cm = torch.full((PAD + 3 * C + PAD,), CAN8, dtype=torch.uint8, device="cuda")
    L.check(lib.mh_deinterleave(_p(d_x), T, C, _p(cm), _p(d_off), None))
    exp = np.full(cm.numel(), CAN8, np.uint8)
    exp[off] = x[0]
    _same(cm.cpu().numpy(), exp, "mh_deinterleave")
    tm = torch.full((PAD + T * C + PAD,), CAN8, dtype=torch.uint8, device="cuda")
    L.check(lib.mh_interleave(_p(cm), _p(d_off), T, C, ct.c_void_p(tm.data_ptr() + PAD), None))
    exp = np.full(tm.numel(), CAN8, np.uint8)
    exp[PAD:PAD + T * C] = x.ravel()
    _same(tm.cpu().numpy(), exp, "mh_interleave")
