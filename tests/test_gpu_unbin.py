"""mhi_unbin_count / mhi_unbin_emit (include/muahuff_ingest.h) on the GPU, and the entry points built on them:
EventSet.from_counts, events.aer_from_counts, archive.Reader.read_events.

The oracle of every case is NumPy, compared entry for entry:
  CSR form   np.repeat(origin + np.arange(T)*period + phase, x[c]) per channel, back to back
  AER form   t, c = np.nonzero(X) (row-major), repeated by X[t, c]
out_ticks, out_ch, ev_off, total and over sit inside canary-filled buffers that are compared WHOLE after every call:
nothing outside [0, total) may change.  The rows of a CSR input are separated by bytes of 255 and start at byte offsets
0, 3 and 7 modulo 16, so that a read past a row's end -- or before its start -- shows up as extra events.  The scratch
starts as garbage every time.

The tile rule, restated from csrc/mh_unbin_layout.hpp: a wave reads 1 KiB per load (16 bytes per lane), a tile is 16 such
wave rows = 16384 bytes of one contiguous span, owned by one wave in either pass; a CSR row is cut into ceil(cols / 16384)
tiles, the AER block is cut flat.  A wave stages 2048 events in LDS before it stores them; 1024 tiles make a group of the
scan.  The sizes below lie around every one of these steps."""
import ctypes as ct
import importlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A5A5A5A5A5A5A5A
CAN32 = 0x5A5A5A5A
PAD = 67
GUARD = 4096
SCRATCH_FILL = 0xC3
CSR, AER = 0, 1
TILE = 16384
GROUP = 1024
STAGE = 2048
ROW_STARTS = (0, 3, 7)


@pytest.fixture(scope="module")
def mh():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()
    import muahuff
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    src = open(os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc", "mh_unbin_layout.hpp")).read()
    assert "kUnbinRowBytes = 1024;" in src and "kUnbinTileRows = 16;" in src and "kUnbinGroup = 1024;" in src
    assert "kUnbinStage = 2048;" in src           # the rule restated above is the header's
    return muahuff


# ---- the yardsticks ----------------------------------------------------------------------------------------------
def csr_oracle(x, origin, period, phase):
    """x: [C, T] uint8 -> (ticks uint64, ev_off uint64 [C + 1])"""
    T = x.shape[1]
    t = np.uint64(origin) + np.arange(T, dtype=np.uint64) * np.uint64(period) + np.uint64(phase)
    per = [np.repeat(t, x[c]) for c in range(x.shape[0])]
    off = np.zeros(x.shape[0] + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in per])
    return np.concatenate(per), off


def aer_oracle(X, origin, period, phase):
    """X: [T, C] uint8 -> (ticks uint64, channels int64)"""
    t, c = np.nonzero(X)
    k = X[t, c]
    ticks = np.uint64(origin) + t.astype(np.uint64) * np.uint64(period) + np.uint64(phase)
    return np.repeat(ticks, k), np.repeat(c, k)


class CsrInput:
    """x [rows, cols] inside a device buffer of 255s, row i at a byte offset congruent to ROW_STARTS[(i + turn) % 3] mod 16"""

    def __init__(self, x, turn=0):
        rows, cols = x.shape
        pitch = (cols + 15) // 16 * 16 + 48
        off = np.array([64 + i * pitch + ROW_STARTS[(i + turn) % 3] for i in range(rows)], np.int64)
        host = np.full(64 + rows * pitch + 64, 255, np.uint8)
        for i in range(rows):
            host[off[i]:off[i] + cols] = x[i]
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.row_off = torch.from_numpy(off).cuda()
        self.rows, self.cols, self.host_off = rows, cols, off

    def load(self, x):
        host = np.full(self.buf.numel(), 255, np.uint8)
        for i in range(self.rows):
            host[self.host_off[i]:self.host_off[i] + self.cols] = x[i]
        self.buf.copy_(torch.from_numpy(host))


class Out:
    """canary-framed out_ticks / out_ch (room entries), ev_off (rows + 1), total, over, and a scratch of garbage"""

    def __init__(self, mh, form, rows, cols, room, ch_bits=32, scratch=None):
        self.form, self.rows, self.cols, self.room, self.ch_bits = form, rows, cols, room, ch_bits
        self.ticks = torch.empty(room + 2 * PAD, dtype=torch.int64, device="cuda")
        self.ch = torch.empty(room + 2 * PAD, dtype=torch.int16 if ch_bits == 16 else torch.int32, device="cuda")
        self.off = torch.empty(rows + 1 + 2 * PAD, dtype=torch.int64, device="cuda")
        self.total = torch.empty(1 + 2 * PAD, dtype=torch.int64, device="cuda")
        self.over = torch.empty(1 + 2 * PAD, dtype=torch.int64, device="cuda")
        self.nscratch = mh._ingest.unbin_scratch_bytes(form, rows, cols)
        self.scratch = torch.empty(self.nscratch + GUARD, dtype=torch.uint8, device="cuda") if scratch is None else scratch
        self.reset(scratch is None)

    def reset(self, scratch=True):
        for t in (self.ticks, self.off, self.total, self.over):
            t.fill_(CANARY)
        self.ch.fill_(CAN32 if self.ch_bits == 32 else 0x5A5A)
        self.over[PAD] = 0                    # the caller zeroes over
        if scratch:
            self.scratch.fill_(SCRATCH_FILL)

    def call(self, mh, inp, row_off, origin=0, period=1, phase=0, capacity=None, stream=None, emit=True):
        st = ct.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        L = mh._ingest.lib()
        p = lambda t, skip=0: ct.c_void_p(t.data_ptr() + t.element_size() * skip)   # noqa: E731
        ro = None if row_off is None else p(row_off)
        ev = p(self.off, PAD) if self.form == CSR else None
        rc = L.mhi_unbin_count(self.form, p(inp), ro, self.rows, self.cols, ev, p(self.total, PAD), p(self.scratch),
                               self.nscratch, st)
        assert rc == 0, L.mhi_last_error()
        if not emit:
            return
        cap = self.room if capacity is None else capacity
        rc = L.mhi_unbin_emit(self.form, p(inp), ro, self.rows, self.cols, origin, period, phase, p(self.ticks, PAD),
                              p(self.ch, PAD) if self.form == AER else None, self.ch_bits, cap, p(self.over, PAD),
                              p(self.scratch), self.nscratch, st)
        assert rc == 0, L.mhi_last_error()

    def check(self, want_ticks, want_off=None, want_ch=None, stored=None, tag=""):
        """every entry of every buffer; stored: the entries below the capacity (default: all of them)"""
        n = want_ticks.size
        stored = n if stored is None else stored
        if self.scratch.numel() > self.nscratch:
            assert bool((self.scratch[self.nscratch:] == SCRATCH_FILL).all()), (tag, "a write behind the scratch")
        can = np.uint64(CANARY)

        def framed(t, body):
            got = t.cpu().numpy().view(np.uint64)
            exp = np.full(got.size, can, np.uint64)
            exp[PAD:PAD + len(body)] = body
            return got, exp
        got, exp = framed(self.total, [n])
        assert np.array_equal(got, exp), (tag, "total", int(got[PAD]), n)
        got, exp = framed(self.over, [n - stored])
        assert np.array_equal(got, exp), (tag, "over", int(got[PAD]), n - stored)
        got, exp = framed(self.off, want_off if self.form == CSR else [])
        assert np.array_equal(got, exp), (tag, "ev_off", int(np.flatnonzero(got != exp)[0]) - PAD)
        got, exp = framed(self.ticks, want_ticks[:stored])
        assert np.array_equal(got, exp), (tag, "out_ticks", int(np.flatnonzero(got != exp)[0]) - PAD, n)
        udt = np.uint16 if self.ch_bits == 16 else np.uint32
        got = self.ch.cpu().numpy().view(udt)
        exp = np.full(got.size, 0x5A5A if self.ch_bits == 16 else CAN32, udt)
        if self.form == AER:
            exp[PAD:PAD + stored] = want_ch[:stored].astype(udt)
        assert np.array_equal(got, exp), (tag, "out_ch", int(np.flatnonzero(got != exp)[0]) - PAD, n)


def csr_once(mh, x, origin=0, period=1, phase=0, turn=0, tag=""):
    want, off = csr_oracle(x, origin, period, phase)
    inp = CsrInput(x, turn)
    o = Out(mh, CSR, x.shape[0], x.shape[1], want.size)
    o.call(mh, inp.buf, inp.row_off, origin, period, phase)
    o.check(want, off, tag=tag)


def aer_once(mh, X, ch_bits, origin=0, period=1, phase=0, tag=""):
    want, ch = aer_oracle(X, origin, period, phase)
    o = Out(mh, AER, X.shape[0], X.shape[1], want.size, ch_bits)
    o.call(mh, torch.from_numpy(X).cuda(), None, origin, period, phase)
    o.check(want, want_ch=ch, tag=tag)


def patterns(rng, rows, cols):
    """name -> [rows, cols] uint8"""
    out = {"zero": np.zeros((rows, cols), np.uint8),
           "bernoulli": (rng.rand(rows, cols) < 0.03).astype(np.uint8),
           "poisson": np.minimum(rng.poisson(1.5, size=(rows, cols)), 9).astype(np.uint8)}
    if cols <= 1025:
        out["all_255"] = np.full((rows, cols), 255, np.uint8)          # the staging is stored in rounds
    for name, at in (("first_byte", 0), ("last_byte", cols - 1), ("tile_end", TILE - 1)):
        if at < cols:
            x = np.zeros((rows, cols), np.uint8)
            x[rows // 2, at] = 255
            out["255_in_" + name] = x
    return out


# ---- 1. CSR shapes and count patterns ----------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 15, 16, 17, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 5])
def test_csr_every_width_around_a_load_a_wave_row_and_a_tile(mh, cols):
    rng = np.random.RandomState(cols)
    for turn, rows in enumerate((1, 3, 5)):
        pats = patterns(rng, rows, cols)
        assert ("255_in_tile_end" in pats) == (cols >= TILE) and ("all_255" in pats) == (cols <= 1025)
        for name, x in pats.items():
            csr_once(mh, x, origin=5, period=3, phase=1, turn=turn, tag=(name, rows, cols))


def test_csr_all_zero_writes_nothing(mh):
    x = np.zeros((3, TILE + 1), np.uint8)
    inp = CsrInput(x)
    o = Out(mh, CSR, 3, TILE + 1, 50)
    o.call(mh, inp.buf, inp.row_off)
    o.check(np.zeros(0, np.uint64), np.zeros(4, np.uint64), tag="zero")


def test_csr_more_than_one_group_of_the_scan(mh):
    """1024 tiles make a group: 1030 short rows, one tile each, two groups; every row a few events"""
    rng = np.random.RandomState(5)
    x = (rng.rand(GROUP + 6, 40) < 0.2).astype(np.uint8) * rng.randint(1, 4, size=(GROUP + 6, 40)).astype(np.uint8)
    csr_once(mh, x, origin=100, period=7, phase=6, tag="groups")


def test_csr_a_wave_row_that_exactly_fills_the_staging(mh):
    """2048 events in one wave row, then more: the staging is stored full, and again at the tile's end"""
    x = np.zeros((1, 3000), np.uint8)
    x[0, :1024] = 2                        # wave row 0: exactly 2048 events
    x[0, 1024:1030] = 1
    x[0, 2048:2060] = 200                  # wave row 2: 2400 events, through a window
    csr_once(mh, x, tag="staging")


# ---- 2. AER shapes -----------------------------------------------------------------------------------------------
def aer_lengths(C):
    """T such that T * C brackets a tile boundary - 1, + 0, + 1 and 2 tiles + 5 as tightly as C allows"""
    out = []
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        out += [max(n // C, 1), -(-n // C)]
    return sorted(set(out))


@pytest.mark.parametrize("ch_bits", [16, 32])
@pytest.mark.parametrize("C", [1, 3, 96, 128, 1000])
def test_aer_every_block_around_a_tile(mh, C, ch_bits):
    from muahuff import container, events
    rng = np.random.RandomState(C + ch_bits)
    Ts = aer_lengths(C)
    if C == 1:
        assert Ts == [TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
    if C == 128:                                                    # 128 rows of 128 channels are one tile exactly
        assert {127, 128, 129} <= set(Ts)
    for k, T in enumerate(Ts):
        X = patterns(rng, T, C)["bernoulli" if k % 2 else "poisson"]
        X[-1, -1] = 3                                               # the block's last byte counts
        aer_once(mh, X, ch_bits, origin=1000, period=30, phase=29, tag=(C, T, ch_bits))
    # ... and the list is what from_aer takes: partitioned and binned, it is the de-interleaved block again
    T = Ts[-1]
    X = np.minimum(rng.poisson(0.7, size=(T, C)), 9).astype(np.uint8)
    ticks, ch = events.aer_from_counts(torch.from_numpy(X).cuda(), 1000, 30, 29,
                                       ch_dtype=torch.int16 if ch_bits == 16 else torch.int32)
    want, wch = aer_oracle(X, 1000, 30, 29)
    assert np.array_equal(ticks.cpu().numpy().view(np.uint64), want) and np.array_equal(ch.cpu().numpy(), wch)
    ev = events.EventSet.from_aer(ticks, ch, C)
    back = container.ChannelSet.from_events(ev, 1000, 30, T)
    assert np.array_equal(back.matrix().cpu().numpy(), X.T)


def test_aer_all_255_and_zero(mh):
    aer_once(mh, np.full((9, 100), 255, np.uint8), 16, tag="aer 255")
    aer_once(mh, np.zeros((TILE // 96 + 3, 96), np.uint8), 32, tag="aer zero")


def test_aer_channels_up_to_the_16_bit_limit(mh):
    X = np.zeros((2, 65536), np.uint8)
    X[0, 65535] = 2
    X[1, [0, 32768, 65535]] = 1
    aer_once(mh, X, 16, origin=7, period=2, phase=1, tag="65536 channels")
    X = np.zeros((2, 65537), np.uint8)
    X[:, 65536] = 3
    aer_once(mh, X, 32, tag="65537 channels")


# ---- 3. arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 29])
def test_ticks_near_2_to_the_62_and_the_largest_accepted_tick(mh, phase):
    rng = np.random.RandomState(phase)
    cols = TILE + 100
    x = np.minimum(rng.poisson(0.5, size=(3, cols)), 9).astype(np.uint8)
    x[:, -1] = 2                                                      # the last column's tick is emitted
    csr_once(mh, x, origin=(1 << 62) - 12345, period=30, phase=phase, turn=1, tag="csr 2^62")
    top = (1 << 63) - 1 - (cols - 1) * 30 - phase                    # the last column's tick is 2^63 - 1
    want, _ = csr_oracle(x, top, 30, phase)
    assert int(want.max()) == (1 << 63) - 1
    csr_once(mh, x, origin=top, period=30, phase=phase, tag="csr largest")
    X = np.ascontiguousarray(x.T[:, :3])
    aer_once(mh, np.tile(X, (1, 4)), 32, origin=(1 << 62) + 99, period=30, phase=phase, tag="aer 2^62")
    top = (1 << 63) - 1 - (X.shape[0] - 1) * 30 - phase
    aer_once(mh, X, 16, origin=top, period=30, phase=phase, tag="aer largest")
    L = mh._ingest.lib()                                              # one tick more is refused, nothing is launched
    o = Out(mh, AER, X.shape[0], 3, 8)
    d = torch.from_numpy(X).cuda()
    p = lambda t: ct.c_void_p(t.data_ptr())   # noqa: E731
    rc = L.mhi_unbin_emit(AER, p(d), None, X.shape[0], 3, top + 1, 30, phase, p(o.ticks), p(o.ch), 16, 8, p(o.over),
                          p(o.scratch), o.nscratch, None)
    assert rc == mh._lib.ERR_ARG and "mhi_unbin_emit" in L.mhi_last_error().decode()


# ---- 4. capacity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [CSR, AER])
def test_nothing_is_stored_at_or_behind_the_capacity(mh, form):
    rng = np.random.RandomState(11 + form)
    x = np.minimum(rng.poisson(1.5, size=(3, TILE + 700)), 9).astype(np.uint8)
    x[-1, -1] = 4
    if form == CSR:
        want, off = csr_oracle(x, 9, 2, 1)
        inp, ch = CsrInput(x), None
        buf, ro, rows, cols = inp.buf, inp.row_off, 3, x.shape[1]
    else:
        X = np.ascontiguousarray(x.T)
        want, ch = aer_oracle(X, 9, 2, 1)
        off, buf, ro, rows, cols = None, torch.from_numpy(X).cuda(), None, X.shape[0], 3
    n = want.size
    for cap in (n - 1, n // 2 + 3, 0):
        o = Out(mh, form, rows, cols, n, 16)
        o.call(mh, buf, ro, 9, 2, 1, capacity=cap)
        o.check(want, off, ch, stored=cap, tag=("capacity", cap))


# ---- 5. the asynchronous contract --------------------------------------------------------------------------------
def _two_inputs():
    rng = np.random.RandomState(77)
    a = np.minimum(rng.poisson(1.0, size=(5, 2 * TILE + 5)), 9).astype(np.uint8)
    b = np.ascontiguousarray(a[::-1, ::-1])                     # the same total, other places
    return a, b


def test_side_stream_and_two_calls_chained_on_one_scratch(mh):
    a, b = _two_inputs()
    b = b.copy()
    b[2, 100:900] = 0                                           # ... and another total for the second call
    wa, oa = csr_oracle(a, 3, 5, 2)
    wb, ob = csr_oracle(b, 3, 5, 2)
    ia, ib = CsrInput(a), CsrInput(b, turn=2)
    A = Out(mh, CSR, 5, a.shape[1], wa.size)
    B = Out(mh, CSR, 5, b.shape[1], wb.size, scratch=A.scratch)     # one scratch, left as the first pair leaves it
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        A.call(mh, ia.buf, ia.row_off, 3, 5, 2, stream=side.cuda_stream)
        B.call(mh, ib.buf, ib.row_off, 3, 5, 2, stream=side.cuda_stream)
    side.synchronize()
    A.check(wa, oa, tag="first")
    B.check(wb, ob, tag="second")


@pytest.mark.parametrize("form", [CSR, AER])
def test_capture_and_replay_on_changed_input_of_equal_total(mh, form):
    a, b = _two_inputs()
    if form == CSR:
        inp = CsrInput(a)
        buf, ro, rows, cols = inp.buf, inp.row_off, 5, a.shape[1]
        want = {0: csr_oracle(a, 3, 5, 2) + (None,), 1: csr_oracle(b, 3, 5, 2) + (None,)}
        load = lambda k: inp.load((a, b)[k])   # noqa: E731
    else:
        A, B = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
        buf, ro, rows, cols = torch.from_numpy(A).cuda(), None, A.shape[0], 5
        want = {k: (aer_oracle(X, 3, 5, 2)[0], None, aer_oracle(X, 3, 5, 2)[1]) for k, X in ((0, A), (1, B))}
        load = lambda k: buf.copy_(torch.from_numpy((A, B)[k]))   # noqa: E731
    n = want[0][0].size
    assert n == want[1][0].size and not np.array_equal(want[0][0], want[1][0])
    o = Out(mh, form, rows, cols, n)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        o.call(mh, buf, ro, 3, 5, 2, stream=side.cuda_stream)             # warm-up outside capture
        side.synchronize()
        o.check(*want[0], tag="warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        o.call(mh, buf, ro, 3, 5, 2, stream=side.cuda_stream)
    for k in (1, 0, 1):
        with torch.cuda.stream(side):
            load(k)
            o.reset()
            g.replay()
            side.synchronize()
            o.check(*want[k], tag=("replay", k))


# ---- 6. through the stack ----------------------------------------------------------------------------------------
def test_from_counts_then_from_events_is_the_channel_set(mh):
    from muahuff import container, events
    rng = np.random.RandomState(3)
    T = 2 * TILE + 77
    chans = [np.minimum(rng.poisson(0.4, size=T), 255).astype(np.uint8) for _ in range(6)]
    chans[2][:] = 0
    chans[4][-1] = 255
    cs = container.ChannelSet.from_channels(chans)
    ev = events.EventSet.from_counts(cs)
    want, off = csr_oracle(np.stack(chans), 0, 1, 0)
    assert ev.C == 6 and np.array_equal(ev.offsets, off) and torch.equal(ev.ev_off.cpu(), torch.from_numpy(off.view(np.int64)))
    assert np.array_equal(ev.ticks.cpu().numpy().view(np.uint64), want)
    back = container.ChannelSet.from_events(ev, 0, 1, T)
    assert np.array_equal(back.ch_off, cs.ch_off) and np.array_equal(back.ch_len, cs.ch_len)
    assert torch.equal(back.data, cs.data)
    ev2 = events.EventSet.from_counts(cs, origin=1 << 40, period=30, phase=7)
    assert np.array_equal(ev2.ticks.cpu().numpy().view(np.uint64), csr_oracle(np.stack(chans), 1 << 40, 30, 7)[0])
    ragged = container.ChannelSet.from_channels([chans[0], chans[1][:-5]])
    with pytest.raises(ValueError):
        events.EventSet.from_counts(ragged)
    for bad in (dict(period=0), dict(period=5, phase=5), dict(origin=-1), dict(origin=(1 << 63) - T + 1)):
        with pytest.raises(ValueError):
            events.EventSet.from_counts(cs, **bad)
    with pytest.raises(ValueError):
        events.EventSet.from_counts(cs.matrix().to(torch.int32))
    with pytest.raises(ValueError):
        events.EventSet.from_counts(cs.matrix()[:, ::2])


def test_from_counts_on_the_pitched_offset_view_of_a_range_decode(mh):
    from muahuff import container_io as cio
    from muahuff import events
    rng = np.random.RandomState(8)
    S, T = 4, 3 * 16384 + 1234
    chans = [np.minimum(rng.poisson(0.3, size=T), 255).astype(np.uint8) for _ in range(5)]
    c = mh.compress(chans, S=S)
    a, b = 16384 + 37, 2 * 16384 + 901
    view = cio.decompress_range(c, a, b, channels=[4, 0, 3])
    assert view.is_cuda and tuple(view.shape) == (3, b - a) and view.stride(1) == 1
    assert view.stride(0) >= b - a
    for v, first in ((view, a), (view[1:, 11:-3], a + 11)):           # as returned; a view into it: pitched and offset
        if v is not view:
            assert v.stride(0) > v.shape[1] and not v.is_contiguous() and v.data_ptr() != view.data_ptr()
        host = v.cpu().numpy()
        ev = events.EventSet.from_counts(v, origin=first * 30, period=30, phase=3)
        want, off = csr_oracle(host, first * 30, 30, 3)
        assert want.size > 1000
        assert np.array_equal(ev.offsets, off) and np.array_equal(ev.ticks.cpu().numpy().view(np.uint64), want)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "checksum"])
def event_archive(request, mh, tmp_path_factory):
    """an archive written with append_events: 7 channels, three blocks of unequal length, at most S - 1 events per bin"""
    from muahuff import archive, events
    C, S, period, origin = 7, 4, 30, 1 << 36
    lens = [5000, 2 * 16384 + 77, 16384 - 3]
    rng = np.random.RandomState(41)
    counts = np.minimum(rng.poisson(0.5, size=(C, sum(lens))), S - 1).astype(np.uint8)
    counts[:, lens[0] - 1] = S - 1                               # events on either side of a block boundary
    counts[:, lens[0]] = 1
    per = []
    for c in range(C):                                           # ticks anywhere inside their bin, in order
        start = np.repeat(np.arange(counts.shape[1], dtype=np.uint64), counts[c]) * np.uint64(period) + np.uint64(origin)
        per.append(np.sort(start + rng.randint(0, period, size=start.size).astype(np.uint64)))
    fn = str(tmp_path_factory.mktemp("unbin") / "events.mua")
    with archive.create(fn, C, S=S, hist_bits=6, checksum=request.param) as w:
        t0 = 0
        for Tb in lens:
            lo, hi = origin + t0 * period, origin + (t0 + Tb) * period
            ev = events.EventSet.from_channels([p[(p >= np.uint64(lo)) & (p < np.uint64(hi))] for p in per])
            w.append_events(ev, lo, period, Tb)
            t0 += Tb
    return dict(fn=fn, C=C, S=S, period=period, origin=origin, lens=lens, per=per, checksum=request.param)


def test_read_events_across_a_block_boundary_with_a_permuted_subset(mh, event_archive):
    from muahuff import archive
    m = event_archive
    o, p = m["origin"], m["period"]
    sel = [5, 0, 6, 2]
    with archive.open(m["fn"]) as a:
        assert a.checksum == m["checksum"] and [b.Tb for b in a.blocks] == m["lens"]
        for start, stop in ((m["lens"][0] - 300, m["lens"][0] + 16384 + 500), (0, a.T), (m["lens"][0], m["lens"][0] + 1)):
            ev = a.read_events(start, stop, channels=sel, origin=o, period=p)
            assert ev.C == len(sel)
            lo, hi = np.uint64(o + start * p), np.uint64(o + stop * p)
            got = ev.ticks.cpu().numpy().view(np.uint64)
            for k, c in enumerate(sel):
                t = m["per"][c]
                t = t[(t >= lo) & (t < hi)]
                want = (t - np.uint64(o)) // np.uint64(p) * np.uint64(p) + np.uint64(o)     # floored to the bin's start
                assert np.array_equal(got[int(ev.offsets[k]):int(ev.offsets[k + 1])], want), (start, stop, c)
        ev = a.read_events(100, 400, origin=o, period=p, phase=29)                           # all channels, a phase
        assert ev.C == m["C"] and bool(((ev.ticks - o) % p == 29).all())
        empty = a.read_events(50, 50, channels=sel)
        assert empty.C == len(sel) and empty.ticks.numel() == 0


def test_read_events_as_a_merged_list(mh, event_archive):
    from muahuff import archive
    m = event_archive
    o, p = m["origin"], m["period"]
    sel = [5, 0, 6, 2]
    start, stop = m["lens"][0] - 300, m["lens"][0] + 16384 + 500
    lo, hi = np.uint64(o + start * p), np.uint64(o + stop * p)
    with archive.open(m["fn"]) as a:
        for channels, dt in ((sel, torch.int32), (None, torch.int16)):
            ticks, ch = a.read_events(start, stop, channels=channels, origin=o, period=p, aer=True, ch_dtype=dt)
            assert ch.dtype == dt and ticks.dtype == torch.int64
            order = sel if channels is not None else list(range(m["C"]))
            tt, cc, kk = [], [], []
            for k, c in enumerate(order):                         # the merged list: by tick, then by place in `channels`
                t = m["per"][c]
                t = t[(t >= lo) & (t < hi)]
                tt.append((t - np.uint64(o)) // np.uint64(p) * np.uint64(p) + np.uint64(o))
                cc.append(np.full(t.size, c))
                kk.append(np.full(t.size, k))
            tt, cc, kk = np.concatenate(tt), np.concatenate(cc), np.concatenate(kk)
            idx = np.lexsort((kk, tt))
            assert np.array_equal(ticks.cpu().numpy().view(np.uint64), tt[idx])
            assert np.array_equal(ch.cpu().numpy().astype(np.int64), cc[idx])
