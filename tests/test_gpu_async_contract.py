"""The asynchronous contract at the top of include/muahuff.h, on the GPU: stream order, graph capture, plan-owned state
across mixed call sequences and two host threads (tests/async_table.py has the classes and the plan layouts).

Every expectation is computed on the host from the bytes a call was given -- oracle.c for the codec, NumPy for layout,
sweep and analysis results -- never from another call into the library.  Every entry point runs as a CASE: fixed
device input buffers that dataset k is copied INTO (`load`), outputs inside canary-filled buffers (`reset`, `fetch`),
the call itself on an explicit stream (`call`) and the comparison with the oracle on dataset k (`verify`).

3a  stream order (test_stream_order): on a non-blocking side stream, with nothing synchronising until the end:
    a delay of plain torch elementwise passes, an event, the call on dataset A (so that every scratch word of the
    library is dirty and every output written), canaries over the outputs, copy_ of dataset B into the same input
    buffers, the call under test, asynchronous copies of the outputs to pinned memory.  The result must be the oracle
    on B.  Internal work that slipped onto the null stream would run during the delay -- ahead of the A call that
    dirties the scratch again, ahead of the canaries and ahead of B -- and the outputs differ.  The event must still
    be pending when a capturable call returns: that shows the race was real and that the call did not block; a case
    where it has completed FAILS (the delay is too short), it is not skipped.
    Known limit: with the 4 hardware queues of a process here a side stream and the null stream can share a queue; the
    race then serialises and the test can miss such a defect.  It cannot report a false one.
3b  graph capture (test_graph_replay): linear graphs on one side stream, replayed with the input contents (and the
    preset word) overwritten before every replay; the transmit and receive pipelines of stream.py as single graphs.
3c  plan state (test_plan_state_across_a_mixed_sequence): one plan per layout, a fixed-seed sequence that contains every
    ordered pair of operation kinds, three datasets with different statistics rotating through the same buffers.
3d  two host threads, each with its own plan, stream and dataset; mh_last_error stays thread-local.
"""
import ctypes as ct
import threading
import time
import zlib

import numpy as np
import pytest
import torch

import oracle
from tests import async_table as at
from tests import helpers
from tests.test_gpu_kernel_cells import _make
from tests.test_gpu_parity import _bitpack, _window

pytestmark = pytest.mark.gpu

OC = oracle.c
CH = at.CHUNK
CANARY = 0xA5
PAD = 256            # canary bytes in front of and behind every output (keeps the 256-byte alignment of the allocation)
NT = 16              # oracle threads

# The delay of 3a: DELAY_PASSES in-place passes over a DELAY_BYTES tensor on the side stream (1 GiB of traffic per
# pass).  It has to outlast the host-side enqueue of the primer call, the canaries, the input copies and the call under
# test several times over; every case prints both figures (run with -s), and a case whose delay had already completed
# fails with those figures in its message.  Measured on an MI355X over all 54 cases: the slowest host-side enqueue of
# that group for a capturable call was 0.17 ms (mh_measure on layout a, the first case of the process; 0.02 - 0.09 ms
# for the others), the delay takes 4.25 - 4.31 ms on the device: 25 times the slowest enqueue.
DELAY_BYTES = 512 << 20
DELAY_PASSES = 24


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    info = muahuff.device_info(0)
    assert "gfx950" in info["arch"], info
    torch.cuda.set_device(0)
    return muahuff


def _lib():
    import muahuff
    return muahuff._lib.lib()


def _ok(rc):
    import muahuff
    muahuff._lib.check(rc)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def _const(a):
    """a device tensor that stays as it is (offsets, lengths)"""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guard:
    """an output buffer of n bytes between two canary margins, and its pinned host copy"""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((2 * PAD + self.n,), CANARY, dtype=torch.uint8, device="cuda")
        self.pin = torch.empty(2 * PAD + self.n, dtype=torch.uint8).pin_memory()

    @property
    def ptr(self):
        return ct.c_void_p(self.buf.data_ptr() + PAD)

    def reset(self):
        self.buf.fill_(CANARY)

    def fetch(self):
        self.pin.copy_(self.buf, non_blocking=True)

    def host(self, dtype=np.uint8):
        h = self.pin.numpy()
        assert (h[:PAD] == CANARY).all() and (h[PAD + self.n:] == CANARY).all(), "bytes outside the output were written"
        return h[PAD:PAD + self.n].view(dtype)


class Input:
    """a device input buffer and the pinned host images of the datasets that are copied into it"""

    def __init__(self, images, slack=0):
        self.pins = []
        size = max(im.nbytes for im in images) + slack
        for im in images:
            pin = torch.zeros(size, dtype=torch.uint8).pin_memory()
            pin[:im.nbytes] = torch.from_numpy(np.ascontiguousarray(im).view(np.uint8).reshape(-1))
            self.pins.append(pin)
        self.buf = torch.zeros(size, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return ct.c_void_p(self.buf.data_ptr())

    def load(self, k):
        self.buf.copy_(self.pins[k], non_blocking=True)


class Case:
    """One entry point (or pipeline) in runnable form.  Subclasses fill inputs / guards and define call and verify."""
    name = ""
    sync = False         # classified `synchronises`: exempt from the did-not-block check only
    n_data = 3

    def __init__(self):
        self.inputs, self.guards = [], []

    def inp(self, images, slack=0):
        self.inputs.append(Input(images, slack))
        return self.inputs[-1]

    def out(self, n):
        self.guards.append(Guard(n))
        return self.guards[-1]

    def load(self, k):
        for i in self.inputs:
            i.load(k)

    def reset(self):
        for g in self.guards:
            g.reset()

    def fetch(self):
        for g in self.guards:
            g.fetch()

    def close(self):
        pass


# ---------------------------------------------------------------------------------------------------------------------
# plan-based cases: one World (host expectations) per layout, one Bench (plan + buffers) per test

def _used_mask(seg_off, seg_words, size):
    d = np.zeros(size + 1, np.int64)
    np.add.at(d, seg_off.astype(np.int64), 1)
    np.add.at(d, (seg_off + seg_words).astype(np.int64), -1)
    return np.cumsum(d[:-1]) > 0


class World:
    """three datasets of one layout -- quiet, busy, and one that sits on the longest code of the quiet word -- with
    everything the oracle says about them"""

    def __init__(self, l):
        self.l = l
        self.rows = helpers.sclv_tables()[l.S]
        self.K, self.C = len(self.rows), len(l.lens)
        self.p = OC.Params(l.S, l.h, l.mode, l.window, self.rows, seg_chunks=l.seg_chunks)
        rng = np.random.RandomState(zlib.crc32(("async" + l.name).encode()))
        sets = [[np.minimum(rng.poisson(0.05, size=T), 255).astype(np.uint8) for T in l.lens],
                [np.minimum(rng.poisson(float(np.exp(rng.uniform(0.0, np.log(6.0)))), size=T), 255).astype(np.uint8)
                 for T in l.lens],
                _make("drift", rng, l.S, l.mode, self.rows, l.lens)[0]]
        self.data, self.om, self.oe, self.od, self.dense, self.doff, self.used, self.pre = [], [], [], [], [], [], [], []
        for chans in sets:
            data, off, ln = OC.flatten(chans)
            self.off, self.ln = off, ln
            self.data.append(data)
            self.om.append(OC.measure(data, off, ln, self.p, nthreads=NT))
            oe = OC.encode(data, off, ln, self.p, nthreads=NT)
            self.oe.append(oe)
            self.od.append(OC.decode(oe["payload"], off, ln, self.p, oe["peak"], oe["enc"], len(data), nthreads=NT))
            used = _used_mask(oe["seg"]["off"], oe["seg_words"], oe["payload"].size)
            self.used.append(used)
            self.dense.append(oe["payload"][used])            # slots ascend: the segments back to back
            self.doff.append(np.concatenate([[0], np.cumsum(oe["seg_words"])[:-1]]).astype(np.uint64))
        self.size = len(self.data[0])
        self.seg = self.oe[0]["seg"]
        self.nseg = len(self.seg["ch"])
        self.cap = self.oe[0]["payload"].size                  # the plan's payload_cap_words
        # preset encode of dataset k with the word calibrated on dataset k + 1
        for k in range(3):
            w = self.oe[(k + 1) % 3]
            pe = OC.encode_preset(self.data[k], self.off, self.ln, self.p, w["peak"], w["enc"], nthreads=NT)
            pe["used"] = _used_mask(pe["seg"]["off"], pe["seg_words"], pe["payload"].size)
            self.pre.append(pe)
        self.inwin = np.zeros(self.size, bool)
        for c, T in enumerate(l.lens):
            w0, w1 = _window(T, l.h, l.window)
            self.inwin[int(self.off[c]) + w0:int(self.off[c]) + w1] = True
        assert self.inwin.sum() > 0
        self.want_dec = [np.where(self.inwin, od, CANARY).astype(np.uint8) for od in self.od]
        # range queries (t0 a multiple of 80: bin factors 5 and 16); channels far apart, one repeated
        C, T = self.C, max(l.lens)
        self.queries = [((C - 1, 0, C - 1, C // 2), 0, T),
                        ((C // 2, C - 1), 16320, min(T, 2 * CH + 777)),
                        ((0, C - 1), 80, 85),
                        ((C - 1,), 2 * CH - 128, T)]

    def rows_of(self, k, q):
        sel, a, b = self.queries[q]
        rows = np.zeros((len(sel), b - a), np.uint8)
        for i, c in enumerate(sel):
            o = int(self.off[c])
            x = self.od[k][o:o + self.l.lens[c]][a:b]
            rows[i, :len(x)] = x
        return rows


_worlds = {}


def _world(name):
    if name not in _worlds:
        _worlds[name] = World(at.BY_NAME[name])
    return _worlds[name]


class Bench:
    """one plan of a layout with the input buffers the datasets are copied into; makes the layout's cases"""

    def __init__(self, mh, w):
        self.w, l = w, w.l
        self.plan = mh.codec.Plan(w.off, w.ln, l.S, l.h, l.mode, l.window, w.rows, seg_chunks=l.seg_chunks)
        assert self.plan.n_segments == w.nseg and self.plan.payload_cap_words == w.cap
        assert np.array_equal(self.plan.segments()["off"], w.seg["off"])
        self.h = self.plan._h
        self.data = Input(w.data)
        self.slot_off = _const(_i64(w.seg["off"]))
        self._cases = []

    def case(self, kind, variant=0):
        c = PLAN_CASES[kind](self, variant)
        self._cases.append(c)
        return c

    def status(self, st):
        flags = ct.c_uint32(7)
        _ok(_lib().mh_decode_status(self.h, ct.byref(flags), st))
        return flags.value

    def close(self):
        self.plan.close()


class PlanCase(Case):
    def __init__(self, b, variant):
        super().__init__()
        self.b, self.w, self.v = b, b.w, variant
        self.inputs.append(b.data)
        self.name = "%s[%s%d]" % (type(self).__name__, b.w.l.name, variant)


class Measure(PlanCase):
    """variant 0: all outputs; 1: every optional output NULL except bits"""

    def __init__(self, b, v):
        super().__init__(b, v)
        C, S = self.w.C, self.w.l.S
        self.bits = self.out(8 * C)
        if v == 0:
            self.o = [self.out(n) for n in (8 * C, 4 * C * S, C, C, 8 * C * S, C)]

    def call(self, st):
        if self.v == 0:
            cut, cal, pk, en, post, sk = (g.ptr for g in self.o)
            _ok(_lib().mh_measure(self.b.h, self.b.data.ptr, cut, cal, pk, en, post, self.bits.ptr, sk, st))
        else:
            _ok(_lib().mh_measure(self.b.h, self.b.data.ptr, None, None, None, None, None, self.bits.ptr, None, st))

    def verify(self, k):
        om = self.w.om[k]
        assert np.array_equal(self.bits.host(np.uint64), om["bits"]), (self.name, k, "bits")
        if self.v == 0:
            for g, key, dt in zip(self.o, ("cutoff", "cal_sorted", "peak", "enc", "post_mapped", "skipped"),
                                  (np.uint64, np.uint32, np.uint8, np.uint8, np.uint64, np.uint8)):
                assert np.array_equal(g.host(dt), om[key].reshape(-1)), (self.name, k, key)


class Encode(PlanCase):
    """variant 0: peak / enc / skipped given; 1: NULL, the plan's own words; 2: mh_encode_preset with the word of the
    NEXT dataset"""

    def __init__(self, b, v):
        super().__init__(b, v)
        w = self.w
        self.pay, self.segw, self.chb = self.out(4 * w.cap), self.out(8 * w.nseg), self.out(8 * w.C)
        if v == 0:
            self.pk, self.en, self.sk = self.out(w.C), self.out(w.C), self.out(w.C)
        if v == 2:
            self.wpk = self.inp([w.oe[(k + 1) % 3]["peak"] for k in range(3)])
            self.wen = self.inp([w.oe[(k + 1) % 3]["enc"] for k in range(3)])

    def call(self, st):
        b, L = self.b, _lib()
        if self.v == 2:
            _ok(L.mh_encode_preset(b.h, b.data.ptr, self.wpk.ptr, self.wen.ptr, self.pay.ptr, self.w.cap, self.segw.ptr,
                                   self.chb.ptr, st))
        elif self.v == 0:
            _ok(L.mh_encode(b.h, b.data.ptr, self.pay.ptr, self.w.cap, self.segw.ptr, self.chb.ptr, self.pk.ptr,
                            self.en.ptr, self.sk.ptr, st))
        else:
            _ok(L.mh_encode(b.h, b.data.ptr, self.pay.ptr, self.w.cap, self.segw.ptr, self.chb.ptr, None, None, None, st))

    def verify(self, k):
        oe = self.w.pre[k] if self.v == 2 else self.w.oe[k]
        used = oe["used"] if self.v == 2 else self.w.used[k]
        tag = (self.name, k)
        assert np.array_equal(self.segw.host(np.uint64), oe["seg_words"]), tag
        assert np.array_equal(self.chb.host(np.uint64), oe["ch_bits"]), tag
        assert np.array_equal(self.pay.host(np.uint32)[used], oe["payload"][used]), tag
        if self.v == 0:
            for g, key in ((self.pk, "peak"), (self.en, "enc"), (self.sk, "skipped")):
                assert np.array_equal(g.host(), oe[key]), tag + (key,)


class Decode(PlanCase):
    """the oracle's stream of dataset k; variant 0: in the plan's slots, 1: compacted, through seg_off; 2: the slots with
    mh_decode_status behind the decode, dataset 1 being an all-zero payload (abandoned: flag 1, nothing outside the
    windows written)"""

    def __init__(self, b, v):
        super().__init__(b, v)
        w = self.w
        self.inputs = []                        # decode does not read the data buffer
        if v == 1:
            self.pay = self.inp(w.dense, slack=16)
            self.soff = self.inp([_i64(d) for d in w.doff])
        else:
            pays = [oe["payload"] for oe in w.oe]
            if v == 2:
                pays[1] = np.zeros_like(pays[1])
            self.pay = self.inp(pays)
        self.pk, self.en = self.inp([oe["peak"] for oe in w.oe]), self.inp([oe["enc"] for oe in w.oe])
        self.o = self.out(w.size)
        self.sync = v == 2
        self.flags = None

    def call(self, st):
        w = self.w
        if self.v == 1:
            words, soff = self.pay.buf.numel() // 4, self.soff.ptr
        else:
            words, soff = w.cap, None
        _ok(_lib().mh_decode(self.b.h, self.pay.ptr, words, soff, self.pk.ptr, self.en.ptr, self.o.ptr, st))
        if self.v == 2:
            self.flags = self.b.status(st)

    def verify(self, k):
        got = self.o.host()
        if self.v == 2:
            assert self.flags == (1 if k == 1 else 0), (self.name, k, self.flags)
            if k == 1:
                assert (got[~self.w.inwin] == CANARY).all(), (self.name, "an abandoned decode wrote outside the windows")
                return
        assert np.array_equal(got, self.w.want_dec[k]), (self.name, k)


class Compact(PlanCase):
    def __init__(self, b, v):
        super().__init__(b, v)
        w = self.w
        self.inputs = []
        self.pay = self.inp([oe["payload"] for oe in w.oe])
        self.segw = self.inp([_i64(oe["seg_words"]) for oe in w.oe])
        self.dense, self.doff, self.tot = self.out(4 * w.cap), self.out(8 * w.nseg), self.out(8)

    def call(self, st):
        _ok(_lib().mh_compact(self.b.h, self.pay.ptr, self.segw.ptr, self.dense.ptr, self.w.cap, self.doff.ptr,
                              self.tot.ptr, st))

    def verify(self, k):
        w = self.w
        total = int(w.oe[k]["seg_words"].sum())
        assert int(self.tot.host(np.uint64)[0]) == total, (self.name, k)
        assert np.array_equal(self.doff.host(np.uint64), w.doff[k]), (self.name, k)
        assert np.array_equal(self.dense.host(np.uint32)[:total], w.dense[k]), (self.name, k)


class Range(PlanCase):
    """mh_decode_range (variant 0) / mh_decode_rebin (variant 1) of query self.q on the oracle's stream of dataset k,
    slots and compacted stream in turn; rows inside a pitched, canary-filled buffer"""
    sync = True
    LEAD, TAIL = 13, 24

    def __init__(self, b, v):
        super().__init__(b, v)
        w = self.w
        self.inputs = []
        self.pay = self.inp([oe["payload"] for oe in w.oe])
        self.dpay = self.inp(w.dense, slack=16)
        self.doff = self.inp([_i64(d) for d in w.doff])
        self.pk, self.en = self.inp([oe["peak"] for oe in w.oe]), self.inp([oe["enc"] for oe in w.oe])
        self.q, self.dense, self.r, self.sat = 0, False, 5, True
        rows = max(len(s) for s, _, _ in w.queries)
        self.o = self.out((rows * (max(b - a for _, a, b in w.queries) + self.TAIL) + self.LEAD) * 4)

    def set(self, q, dense=False, r=5, sat=True):
        self.q, self.dense, self.r, self.sat = q, dense, r, sat
        return self

    def _shape(self):
        sel, a, b = self.w.queries[self.q]
        n = b - a if self.v == 0 else (b - a + self.r - 1) // self.r
        return sel, a, b, n, n + self.TAIL, 1 if self.v == 0 or self.sat else 4

    def call(self, st):
        sel, a, b, n, pitch, el = self._shape()
        sel32 = np.array(sel, np.uint32)
        pay, words, soff = (self.dpay.ptr, self.dpay.buf.numel() // 4, self.doff.ptr) if self.dense else \
                           (self.pay.ptr, self.w.cap, ct.c_void_p(self.b.slot_off.data_ptr()))
        out = ct.c_void_p(self.o.ptr.value + self.LEAD * el)
        if self.v == 0:
            _ok(_lib().mh_decode_range(self.b.h, pay, words, soff, sel32.ctypes.data, len(sel), a, b, self.pk.ptr,
                                       self.en.ptr, out, pitch, st))
        else:
            _ok(_lib().mh_decode_rebin(self.b.h, pay, words, soff, sel32.ctypes.data, len(sel), a, b, self.r,
                                       1 if self.sat else 0, self.pk.ptr, self.en.ptr, out, pitch, st))

    def verify(self, k):
        sel, a, b, n, pitch, el = self._shape()
        want = self.w.rows_of(k, self.q)
        if self.v == 1:
            r = self.r
            y = np.zeros((len(sel), n * r), np.uint32)
            y[:, :b - a] = want
            want = y.reshape(len(sel), n, r).sum(axis=2)
            want = np.minimum(want, 255).astype(np.uint8) if self.sat else want.astype(np.uint32)
        got = self.o.host(np.uint8 if el == 1 else np.uint32)
        fill = CANARY if el == 1 else CANARY * 0x01010101
        tag = (self.name, k, self.q, self.dense, self.r, self.sat)
        assert (got[:self.LEAD] == fill).all(), tag
        body = got[self.LEAD:self.LEAD + len(sel) * pitch].reshape(len(sel), pitch)
        assert np.array_equal(body[:, :n], want), tag
        assert (body[:, n:] == fill).all() and (got[self.LEAD + len(sel) * pitch:] == fill).all(), tag


PLAN_CASES = dict(measure=Measure, encode=Encode, decode=Decode, compact=Compact, range=Range)


# ---------------------------------------------------------------------------------------------------------------------
# entry points without a plan (layout, synthesis, analysis, sweep) and the packed decoder

def _pieces(x, bits):
    npiece = (len(x) + 15) // 16
    s = np.zeros(npiece * 16, np.uint32)
    s[:len(x)] = np.minimum(x, (1 << bits) - 1)
    return _bitpack(s.reshape(npiece, 16), bits)


def _blocked(tm, bits, fill):
    """the chunk-blocked packed layout of stream.py for time-major samples tm[T, C]: chunk j of channel c at
    (j * C + c) * cb; bytes that hold no piece keep `fill`"""
    T, C = tm.shape
    pb, cb = 2 * bits, 1024 * 2 * bits
    buf = np.full((T + CH - 1) // CH * C * cb, fill, np.uint8)
    for c in range(C):
        by = _pieces(tm[:, c], bits)
        for j in range(0, len(by), 1024):
            at_ = (j // 1024 * C + c) * cb
            n = min(1024, len(by) - j)
            buf[at_:at_ + n * pb] = by[j:j + n].reshape(-1)
    return buf


def _time_major(rng, T, C, k):
    """[T, C] counts: quiet, busy with values far above 15, all on one high value"""
    if k == 0:
        return np.minimum(rng.poisson(0.1, size=(T, C)), 255).astype(np.uint8)
    if k == 1:
        x = rng.poisson(3.0, size=(T, C))
        return np.where(rng.random_sample((T, C)) < 0.2, rng.randint(0, 256, size=(T, C)), x).astype(np.uint8)
    x = np.full((T, C), 200, np.uint8)
    x[:300] = rng.randint(0, 20, size=(min(T, 300), C))
    return x


TP, CP = 2 * CH + 117, 9      # a block whose last piece is cut (117 = 7 * 16 + 5) and whose pieces end on 16 bytes


class Synth(Case):
    name = "mh_synth_poisson"

    def __init__(self):
        super().__init__()
        rng = np.random.RandomState(1)
        lens = [5, 16, 1000, CH + 3, 40000]
        _, self.off, self.ln = OC.flatten([np.zeros(T, np.uint8) for T in lens])
        self.size = int(self.off[-1]) + lens[-1] + 11
        self.thrs = [np.sort(rng.randint(0, 65537, size=(len(lens), 15)), axis=1).astype(np.uint32) for _ in range(3)]
        self.thr = self.inp(self.thrs)
        self.d_off, self.d_ln = _const(_i64(self.off)), _const(_i64(self.ln))
        self.o = self.out(self.size)

    def call(self, st):
        _ok(_lib().mh_synth_poisson(self.o.ptr, ct.c_void_p(self.d_off.data_ptr()), ct.c_void_p(self.d_ln.data_ptr()),
                                    len(self.ln), int(self.ln.max()), self.thr.ptr, 12345, st))

    def verify(self, k):
        x = OC.synth(self.off, self.ln, self.thrs[k], 12345, total=self.size)
        want = np.full(self.size, CANARY, np.uint8)
        for o, n in zip(self.off, self.ln):
            want[int(o):int(o + n)] = x[int(o):int(o + n)]
        assert np.array_equal(self.o.host(), want), (self.name, k)


class Rebin(Case):
    def __init__(self, r, sat):
        super().__init__()
        self.r, self.sat, self.name = r, sat, "mh_rebin[r=%d,%s]" % (r, "u8" if sat else "u32")
        rng = np.random.RandomState(2 + r)
        self.lens = [1, r, 5 * r + 1, 70001, CH]
        self.sets = [[(rng.randint(0, m, size=T)).astype(np.uint8) for T in self.lens] for m in (3, 256, 40)]
        flat = [OC.flatten(s) for s in self.sets]
        self.off, self.ln = flat[0][1], flat[0][2]
        self.data = self.inp([f[0] for f in flat])
        self.nb = [(T + r - 1) // r for T in self.lens]
        self.ooff = np.concatenate([[0], np.cumsum([n + 64 for n in self.nb])[:-1]]).astype(np.uint64)
        self.el = 1 if sat else 4
        self.o = self.out(int(self.ooff[-1] + self.nb[-1] + 64) * self.el)
        self.d = [_const(_i64(a)) for a in (self.off, self.ln, self.ooff)]

    def call(self, st):
        off, ln, ooff = (ct.c_void_p(t.data_ptr()) for t in self.d)
        _ok(_lib().mh_rebin(self.data.ptr, off, ln, len(self.lens), max(self.lens), self.r, 1 if self.sat else 0,
                            self.o.ptr, ooff, st))

    def verify(self, k):
        got = self.o.host(np.uint8 if self.sat else np.uint32)
        for c, x in enumerate(self.sets[k]):
            y = np.zeros(self.nb[c] * self.r, np.uint32)
            y[:len(x)] = x
            want = y.reshape(-1, self.r).sum(axis=1)
            want = np.minimum(want, 255).astype(np.uint8) if self.sat else want
            o = int(self.ooff[c])
            assert np.array_equal(got[o:o + self.nb[c]], want), (self.name, k, c)


class Transpose(Case):
    """mh_deinterleave (packed = 0, inverse = False), mh_interleave, and their packed forms on the chunk-blocked layout"""

    def __init__(self, bits, inverse):
        super().__init__()
        self.bits, self.inverse = bits, inverse
        self.name = "mh_%sinterleave%s" % ("" if inverse else "de", "_packed[%d]" % bits if bits else "")
        rng = np.random.RandomState(3 + bits + 10 * inverse)
        self.tm = [_time_major(rng, TP, CP, k) for k in range(3)]
        if bits:
            cb = 1024 * 2 * bits
            self.off, self.stride = np.arange(CP, dtype=np.uint64) * np.uint64(cb), CP * cb
            self.cm = [_blocked(t, bits, 0 if inverse else CANARY) for t in self.tm]
        else:
            pitch = (TP + 15) // 16 * 16 + 48
            self.off, self.stride = np.arange(CP, dtype=np.uint64) * np.uint64(pitch), 0
            self.cm = []
            for t in self.tm:
                buf = np.full(CP * pitch, 0 if inverse else CANARY, np.uint8)
                for c in range(CP):
                    buf[c * pitch:c * pitch + TP] = t[:, c]
                self.cm.append(buf)
        self.d_off = _const(_i64(self.off))
        self.src = self.inp(self.cm if inverse else self.tm)
        self.o = self.out(TP * CP if inverse else len(self.cm[0]))

    def call(self, st):
        L, off = _lib(), ct.c_void_p(self.d_off.data_ptr())
        if self.bits and self.inverse:
            _ok(L.mh_interleave_packed(self.src.ptr, off, TP, CP, self.bits, self.stride, self.o.ptr, st))
        elif self.bits:
            _ok(L.mh_deinterleave_packed(self.src.ptr, TP, CP, self.bits, self.o.ptr, off, self.stride, st))
        elif self.inverse:
            _ok(L.mh_interleave(self.src.ptr, off, TP, CP, self.o.ptr, st))
        else:
            _ok(L.mh_deinterleave(self.src.ptr, TP, CP, self.o.ptr, off, st))

    def verify(self, k):
        if self.inverse:
            want = np.minimum(self.tm[k], (1 << self.bits) - 1) if self.bits else self.tm[k]
            want = want.reshape(-1)
        else:
            want = self.cm[k]
        assert np.array_equal(self.o.host(), want), (self.name, k)


class Sweep(Case):
    name = "mh_sweep_run"

    def __init__(self, lens=(3, 100, 5000, 3 * CH + 5, 300000)):
        super().__init__()
        rng = np.random.RandomState(5)
        self.lens = list(lens)
        self.hb = np.array([2, 6, 10, 14], np.uint32)
        self.sets = [[np.minimum(rng.poisson(lam, size=T), 255).astype(np.uint8) for T in self.lens] for lam in (0.1, 4.0, 12.0)]
        flat = [OC.flatten(s) for s in self.sets]
        self.off, self.ln = flat[0][1], flat[0][2]
        self.data = self.inp([f[0] for f in flat])
        h_ = ct.c_void_p()
        _ok(_lib().mh_sweep_create(ct.byref(h_), self.off.ctypes.data, self.ln.ctypes.data, len(self.lens),
                                   self.hb.ctypes.data, len(self.hb)))
        self.h = h_
        self.ni = 2 * len(self.hb) + 1
        self.o = self.out(len(self.lens) * self.ni * 10 * 8)

    def call(self, st):
        _ok(_lib().mh_sweep_run(self.h, self.data.ptr, self.o.ptr, st))

    def verify(self, k):
        got = self.o.host(np.uint64).reshape(len(self.lens), self.ni, 10)
        for c, x in enumerate(self.sets[k]):
            T = len(x)
            b = [0, T]
            for h in self.hb:
                cut = min(1 << int(h), T)
                b += [cut, min(cut + T // 2, T)]
            b = sorted(b)
            for j in range(self.ni):
                want = np.bincount(np.minimum(x[b[j]:b[j + 1]], 9), minlength=10)
                assert np.array_equal(got[c, j], want), (self.name, k, c, j)

    def close(self):
        if self.h:
            _lib().mh_sweep_destroy(self.h)
            self.h = None


class PowerDraws(Case):
    """x[d * stride] += comm * np.sum(br[idx[:, d]]) + per_channels + static: x is input and output"""
    name = "mh_power_draws"
    ND, Z, NBR, STRIDE = 1000, 5, 37, 2

    def __init__(self):
        super().__init__()
        rng = np.random.RandomState(6)
        self.br = [rng.rand(self.NBR) * 10.0 ** e for e in (3, 5, 1)]
        self.idx = [rng.randint(0, self.NBR, size=(self.Z, self.ND)).astype(np.int32) for _ in range(3)]
        self.x0 = [rng.rand(self.ND * self.STRIDE) for _ in range(3)]
        self.d_br, self.d_idx, self.x = self.inp(self.br), self.inp(self.idx), self.inp(self.x0)
        self.pin = torch.empty(self.ND * self.STRIDE * 8, dtype=torch.uint8).pin_memory()

    def fetch(self):
        self.pin.copy_(self.x.buf, non_blocking=True)

    def call(self, st):
        _ok(_lib().mh_power_draws(self.d_br.ptr, self.NBR, self.d_idx.ptr, self.Z, self.ND, 20e-9, 4.8e-6, 0.1618e-3,
                                  self.x.ptr, self.STRIDE, st))

    def verify(self, k):
        want = self.x0[k].copy()
        for d in range(self.ND):
            s = np.sum(self.br[k][self.idx[k][:, d]])          # fewer than 8 terms: NumPy adds them in order
            want[d * self.STRIDE] = want[d * self.STRIDE] + (20e-9 * s + 4.8e-6 + 0.1618e-3)
        assert helpers.same_float(self.pin.numpy().view(np.float64), want), (self.name, k)


class ReduceRows(Case):
    name = "mh_reduce_rows"

    def __init__(self):
        super().__init__()
        rng = np.random.RandomState(7)
        self.lens = [1, 7, 8, 129, 1000, 4097]
        self.roff = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.vals = [rng.rand(int(self.roff[-1])) * 10.0 ** rng.randint(-3, 6, size=int(self.roff[-1])) for _ in range(3)]
        self.vals[2][int(self.roff[3]) + 5] = np.nan
        self.v = self.inp(self.vals)
        self.d_off = _const(_i64(self.roff))
        self.s, self.m = self.out(8 * len(self.lens)), self.out(8 * len(self.lens))

    def call(self, st):
        _ok(_lib().mh_reduce_rows(self.v.ptr, ct.c_void_p(self.d_off.data_ptr()), len(self.lens), self.s.ptr, self.m.ptr, st))

    def verify(self, k):
        rows = [self.vals[k][int(a):int(b)] for a, b in zip(self.roff[:-1], self.roff[1:])]
        assert helpers.same_float(self.s.host(np.float64), [np.sum(r) for r in rows]), (self.name, k)
        assert helpers.same_float(self.m.host(np.float64), [np.max(r) for r in rows]), (self.name, k)


class StreamBlock(Case):
    """The stream path of stream.py on one block [TP, CP], chunk-blocked packed intermediate, word of the next dataset:
    kind 'tx' = mh_deinterleave_packed -> mh_encode_preset -> mh_compact (checked against oracle.c.encode_preset),
    kind 'rx' = mh_decode_packed -> mh_interleave_packed (a NumPy transpose of the clipped block),
    kind 'decode_packed' = mh_decode_packed alone (the pieces)."""

    def __init__(self, mh, kind, S):
        super().__init__()
        self.kind, self.S, self.name = kind, S, "%s[S=%d]" % (kind, S)
        rng = np.random.RandomState(8 + S)
        self.rows = helpers.sclv_tables()[S]
        self.bits = 2 if S <= 4 else 4
        cb = 1024 * 2 * self.bits
        self.stride = CP * cb
        self.tm = [_time_major(rng, TP, CP, k) for k in range(3)]
        self.p = OC.Params(S, 0, 1, OC.WIN_FULL, self.rows, seg_chunks=2)
        ln = np.full(CP, TP, np.uint64)
        poff = np.arange(CP, dtype=np.uint64) * np.uint64(cb)
        self.plan = mh.codec.Plan(poff, ln, S, 0, 1, mh.WIN_FULL, self.rows, seg_chunks=2, input_bits=self.bits,
                                  chunk_stride=self.stride)
        self.d_off = _const(_i64(poff))
        # the RAM word of dataset k: calibrated on 64 quiet steps for k = 0, 2 (dataset 2 then sits on its longest
        # code), on busy ones for k = 1
        words = []
        for k in range(3):
            cal = np.minimum(rng.poisson((0.05, 3.0, 0.05)[k], size=(64, CP)), 255).astype(np.uint8)
            d, o, n = OC.flatten([cal[:, c].copy() for c in range(CP)])
            m = OC.measure(d, o, n, OC.Params(S, 6, 1, OC.WIN_FULL, self.rows))
            words.append((m["peak"].copy(), m["enc"].copy()))
        self.oe = []
        for k in range(3):
            d, o, n = OC.flatten([self.tm[k][:, c].copy() for c in range(CP)])
            self.oe.append(OC.encode_preset(d, o, n, self.p, words[k][0], words[k][1]))
        self.cap = self.oe[0]["payload"].size
        self.nseg = len(self.oe[0]["seg"]["ch"])
        assert self.plan.n_segments == self.nseg and self.plan.payload_cap_words == self.cap
        self.used = [_used_mask(oe["seg"]["off"], oe["seg_words"], self.cap) for oe in self.oe]
        self.pk, self.en = self.inp([w[0] for w in words]), self.inp([w[1] for w in words])
        npieces = len(_blocked(self.tm[0], self.bits, 0))
        if kind == "tx":
            self.src = self.inp(self.tm)
            self.pieces = torch.zeros(npieces + 16, dtype=torch.uint8, device="cuda")
            self.pay = torch.zeros(self.cap, dtype=torch.int32, device="cuda")
            self.segw, self.chb = self.out(8 * self.nseg), self.out(8 * CP)
            self.dense, self.doff, self.tot = self.out(4 * self.cap), self.out(8 * self.nseg), self.out(8)
        else:
            self.pay = self.inp([oe["payload"][u] for oe, u in zip(self.oe, self.used)], slack=16)
            self.soff = self.inp([_i64(np.concatenate([[0], np.cumsum(oe["seg_words"])[:-1]])) for oe in self.oe])
            self.pieces = self.out(npieces)
            if kind == "rx":
                self.o = self.out(TP * CP)

    def call(self, st):
        L, h, off = _lib(), self.plan._h, ct.c_void_p(self.d_off.data_ptr())
        if self.kind == "tx":
            pc, pay = ct.c_void_p(self.pieces.data_ptr()), ct.c_void_p(self.pay.data_ptr())
            _ok(L.mh_deinterleave_packed(self.src.ptr, TP, CP, self.bits, pc, off, self.stride, st))
            _ok(L.mh_encode_preset(h, pc, self.pk.ptr, self.en.ptr, pay, self.cap, self.segw.ptr, self.chb.ptr, st))
            _ok(L.mh_compact(h, pay, self.segw.ptr, self.dense.ptr, self.cap, self.doff.ptr, self.tot.ptr, st))
            return
        _ok(L.mh_decode_packed(h, self.pay.ptr, self.pay.buf.numel() // 4, self.soff.ptr, self.pk.ptr, self.en.ptr,
                               self.pieces.ptr, st))
        if self.kind == "rx":
            _ok(L.mh_interleave_packed(self.pieces.ptr, off, TP, CP, self.bits, self.stride, self.o.ptr, st))

    def verify(self, k):
        oe, tag = self.oe[k], (self.name, k)
        if self.kind == "tx":
            total = int(oe["seg_words"].sum())
            assert np.array_equal(self.segw.host(np.uint64), oe["seg_words"]), tag
            assert np.array_equal(self.chb.host(np.uint64), oe["ch_bits"]), tag
            assert int(self.tot.host(np.uint64)[0]) == total, tag
            assert np.array_equal(self.doff.host(np.uint64), np.concatenate([[0], np.cumsum(oe["seg_words"])[:-1]])), tag
            assert np.array_equal(self.dense.host(np.uint32)[:total], oe["payload"][self.used[k]]), tag
            return
        clip = np.minimum(self.tm[k], self.S - 1)
        assert np.array_equal(self.pieces.host(), _blocked(clip, self.bits, CANARY)), tag
        if self.kind == "rx":
            assert np.array_equal(self.o.host(), clip.reshape(-1)), tag

    def status(self):
        flags = ct.c_uint32(7)
        _ok(_lib().mh_decode_status(self.plan._h, ct.byref(flags), None))
        return flags.value

    def close(self):
        self.plan.close()


# (id, entry points it covers, factory(mh)); the plan cases run on the small layouts a (wave tasks, S = 3), c (wave
# tasks, tiled calibration, S = 10) and d (workgroup tasks, k_lut_preset, heads, S = 7)
def _plan_factory(layout, kind, variant, **kw):
    def make(mh):
        b = Bench(mh, _world(layout))
        c = b.case(kind, variant)
        if kw:
            c.set(**kw)
        c.close = b.close
        return c
    return make


CASES = []
for _l in ("a", "c", "d"):
    CASES += [("measure-%s" % _l, "mh_measure", _plan_factory(_l, "measure", 0)),
              ("measure_bits-%s" % _l, "mh_measure", _plan_factory(_l, "measure", 1)),
              ("encode-%s" % _l, "mh_encode", _plan_factory(_l, "encode", 0)),
              ("encode_null-%s" % _l, "mh_encode", _plan_factory(_l, "encode", 1)),
              ("encode_preset-%s" % _l, "mh_encode_preset", _plan_factory(_l, "encode", 2)),
              ("decode-%s" % _l, "mh_decode", _plan_factory(_l, "decode", 0)),
              ("decode_dense-%s" % _l, "mh_decode", _plan_factory(_l, "decode", 1)),
              ("compact-%s" % _l, "mh_compact", _plan_factory(_l, "compact", 0)),
              ("decode_status-%s" % _l, "mh_decode_status", _plan_factory(_l, "decode", 2)),
              ("decode_range-%s" % _l, "mh_decode_range", _plan_factory(_l, "range", 0, q=0)),
              ("decode_range_dense-%s" % _l, "mh_decode_range", _plan_factory(_l, "range", 0, q=1, dense=True)),
              ("decode_rebin_u8-%s" % _l, "mh_decode_rebin", _plan_factory(_l, "range", 1, q=0, r=5, sat=True)),
              ("decode_rebin_u32-%s" % _l, "mh_decode_rebin", _plan_factory(_l, "range", 1, q=1, r=16, sat=False, dense=True))]
CASES += [("synth_poisson", "mh_synth_poisson", lambda mh: Synth()),
          ("rebin_r5_u8", "mh_rebin", lambda mh: Rebin(5, True)),
          ("rebin_r3_u32", "mh_rebin", lambda mh: Rebin(3, False)),
          ("rebin_r7_u32", "mh_rebin", lambda mh: Rebin(7, False)),
          ("deinterleave", "mh_deinterleave", lambda mh: Transpose(0, False)),
          ("interleave", "mh_interleave", lambda mh: Transpose(0, True)),
          ("deinterleave_packed2", "mh_deinterleave_packed", lambda mh: Transpose(2, False)),
          ("deinterleave_packed4", "mh_deinterleave_packed", lambda mh: Transpose(4, False)),
          ("interleave_packed2", "mh_interleave_packed", lambda mh: Transpose(2, True)),
          ("interleave_packed4", "mh_interleave_packed", lambda mh: Transpose(4, True)),
          ("decode_packed_S3", "mh_decode_packed", lambda mh: StreamBlock(mh, "decode_packed", 3)),
          ("decode_packed_S8", "mh_decode_packed", lambda mh: StreamBlock(mh, "decode_packed", 8)),
          ("sweep_run", "mh_sweep_run", lambda mh: Sweep()),
          ("power_draws", "mh_power_draws", lambda mh: PowerDraws()),
          ("reduce_rows", "mh_reduce_rows", lambda mh: ReduceRows())]
PIPELINES = [("transmit_S3", None, lambda mh: StreamBlock(mh, "tx", 3)),
             ("transmit_S8", None, lambda mh: StreamBlock(mh, "tx", 8)),
             ("receive_S3", None, lambda mh: StreamBlock(mh, "rx", 3)),
             ("receive_S8", None, lambda mh: StreamBlock(mh, "rx", 8))]


def test_the_cases_cover_the_table():
    covered = {e for _, e, _ in CASES}
    assert covered == set(at.of_class(at.CAPTURABLE)) | {"mh_decode_status", "mh_decode_range", "mh_decode_rebin"}


# ---------------------------------------------------------------------------------------------------------------------
# 3a

_delay_buf = []


def _delay():
    if not _delay_buf:
        _delay_buf.append(torch.zeros(DELAY_BYTES // 4, dtype=torch.int32, device="cuda"))
    for _ in range(DELAY_PASSES):
        _delay_buf[0].add_(1)


@pytest.mark.parametrize("ident,entry,make", CASES, ids=[c[0] for c in CASES])
def test_stream_order(mh, ident, entry, make):
    case = make(mh)
    try:
        side = torch.cuda.Stream()
        st = ct.c_void_p(side.cuda_stream)
        with torch.cuda.stream(side):
            case.load(0)
            case.reset()
            case.call(st)                      # warm-up, and the oracle on A
            case.fetch()
        side.synchronize()
        case.verify(0)
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        t_dev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        with torch.cuda.stream(side):
            t_dev[0].record()
            _delay()
            t_dev[1].record()
            ev.record()
            t0 = time.perf_counter()
            case.call(st)                      # A once more, behind the delay: dirties every scratch word again
            case.reset()
            case.load(1)                       # B into the same buffers
            case.call(st)
            t1 = time.perf_counter()
            pending = not ev.query()
            case.fetch()
        side.synchronize()
        print("\n%s: host enqueue %.3f ms, delay %.3f ms on the device, event %s" %
              (ident, 1e3 * (t1 - t0), t_dev[0].elapsed_time(t_dev[1]), "pending" if pending else "complete"))
        case.verify(1)
        if at.CLASS[entry] == at.CAPTURABLE:
            assert not case.sync
            assert pending, ("%s: the delay had completed when the call returned -- either the call blocked on the "
                             "stream or the delay is too short for this machine (host enqueue %.3f ms)"
                             % (ident, 1e3 * (t1 - t0)))
        else:
            assert case.sync
    finally:
        case.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3b

def _replay(mh, make):
    case = make(mh)
    try:
        side = torch.cuda.Stream()
        st = ct.c_void_p(side.cuda_stream)
        with torch.cuda.stream(side):
            case.load(0)
            case.reset()
            case.call(st)                      # warm-up outside capture
            case.fetch()
        side.synchronize()
        case.verify(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            case.call(st)
        for k in (1, 2, 0, 2):                 # same buffers, other contents (and another preset word) every time
            with torch.cuda.stream(side):
                case.load(k)
                case.reset()
                g.replay()
                case.fetch()
            side.synchronize()
            case.verify(k)
        return case
    except BaseException:
        case.close()
        raise


@pytest.mark.parametrize("ident,entry,make", [c for c in CASES if at.CLASS[c[1]] == at.CAPTURABLE],
                         ids=[c[0] for c in CASES if at.CLASS[c[1]] == at.CAPTURABLE])
def test_graph_replay(mh, ident, entry, make):
    case = _replay(mh, make)
    try:
        if isinstance(case, PlanCase):
            assert case.b.status(None) == 0
        elif isinstance(case, StreamBlock):
            assert case.status() == 0
    finally:
        case.close()


@pytest.mark.parametrize("ident,entry,make", PIPELINES, ids=[c[0] for c in PIPELINES])
def test_pipeline_graph_replay(mh, ident, entry, make):
    case = _replay(mh, make)
    try:
        assert case.status() == 0
    finally:
        case.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3c

KINDS = ("measure", "encode", "encode_preset", "decode", "decode_abandoned", "decode_range", "decode_rebin", "compact")


def _sequence(seed):
    """an Eulerian circuit of the complete directed graph on KINDS (Hierholzer, successors in a seeded random order):
    every ordered pair of distinct kinds exactly once, 57 calls"""
    rng = np.random.RandomState(seed)
    n = len(KINDS)
    nxt = {u: [v for v in rng.permutation(n) if v != u] for u in range(n)}
    stack, path = [int(rng.randint(n))], []
    while stack:
        u = stack[-1]
        if nxt[u]:
            stack.append(int(nxt[u].pop()))
        else:
            path.append(stack.pop())
    return [KINDS[u] for u in reversed(path)]


def _run_sequence(mh, layout, seq, seed):
    """Runs `seq` on ONE plan of the layout, on a side stream of its own, rotating the datasets; every call is checked
    against the oracle for the dataset it was given.  Then a second plan of the same layout."""
    w = _world(layout)
    rng = np.random.RandomState(seed)
    side = torch.cuda.Stream()
    st = ct.c_void_p(side.cuda_stream)
    b = Bench(mh, w)
    cases = dict(measure=[b.case("measure", 0), b.case("measure", 1)],
                 encode=[b.case("encode", 0), b.case("encode", 1)],
                 encode_preset=[b.case("encode", 2)],
                 decode=[b.case("decode", 0), b.case("decode", 1)],
                 decode_abandoned=[b.case("decode", 2)],
                 decode_range=[b.case("range", 0)],
                 decode_rebin=[b.case("range", 1)],
                 compact=[b.case("compact", 0)])
    seen = {k: 0 for k in KINDS}

    def run(case, k):
        with torch.cuda.stream(side):
            case.load(k)
            case.reset()
            case.call(st)
            case.fetch()
        side.synchronize()
        case.verify(k)

    try:
        k = 0
        for step, kind in enumerate(seq):
            k = (k + 1 + int(rng.randint(2))) % 3          # never the dataset of the previous call
            i = seen[kind]
            seen[kind] += 1
            case = cases[kind][i % len(cases[kind])]
            if kind in ("decode_range", "decode_rebin"):
                # queries 0 0 1 1 2 2 3 ...: the same query twice in a row (the list is reused, on other data) and then
                # a different one; slots and compacted stream, both bin factors and both output types in turn
                case.set(q=(i // 2) % len(w.queries), dense=i % 3 == 1, r=(5, 16)[(i // 2) % 2], sat=i % 4 < 2)
            try:
                if kind == "decode_abandoned":
                    run(case, 1)                            # the all-zero payload: flagged, and the flag cleared
                    run(case, (0, 2)[i % 2])                # then a good decode, which reports clean
                else:
                    run(case, k)
                    if kind.startswith("decode"):
                        assert b.status(st) == 0
            except AssertionError as e:
                raise AssertionError("layout %s, step %d (%s after %s): %s" % (layout, step, kind, seq[step - 1] if step else "-", e))
        assert b.status(st) == 0
    finally:
        b.close()
    # state kept outside the plan: a second plan of the same layout starts clean
    b2 = Bench(mh, w)
    try:
        for kind, v, k in (("measure", 0, 2), ("encode", 1, 1), ("encode", 0, 2)):
            case = b2.case(kind, v)
            with torch.cuda.stream(side):
                case.load(k)
                case.reset()
                case.call(st)
                case.fetch()
            side.synchronize()
            case.verify(k)
    finally:
        b2.close()


def test_the_sequence_holds_every_ordered_pair_of_kinds():
    seq = _sequence(2024)
    pairs = set(zip(seq[:-1], seq[1:]))
    assert pairs == {(a, b) for a in KINDS for b in KINDS if a != b}
    assert len(seq) == len(KINDS) * (len(KINDS) - 1) + 1 >= 36
    assert all(seq.count(k) >= 7 for k in KINDS)        # every variant and every query of a kind gets its turn


@pytest.mark.parametrize("layout", [l.name for l in at.LAYOUTS])
def test_plan_state_across_a_mixed_sequence(mh, layout):
    seq = _sequence(2024)
    pairs = set(zip(seq[:-1], seq[1:]))
    assert pairs == {(a, b) for a in KINDS for b in KINDS if a != b}, "the sequence was thinned out"
    _run_sequence(mh, layout, seq, seed=11)


class PackedMeasure(Case):
    """mh_measure of a packed plan (contiguous `bits`-bit pieces, S symbols) over the lengths of world w, on w's datasets
    clipped to the piece width; the oracle measures the clipped bytes with the whole-channel window"""

    def __init__(self, mh, w, bits, S):
        super().__init__()
        l, self.C, self.S, self.name = w.l, w.C, S, "measure_packed[%s,%d]" % (w.l.name, bits)
        rows = helpers.sclv_tables()[S]
        sets = [[np.minimum(d[int(o):int(o) + T], (1 << bits) - 1) for o, T in zip(w.off, l.lens)] for d in w.data]
        size = [((T + 15) // 16 * 2 * bits + 15) // 16 * 16 + 16 for T in l.lens]
        off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64)
        images = []
        for chans in sets:
            buf = np.full(sum(size), CANARY, np.uint8)
            for x, o in zip(chans, off):
                pk = _pieces(x, bits).reshape(-1)
                buf[int(o):int(o) + len(pk)] = pk
            images.append(buf)
        p = OC.Params(S, l.h, l.mode, OC.WIN_FULL, rows)
        self.om = [OC.measure(*OC.flatten(chans), p, nthreads=NT) for chans in sets]
        self.plan = mh.codec.Plan(off, np.array(l.lens, np.uint64), S, l.h, l.mode, mh.WIN_FULL, rows, seg_chunks=1,
                                  input_bits=bits)
        self.data = self.inp(images)
        C = self.C
        self.o = [self.out(n) for n in (8 * C, 4 * C * S, C, C, 8 * C * S, 8 * C, C)]

    def call(self, st):
        cut, cal, pk, en, post, bits, sk = (g.ptr for g in self.o)
        _ok(_lib().mh_measure(self.plan._h, self.data.ptr, cut, cal, pk, en, post, bits, sk, st))

    def verify(self, k):
        for g, key, dt in zip(self.o, ("cutoff", "cal_sorted", "peak", "enc", "post_mapped", "bits", "skipped"),
                              (np.uint64, np.uint32, np.uint8, np.uint8, np.uint64, np.uint64, np.uint8)):
            assert np.array_equal(g.host(dt), self.om[k][key].reshape(-1)), (self.name, k, key)

    def close(self):
        self.plan.close()


def test_six_handles_alive_at_once(mh):
    """Every plan and sweep handle keeps its device tables and scratch in one allocation of its own
    (csrc/mh_plan_arena.hpp).  Byte plans of layouts a, c and d, a 4-bit and a 2-bit packed plan and a sweep handle over
    layout a's lengths, all alive: measure, encode and decode on the byte plans in an interleaved order, measure on the
    packed pieces, the sweep; three handles destroyed in another order than they were made, the rest run once more.
    Arenas that alias, a region sized short or a view taken before its arena exists show as a result that differs from
    the oracle (or as a write outside an output)."""
    side = torch.cuda.Stream()
    st = ct.c_void_p(side.cuda_stream)

    def run(case, k):
        with torch.cuda.stream(side):
            case.load(k)
            case.reset()
            case.call(st)
            case.fetch()
        side.synchronize()
        case.verify(k)

    alive = []
    try:
        benches = {}
        for name in ("a", "c", "d"):
            benches[name] = Bench(mh, _world(name))
            alive.append(benches[name])
        p4, p2 = PackedMeasure(mh, _world("a"), 4, 5), PackedMeasure(mh, _world("a"), 2, 3)
        alive += [p4, p2]
        sweep = Sweep(at.BY_NAME["a"].lens)
        alive.append(sweep)
        ops = {n: [b.case("measure", 0), b.case("encode", 0), b.case("decode", 0)] for n, b in benches.items()}
        for i in range(3):                                  # a measures while c encodes and d decodes, then they rotate
            for j, name in enumerate(("a", "c", "d")):
                run(ops[name][(i + j) % 3], (i + 2 * j) % 3)
        run(p4, 1)
        run(p2, 2)
        run(sweep, 0)
        for b in benches.values():
            assert b.status(st) == 0
        for gone in (sweep, benches["c"], p4):              # made third from last, second and fourth
            gone.close()
            alive.remove(gone)
        for i, name in enumerate(("d", "a")):
            for j in (1, 2, 0):                             # encode, decode, measure on another dataset
                run(ops[name][j], (i + j + 1) % 3)
            assert benches[name].status(st) == 0
        run(p2, 0)
    finally:
        for h in alive:
            h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3d

def test_two_host_threads_with_a_plan_and_a_stream_each(mh):
    """layout a on one thread, b on the other, each a shuffled sequence on its own plan and side stream, at once"""
    for name in ("a", "b"):
        _world(name)                                        # (the oracle runs before the threads start)
    errors = {}
    start = threading.Barrier(2)

    def work(name, seed):
        try:
            torch.cuda.set_device(0)
            start.wait(timeout=600)
            _run_sequence(mh, name, _sequence(seed)[:17], seed)
        except BaseException as e:   # noqa: B036  (reported in the main thread)
            errors[name] = e

    ts = [threading.Thread(target=work, args=("a", 5)), threading.Thread(target=work, args=("b", 6))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_last_error_is_thread_local(mh):
    L = _lib()
    step = threading.Barrier(2)
    seen = {}

    def thread_b():
        code = np.zeros(16, np.uint16)
        ln = np.zeros(16, np.uint8)
        row = np.array([1, 1, 2], np.uint8)                  # Kraft sum above 1
        seen["b_rc"] = L.mh_codebook(row.ctypes.data, 3, code.ctypes.data, ln.ctypes.data)
        seen["b_before"] = L.mh_last_error()
        step.wait(timeout=60)                                # A fails now
        step.wait(timeout=60)
        seen["b_after"] = L.mh_last_error()

    def thread_a():
        step.wait(timeout=60)
        seen["a_rc"] = L.mh_rebin(None, None, None, 0, 0, 0, 0, None, None, None)
        seen["a_msg"] = L.mh_last_error()
        step.wait(timeout=60)

    ts = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert seen["a_rc"] == mh._lib.ERR_ARG and b"mh_rebin" in seen["a_msg"]
    assert seen["b_rc"] == mh._lib.ERR_SCLV and b"SCLV" in seen["b_before"]
    assert seen["b_after"] == seen["b_before"] and seen["b_after"] != seen["a_msg"]
