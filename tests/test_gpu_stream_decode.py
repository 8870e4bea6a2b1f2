"""The receiving side of the stream path on the device: mh_interleave_packed, mh_decode_packed (every packed-output
decoder instance, kernel_cells.PACKED_DECODER_CELLS) and stream.StreamDecoder.  Expected values come from the CPU
oracle (streams, decodes) or from plain torch / NumPy ops (bit packing, clipping), never from the kernels under test."""
import ctypes as ct

import numpy as np
import pytest
import torch

import oracle
from tests import helpers
from tests import kernel_cells as kc
from tests.test_gpu_parity import _bitpack

pytestmark = pytest.mark.gpu

OC = oracle.c
CANARY = 0xAB
GiB = 1 << 30


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, stream  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    return muahuff


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(nbytes, what):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    assert nbytes < free, "%s needs ~%.1f GB of free HBM; %.1f GB free" % (what, nbytes / 1e9, free / 1e9)


# ---- host-side layout of packed pieces ----------------------------------------------------------------------------
def _layout(lens, bits, blocked, gap=16):
    """-> (ch_off uint64, chunk_stride, buffer bytes) of a packed buffer: contiguous pieces with `gap` canary bytes
    between channels, or chunk-blocked (chunk j of channel c at c * cb + j * C * cb) as StreamEncoder lays it out"""
    pb = 2 * bits
    cb = 1024 * pb
    C = len(lens)
    if blocked:
        nch = max((T + kc.CHUNK - 1) // kc.CHUNK for T in lens)
        return np.arange(C, dtype=np.uint64) * np.uint64(cb), C * cb, nch * C * cb + 64
    sz = [((T + 15) // 16 * pb + 15) // 16 * 16 + gap for T in lens]
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    return off, 0, int(sum(sz)) + 64


def _expected_pieces(chans, S, bits, off, stride, size):
    """canary buffer with min(x, S-1) of every channel packed where the layout puts its pieces"""
    want = np.full(size, CANARY, np.uint8)
    mask = np.zeros(size, bool)
    pb = 2 * bits
    cb = 1024 * pb
    for c, x in enumerate(chans):
        T = len(x)
        s = np.zeros((T + 15) // 16 * 16, np.uint8)
        s[:T] = np.minimum(x, S - 1)
        pk = _bitpack(s.reshape(-1, 16), bits).reshape(-1)
        o = int(off[c])
        if stride:
            for j in range(0, len(pk), cb):
                a = o + (j // cb) * stride
                want[a:a + len(pk[j:j + cb])] = pk[j:j + cb]
                mask[a:a + len(pk[j:j + cb])] = True
        else:
            want[o:o + len(pk)] = pk
            mask[o:o + len(pk)] = True
    return want, mask


def _stream_case(rng, S, rows, lens, sc, pattern, mode=1):
    """channels + the oracle's preset stream of them (slot layout), with a random word per channel"""
    C = len(lens)
    K = len(rows)
    peak = rng.randint(0, S, size=C).astype(np.uint8)
    enc = rng.randint(0, K, size=C).astype(np.uint8)
    chans = []
    for c, T in enumerate(lens):
        if pattern == "long" and c % 2 == 0:      # every sample on the longest code: oversize chunks, slow paths
            order = OC.approx_sort_rule(S, int(peak[c])) if mode == 1 else np.arange(S)
            x = np.full(T, order[S - 1], np.uint8)
        else:
            x = rng.poisson(float(np.exp(rng.uniform(np.log(0.05), np.log(6.0)))), size=T)
            x[rng.random_sample(T) < 0.02] = 200
            x = np.minimum(x, 255).astype(np.uint8)
        chans.append(x)
    data, off, ln = OC.flatten(chans)
    p = OC.Params(S, 6, mode, OC.WIN_FULL, np.asarray(rows, np.uint8), seg_chunks=sc)
    oe = OC.encode_preset(data, off, ln, p, peak, enc)
    return chans, oe, p


def _dense(oe):
    """the oracle's slotted stream compacted on the host: (words + 4 of slack, dense segment offsets)"""
    segs = [oe["payload"][int(o):int(o) + int(n)] for o, n in zip(oe["seg"]["off"], oe["seg_words"])]
    pay = np.concatenate(segs + [np.zeros(4, np.uint32)])
    off = np.concatenate([[0], np.cumsum(oe["seg_words"])[:-1]]).astype(np.int64)
    return pay, off


def _encoded(mh, pay, seg_words, peak, enc, seg_off=None):
    from muahuff.codec import Encoded
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    return Encoded(t(pay.view(np.int32), np.int32), t(seg_words, np.int64), torch.zeros(len(peak), dtype=torch.int64, device=dev),
                   t(peak, np.uint8), t(enc, np.uint8), torch.zeros(len(peak), dtype=torch.uint8, device=dev),
                   None if seg_off is None else t(seg_off, np.int64), seg_off is not None)


# ---- 1. mh_interleave_packed ----------------------------------------------------------------------------------------
def _pack_dev(x, bits):
    """[T, C] device counts -> [C, npc * 2 * bits] packed pieces of min(x, 2^bits - 1) (torch ops)"""
    T, C = x.shape
    npc = (T + 15) // 16
    s = torch.zeros((C, npc * 16), dtype=torch.int32, device=x.device)
    s[:, :T] = torch.clamp(x, max=(1 << bits) - 1).t().to(torch.int32)
    per = 8 // bits
    g = s.view(C, npc * 16 // per, per)
    by = torch.zeros(g.shape[:2], dtype=torch.int32, device=x.device)
    for f in range(per):
        by |= g[:, :, f] << (bits * f)
    return by.to(torch.uint8)


def _place_dev(pk, bits, blocked, C):
    """packed [C, n] pieces -> (buffer, ch_off device int64, chunk_stride) in the contiguous or chunk-blocked layout"""
    n = pk.shape[1]
    cb = 1024 * 2 * bits
    if blocked:
        nch = (n + cb - 1) // cb
        buf = torch.full((nch * C * cb,), CANARY, dtype=torch.uint8, device=pk.device)
        padded = torch.zeros((C, nch * cb), dtype=torch.uint8, device=pk.device)
        padded[:, :n] = pk
        buf.view(nch, C, cb).copy_(padded.view(C, nch, cb).transpose(0, 1))
        return buf, torch.arange(C, dtype=torch.int64, device=pk.device) * cb, C * cb
    row = (n + 15) // 16 * 16 + 16
    buf = torch.full((C * row,), CANARY, dtype=torch.uint8, device=pk.device)
    buf.view(C, row)[:, :n] = pk
    return buf, torch.arange(C, dtype=torch.int64, device=pk.device) * row, 0


@pytest.mark.parametrize("bits", [2, 4])
def test_interleave_packed_layout_ragged_shapes(mh, bits):
    lib = mh._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7 + bits)
    i = 0
    for T in (1, 15, 16, 17, 16383, 16385, 3 * 16384 + 5):
        for C in (1, 3, 127, 128, 129, 1000):
            x = torch.randint(0, 256, (T, C), generator=g, device="cuda", dtype=torch.uint8)
            x[torch.rand((T, C), generator=g, device="cuda") < 0.5] = 0
            x[x > 40] = torch.randint(0, 1 << bits, (1,), generator=g, device="cuda", dtype=torch.uint8)
            pk = _pack_dev(x, bits)
            for blocked in ((False, True) if i % 3 == 0 else (bool(i % 2),)):
                buf, off, stride = _place_dev(pk, bits, blocked, C)
                out = torch.full((T * C + 64,), 0xCD, dtype=torch.uint8, device="cuda")
                mh._lib.check(lib.mh_interleave_packed(ct.c_void_p(buf.data_ptr()), ct.c_void_p(off.data_ptr()), T, C, bits,
                                                       stride, ct.c_void_p(out.data_ptr()), _st()))
                want = torch.clamp(x, max=(1 << bits) - 1).reshape(-1)
                assert torch.equal(out[:T * C], want), (T, C, blocked)
                assert bool((out[T * C:] == 0xCD).all()), ("wrote past T*C", T, C, blocked)
            i += 1


def test_interleave_packed_inverts_the_deinterleaver_above_the_store_switch(mh):
    """1024 x 1e6 steps, 2-bit chunk-blocked pieces (256 MB, above k_deinterleave_p's 192-MiB switch to non-temporal
    stores): interleave_packed(deinterleave_packed(x)) == min(x, 3), on the device."""
    lib = mh._lib.lib()
    T, C, bits = 1_000_000, 1024, 2
    _need(T * C * 3 + GiB, "the 1024 x 1e6 round trip")
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(0, 8, (T, C), generator=g, device="cuda", dtype=torch.uint8)
    cb = 1024 * 2 * bits
    nch = (T + kc.CHUNK - 1) // kc.CHUNK
    pieces = torch.zeros(nch * C * cb, dtype=torch.uint8, device="cuda")
    assert pieces.numel() > 192 * (1 << 20)
    off = torch.arange(C, dtype=torch.int64, device="cuda") * cb
    mh._lib.check(lib.mh_deinterleave_packed(ct.c_void_p(x.data_ptr()), T, C, bits, ct.c_void_p(pieces.data_ptr()),
                                             ct.c_void_p(off.data_ptr()), C * cb, _st()))
    out = torch.empty((T, C), dtype=torch.uint8, device="cuda")
    mh._lib.check(lib.mh_interleave_packed(ct.c_void_p(pieces.data_ptr()), ct.c_void_p(off.data_ptr()), T, C, bits, C * cb,
                                           ct.c_void_p(out.data_ptr()), _st()))
    assert torch.equal(out, torch.clamp(x, max=3))


# ---- 2. mh_decode_packed, every instance ----------------------------------------------------------------------------
def _cell_id(c):
    return c.key.replace("mh::", "").replace(" ", "")


@pytest.mark.parametrize("cell", kc.PACKED_DECODER_CELLS, ids=_cell_id)
def test_decode_packed_cell_against_the_oracle(mh, cell):
    import zlib
    rng = np.random.RandomState(zlib.crc32(cell.key.encode()) & 0x7FFFFFFF)
    for ci, k in enumerate(cell.cases):
        for li, (lens, sc) in enumerate(cell.layouts):
            blocked = (li + ci) % 2 == 1
            pattern = "long" if li % 2 == 0 else "poisson"
            chans, oe, _p = _stream_case(rng, k.S, k.rows, list(lens), sc, pattern, mode=(li % 2))
            off, stride, size = _layout(lens, cell.input_bits, blocked)
            plan = mh.codec.Plan(off, np.asarray(lens, np.uint64), k.S, 6, li % 2, mh.WIN_FULL, np.asarray(k.rows, np.uint8),
                                 seg_chunks=sc, input_bits=cell.input_bits, chunk_stride=stride)
            assert plan.n_segments == len(oe["seg_words"])
            want, _mask = _expected_pieces(chans, k.S, cell.input_bits, off, stride, size)
            tag = (cell.symbol, k.S, lens, sc, blocked, pattern)
            # the slotted stream (plan_slots) and the same stream compacted (dense seg_off)
            pay_d, off_d = _dense(oe)
            for form, e in (("slots", _encoded(mh, oe["payload"], oe["seg_words"], oe["peak"], oe["enc"])),
                            ("dense", _encoded(mh, pay_d, oe["seg_words"], oe["peak"], oe["enc"], off_d))):
                out = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
                plan.decode_packed(e, out)
                assert plan.decode_ok(), tag + (form,)
                got = out.cpu().numpy()
                assert np.array_equal(got, want), tag + (form, int(np.flatnonzero(got != want)[0]))
            plan.close()


# ---- 3. untrusted streams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 5, 10])
def test_decode_packed_never_writes_outside_its_pieces_on_an_untrusted_stream(mh, S):
    rng = np.random.RandomState(60 + S)
    tab = helpers.sclv_tables()[S]
    po = 2 if S <= 4 else 4
    for lens, sc, blocked in (((70001, 16384 * 3 + 17, 40000, 5, 200000, 16384), 1, False),
                              ((16384 * 5 + 3,) * 4, 2, True)):
        chans, oe, _p = _stream_case(rng, S, tab, list(lens), sc, "poisson")
        off, stride, size = _layout(lens, po, blocked)
        plan = mh.codec.Plan(off, np.asarray(lens, np.uint64), S, 6, 1, mh.WIN_FULL, tab, seg_chunks=sc, input_bits=po,
                             chunk_stride=stride)
        want, mask = _expected_pieces(chans, S, po, off, stride, size)
        pay, doff = _dense(oe)
        total = len(pay) - 4
        good = _encoded(mh, pay, oe["seg_words"], oe["peak"], oe["enc"], doff)
        bad = []
        bad.append(("truncated", _encoded(mh, pay[:total // 2], oe["seg_words"], oe["peak"], oe["enc"], doff), True))
        big = pay.copy()
        big[::7] = 0x7FFFFFFF
        bad.append(("huge headers", _encoded(mh, big, oe["seg_words"], oe["peak"], oe["enc"], doff), None))
        bad.append(("random words", _encoded(mh, rng.randint(0, 2 ** 31, size=total + 4).astype(np.uint32), oe["seg_words"],
                                             oe["peak"], oe["enc"], doff), None))
        bad.append(("wild offsets, bad word", _encoded(mh, pay, oe["seg_words"], np.full(len(lens), 200, np.uint8),
                                                      np.full(len(lens), 200, np.uint8),
                                                      np.full(len(doff), 2 ** 40, np.int64)), True))
        bad.append(("zeros", _encoded(mh, np.zeros_like(pay), oe["seg_words"], oe["peak"], oe["enc"], doff), True))
        for what, e, raised in bad:
            out = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
            plan.decode_packed(e, out)
            ok = plan.decode_ok()
            if raised:
                assert not ok, (S, what)
            got = out.cpu().numpy()
            assert np.all(got[~mask] == CANARY), (S, what, "wrote outside the pieces")
            # a good decode on the same plan right after is exact, with a clean status
            out = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
            plan.decode_packed(good, out)
            assert plan.decode_ok(), (S, what)
            assert np.array_equal(out.cpu().numpy(), want), (S, what)
        plan.close()


# ---- 4. StreamDecoder round trips -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 4, 5, 7, 10])
def test_stream_decoder_round_trip(mh, S):
    from muahuff import stream
    rng = np.random.RandomState(200 + S)
    tab = helpers.sclv_tables()[S]
    for C, lengths in ((70, [16384 * 9 + 5, 16384 * 2, 16383, 100, 17, 16, 1]),
                       (130, [16384 * 16 - 1, 16384 * 16, 16384 * 16 + 17])):
        rates = np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=C))

        def block(T):
            x = np.minimum(rng.poisson(rates, size=(T, C)), 255).astype(np.uint8)
            x[rng.random_sample((T, C)) < 0.01] = rng.randint(4, 256)
            return x
        se = stream.StreamEncoder(C, S, 6, tab)
        se.calibrate(block(64))
        sd = stream.StreamDecoder(C, S, tab)
        for i, T in enumerate(lengths):
            x = block(T)
            xd = torch.from_numpy(x).cuda()
            want = torch.clamp(xd, max=S - 1)
            dense, tot, slot = se.encode_block_device(xd)
            n = slot["plan"].n_segments
            got = sd.decode_block_device(dense.payload, dense.seg_words, se.peak, se.enc, T,
                                         seg_off=dense.seg_off if i % 2 else None)
            assert got.shape == (T, C) and got.dtype == torch.uint8
            assert torch.equal(got, want), (S, C, T)
            assert sd.ok(), (S, C, T)
            # the scanned offsets equal the compaction's
            if i % 2 == 0 and n > 1:
                assert torch.equal(sd._slots[T]["seg_off"][:n], dense.seg_off[:n]), (S, C, T)
            c = se.encode_block(x)
            old = stream.StreamEncoder.decode_block(c)
            assert np.array_equal(sd.decode_block(c), old), (S, C, T)
        sd.close()
        se.close()


# ---- 5. full size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 5])
def test_stream_decoder_at_full_size(mh, S):
    from muahuff import stream, synth
    C, T = 1024, 10_000_000
    bits = 2 if S <= 4 else 4
    tab = helpers.sclv_tables()[S]
    maxlen = int(tab.max())
    # x, encoder slot (pieces, slotted payload, dense), decoder slot (pieces, output)
    _need(T * C * (1 + bits / 8 + 2 * maxlen / 8 + bits / 8 + 1 + 0.25) + 4 * GiB, "the full-size stream round trip")
    cs = synth.generate(C, T, seed=S)
    x = cs.matrix().t().contiguous()
    del cs
    torch.cuda.empty_cache()
    g = torch.Generator(device="cuda").manual_seed(100 + S)
    idx = torch.randint(0, x.numel(), (x.numel() // 1000,), generator=g, device="cuda")
    x.view(-1)[idx] = torch.randint(0, 256, (idx.numel(),), generator=g, device="cuda", dtype=torch.uint8)
    se = stream.StreamEncoder(C, S, 6, tab)
    se.calibrate(x[:64])
    dense, tot, slot = se.encode_block_device(x)
    sd = stream.StreamDecoder(C, S, tab)
    got = sd.decode_block_device(dense.payload, dense.seg_words, se.peak, se.enc, T, seg_off=dense.seg_off)
    assert sd.ok()
    for t0 in range(0, T, 1 << 20):
        assert torch.equal(got[t0:t0 + (1 << 20)], torch.clamp(x[t0:t0 + (1 << 20)], max=S - 1)), (S, t0)
    sd.close()
    se.close()


# ---- 6. slots -------------------------------------------------------------------------------------------------------
def test_stream_decoder_slots_are_reused_and_follow_recalibration(mh):
    from muahuff import stream
    rng = np.random.RandomState(33)
    C, S = 20, 4
    tab = helpers.sclv_tables()[S]
    se = stream.StreamEncoder(C, S, 5, tab)
    sd = stream.StreamDecoder(C, S, tab)
    lo = lambda T: np.minimum(rng.poisson(0.1, size=(T, C)), 255).astype(np.uint8)
    hi = lambda T: (3 - np.minimum(rng.poisson(0.3, size=(T, C)), 3)).astype(np.uint8)
    se.calibrate(lo(32))
    ptrs = {}
    for rnd in range(3):
        for T in (40000, 16384 * 5 + 1):
            x = lo(T)
            dense, tot, slot = se.encode_block_device(x)
            if T in ptrs:
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
            got = sd.decode_block_device(dense.payload, dense.seg_words, se.peak, se.enc, T)
            if T in ptrs:
                assert torch.cuda.memory_allocated() == before, "a second block of a shape allocated"
                assert got.data_ptr() == ptrs[T]
            ptrs[T] = got.data_ptr()
            assert torch.equal(got, torch.from_numpy(np.minimum(x, S - 1)).cuda()), (rnd, T)
    peak0 = se.peak.clone()
    se.calibrate(hi(32))
    assert not torch.equal(peak0, se.peak)
    for T in (40000, 16384 * 5 + 1):
        x = hi(T)
        dense, tot, slot = se.encode_block_device(x)
        got = sd.decode_block_device(dense.payload, dense.seg_words, se.peak, se.enc, T)
        assert torch.equal(got, torch.from_numpy(np.minimum(x, S - 1)).cuda()), T
    assert sd.ok()
    sd.close()
    se.close()


# ---- 7. decode_block(c) ---------------------------------------------------------------------------------------------
def test_stream_decoder_checked_host_form(mh):
    import copy

    from muahuff import stream
    rng = np.random.RandomState(34)
    C, S = 33, 5
    tab = helpers.sclv_tables()[S]
    se = stream.StreamEncoder(C, S, 6, tab)
    se.calibrate(np.minimum(rng.poisson(1.0, size=(64, C)), 255).astype(np.uint8))
    sd = stream.StreamDecoder(C, S, tab)
    x = np.minimum(rng.poisson(1.5, size=(70000, C)), 255).astype(np.uint8)
    c = se.encode_block(x)
    host = sd.decode_block(c)
    assert np.array_equal(host, np.minimum(x, S - 1))
    dense, tot, slot = se.encode_block_device(x)
    dev = sd.decode_block_device(dense.payload, dense.seg_words, se.peak, se.enc, 70000).cpu().numpy()
    assert np.array_equal(host, dev)
    for what, mutate in (("S", lambda h: h.__setitem__("S", 6)), ("seg_chunks", lambda h: h.__setitem__("seg_chunks", 1)),
                         ("mode", lambda h: h.__setitem__("mode", 0))):
        bad = copy.deepcopy(c)
        mutate(bad.header)
        with pytest.raises(ValueError):
            sd.decode_block(bad)
    bad = copy.deepcopy(c)
    bad.ch_len = bad.ch_len.copy()
    bad.ch_len[3] += 1
    with pytest.raises(ValueError):
        sd.decode_block(bad)
    bad = copy.deepcopy(c)
    bad.payload = bad.payload.copy()
    bad.payload[0] ^= 0xFFFF
    with pytest.raises(ValueError):
        sd.decode_block(bad)
    bad = copy.deepcopy(c)
    bad.payload = bad.payload[:-5].copy()
    with pytest.raises(ValueError):
        sd.decode_block(bad)
    sd.close()
    se.close()


def test_decode_packed_refuses_other_plans(mh):
    tab = helpers.sclv_tables()[3]
    lens = np.array([1000, 2000], np.uint64)
    byte_plan = mh.codec.Plan(np.array([0, 1024], np.uint64), lens, 3, 6, 1, mh.WIN_FULL, tab)
    e = byte_plan.alloc_encoded()
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(mh._lib.MuaHuffError):
        byte_plan.decode_packed(e, out)
    wide = mh.codec.Plan(np.array([0, 1024], np.uint64), lens, 3, 6, 1, mh.WIN_FULL, tab, input_bits=4)
    with pytest.raises(mh._lib.MuaHuffError):   # S <= 4 decodes to 2-bit pieces
        wide.decode_packed(e, out)
    byte_plan.close()
    wide.close()
