"""Segments that hold staged AND oversize chunks, through every entry point that walks a segment, against the CPU oracle
(tests/mixed_chunks.py has the scenarios; tests/test_host_mixed_chunks.py shows without a GPU that they are what they
claim, land on the intended kernel instances and reach every (rung, transition) pair that can be reached).

Per scenario -- one SCLV row, one seg_chunks, one task form -- exact comparisons only:

  mh_encode          seg_words, ch_bits and every used payload word equal the oracle's; the words in front of and behind
                     the payload buffer keep their canary (a slow chunk writes with plain stores at an unaligned dst)
  mh_encode_preset   4-bit pieces, contiguous and chunk-blocked, against the oracle's encode_preset
  mh_decode          the GPU's slotted stream and the oracle's dense one: the oracle's decode, the bytes between the
                     windows untouched, status 0
  mh_decode_packed   4-bit pieces, contiguous and chunk-blocked, every byte outside the pieces untouched
  mh_decode_range    the whole range, and around every oversize chunk: cut inside it (through scratch), over its first
                     and its last sample, passed over, and a start in the chunk behind it -- through
                     container_io.decompress_range and into a canary-framed buffer with a padded pitch
  mh_decode_rebin    the same ranges for r = 1, 7, 50, 4096, saturating and exact; r = 1 exact is the range decode
  mh_compact         the compacted GPU stream is the oracle's segments back to back and passes mh_validate_stream
"""
import numpy as np
import pytest
import torch

import oracle
from tests import mixed_chunks as mc
from tests import standins
from tests.test_gpu_kernel_cells import _pack_host
from tests.test_gpu_stream_decode import _dense, _encoded, _expected_pieces, _layout

pytestmark = pytest.mark.gpu

OC = oracle.c
CH = mc.CHUNK
FILL = 0xAB
CANARY_WORD = 0x5A5AA5A5
GUARD = 64          # words: keeps the payload 256-byte aligned inside its canary frame
RS = (1, 7, 50, 4096)
IDS = [s.name for s in mc.SCENARIOS]


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, container_io  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    return muahuff


def _framed_encoded(plan):
    """alloc_encoded() with the payload inside a canary frame of exactly payload_cap_words words"""
    cap = plan.payload_cap_words
    frame = torch.full((cap + 2 * GUARD,), CANARY_WORD, dtype=torch.int32, device="cuda")
    e = plan.alloc_encoded()
    e.payload = frame[GUARD:GUARD + cap]
    assert e.payload.data_ptr() % 256 == 0
    return e, frame


def _check_stream(plan, e, frame, oe, tag):
    """segment sizes, bit totals, every used payload word, the frame"""
    nseg = plan.n_segments
    seg = plan.segments()
    assert np.array_equal(seg["off"], oe["seg"]["off"]) and plan.payload_cap_words == oe["payload"].size, tag
    sw = e.seg_words.cpu().numpy().astype(np.uint64)[:nseg]
    host = frame.cpu().numpy().view(np.uint32)
    pay = host[GUARD:GUARD + plan.payload_cap_words]
    bad = np.flatnonzero(sw != oe["seg_words"])
    assert bad.size == 0, tag + ("seg_words", int(bad[0]), int(sw[bad[0]]), int(oe["seg_words"][bad[0]]))
    assert np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), oe["ch_bits"]), tag
    for s in range(nseg):
        o, n = int(seg["off"][s]), int(sw[s])
        diff = np.flatnonzero(pay[o:o + n] != oe["payload"][o:o + n])
        assert diff.size == 0, tag + ("segment", s, "word", int(diff[0]), "of", n)
    assert (host[:GUARD] == CANARY_WORD).all() and (host[GUARD + plan.payload_cap_words:] == CANARY_WORD).all(), tag


def _piece_layout(lens, blocked):
    """where the 4-bit pieces of a packed ENCODE plan lie (as tests/test_gpu_kernel_cells.py lays them out)"""
    bits, pb = 4, 8
    cb = 1024 * pb
    C = len(lens)
    if blocked:
        nch = [(T + CH - 1) // CH for T in lens]
        return np.arange(C, dtype=np.uint64) * np.uint64(cb), C * cb, max(nch) * C * cb + 64
    sz = [((T + 15) // 16 * pb + 15) // 16 * 16 for T in lens]
    return np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64), 0, int(sum(sz)) + 64


@pytest.mark.parametrize("name", IDS)
def test_encode_decode_compact_vs_oracle(mh, name):
    ref = mc.reference(name)
    scn, oe = ref.scn, ref.enc
    tag = (name,)
    plan = mh.codec.Plan(ref.off, ref.ln, scn.S, 0, mh.MODE_NOSORT, mh.WIN_FULL, ref.rows, seg_chunks=scn.sc)
    assert plan.n_segments == len(oe["seg_words"])
    d_data = torch.from_numpy(ref.data.copy()).cuda()
    e, frame = _framed_encoded(plan)
    plan.encode(d_data, out=e)
    assert np.array_equal(e.peak.cpu().numpy(), oe["peak"]) and np.array_equal(e.enc.cpu().numpy(), oe["enc"]), tag
    _check_stream(plan, e, frame, oe, tag + ("mh_encode",))
    # decode: the GPU's slotted stream, the oracle's dense stream
    want = np.full(len(ref.data), FILL, np.uint8)
    for c, x in enumerate(ref.chans):
        o = int(ref.off[c])
        assert np.array_equal(ref.dec[o:o + len(x)], np.minimum(x, scn.S - 1)), tag
        want[o:o + len(x)] = ref.dec[o:o + len(x)]
    pay_d, off_d = _dense(oe)
    theirs = _encoded(mh, pay_d, oe["seg_words"], oe["peak"], oe["enc"], off_d)
    for what, enc in (("gpu slots", e), ("oracle dense", theirs)):
        out = torch.full((len(ref.data),), FILL, dtype=torch.uint8, device="cuda")
        plan.decode(enc, out)
        assert plan.decode_ok(), tag + (what,)
        got = out.cpu().numpy()
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, tag + (what, "byte", int(diff[0]))
    # full cycle: compact, validate
    dense, tot = plan.compact(e)
    total = int(tot.item())
    dense_h = dense.payload[:total].cpu().numpy().view(np.uint32).copy()
    assert total == int(oe["seg_words"].sum()), tag
    assert np.array_equal(dense_h, pay_d[:total]), tag
    lib = mh._lib.lib()
    ln = np.ascontiguousarray(ref.ln, np.uint64)
    sw = np.ascontiguousarray(oe["seg_words"], np.uint64)
    rc = lib.mh_validate_stream(ln.ctypes.data, len(ln), scn.S, 0, mh.MODE_NOSORT, mh.WIN_FULL, ref.rows.ctypes.data, 1,
                                scn.sc, dense_h.ctypes.data, total, sw.ctypes.data, sw.size, oe["peak"].ctypes.data,
                                oe["enc"].ctypes.data)
    assert rc == 0, tag + (lib.mh_last_error(),)
    plan.close()


@pytest.mark.parametrize("name", IDS)
def test_preset_encode_and_packed_decode_of_4bit_pieces_vs_oracle(mh, name):
    ref = mc.reference(name)
    scn = ref.scn
    lens = [int(n) for n in ref.ln]
    C = len(lens)
    pk = np.zeros(C, np.uint8)
    oe = OC.encode_preset(ref.data, ref.off, ref.ln, ref.params, pk, pk)
    pay_d, off_d = _dense(oe)
    for blocked in (False, True):
        tag = (name, "blocked" if blocked else "contiguous")
        # encode from pieces packed on the host
        poff, stride, size = _piece_layout(lens, blocked)
        src = torch.from_numpy(_pack_host(ref.chans, 4, poff, stride, size)).cuda()
        eplan = mh.codec.Plan(poff, ref.ln, scn.S, 0, mh.MODE_NOSORT, mh.WIN_FULL, ref.rows, seg_chunks=scn.sc,
                              input_bits=4, chunk_stride=stride)
        e, frame = _framed_encoded(eplan)
        eplan.encode(src, out=e, preset=(torch.from_numpy(pk).cuda(), torch.from_numpy(pk).cuda()))
        _check_stream(eplan, e, frame, oe, tag + ("mh_encode_preset",))
        eplan.close()
        # decode into pieces, canary bytes between the channels
        off, stride, size = _layout(lens, 4, blocked)
        dplan = mh.codec.Plan(off, ref.ln, scn.S, 0, mh.MODE_NOSORT, mh.WIN_FULL, ref.rows, seg_chunks=scn.sc,
                              input_bits=4, chunk_stride=stride)
        want, _mask = _expected_pieces(ref.chans, scn.S, 4, off, stride, size)
        theirs = _encoded(mh, pay_d, oe["seg_words"], oe["peak"], oe["enc"], off_d)
        for form, enc in (("gpu slots", e), ("oracle dense", theirs)):
            out = torch.full((size,), 0xAB, dtype=torch.uint8, device="cuda")     # CANARY of _expected_pieces
            dplan.decode_packed(enc, out)
            assert dplan.decode_ok(), tag + (form,)
            got = out.cpu().numpy()
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, tag + (form, "byte", int(diff[0]))
        dplan.close()


def _container(mh, ref):
    """the oracle's stream as a dense container (as _container of tests/test_gpu_decode_rebin.py)"""
    cio = mh.container_io
    scn, e = ref.scn, ref.enc
    dense = standins.dense_words(e["payload"], e["seg"]["off"], e["seg_words"])
    hdr = cio.make_header(scn.S, 0, mh.MODE_NOSORT, mh.WIN_FULL, scn.sc, ref.rows)
    hdr["format_revision"] = 3
    C = len(ref.ln)
    return cio.Compressed(hdr, np.array(ref.ln, np.uint64), e["peak"].astype(np.uint8), e["enc"].astype(np.uint8),
                          np.zeros(C, np.uint8), np.zeros(C, np.uint64), e["seg_words"].astype(np.uint64), dense)


def _plan_and_stream(mh, ref):
    scn, oe = ref.scn, ref.enc
    plan = mh.codec.Plan(np.zeros(len(ref.ln), np.uint64), ref.ln, scn.S, 0, mh.MODE_NOSORT, mh.WIN_FULL, ref.rows,
                         seg_chunks=scn.sc)
    pay_d, off_d = _dense(oe)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return plan, t(pay_d.view(np.int32)), t(off_d), t(oe["peak"].copy()), t(oe["enc"].copy())


def _rows(ref, sel, a, b):
    """the oracle's decode of channels sel, sliced and zero-extended to [a, b)"""
    y = np.zeros((len(sel), b - a), np.uint8)
    for i, c in enumerate(sel):
        x = ref.full[c][a:b]
        y[i, :len(x)] = x
    return y


@pytest.mark.parametrize("name", IDS)
def test_range_decode_around_every_oversize_chunk_vs_oracle(mh, name):
    ref = mc.reference(name)
    cio = mh.container_io
    cont = _container(mh, ref)
    C, T = len(ref.ln), int(max(ref.ln))
    got = cio.decompress_range(cont, 0, T).cpu().numpy()
    assert np.array_equal(got, _rows(ref, range(C), 0, T)), (name, "whole range")
    plan, pay, seg_off, peak, enc = _plan_and_stream(mh, ref)
    for k, (c, a, b) in enumerate(mc.query_ranges(ref.scn)):
        tag = (name, c, a, b)
        want = _rows(ref, [c], a, b)
        got = cio.decompress_range(cont, a, b, channels=[c]).cpu().numpy()
        diff = np.flatnonzero(got != want)
        assert got.shape == want.shape and diff.size == 0, tag + ("sample", a + int(diff[0]) if diff.size else -1)
        # the same range of this channel, a neighbour and this channel again into a canary frame with a padded pitch
        sel = [c, (c + 1) % C, c]
        lead = (0, 7, 13)[k % 3]
        buf = torch.full((len(sel) + 2, lead + (b - a) + 45), FILL, dtype=torch.uint8, device="cuda")
        view = buf[1:-1, lead:lead + (b - a)]
        out = plan.decode_range(pay, seg_off, peak, enc, sel, a, b, out=view)
        assert plan.decode_ok() and out.data_ptr() == view.data_ptr(), tag
        host = buf.cpu().numpy()
        assert (host[0] == FILL).all() and (host[-1] == FILL).all(), tag
        assert (host[1:-1, :lead] == FILL).all() and (host[1:-1, lead + b - a:] == FILL).all(), tag
        assert np.array_equal(host[1:-1, lead:lead + b - a], _rows(ref, sel, a, b)), tag
    plan.close()


@pytest.mark.parametrize("name", IDS)
def test_decode_rebin_around_every_oversize_chunk_vs_oracle(mh, name):
    ref = mc.reference(name)
    plan, pay, seg_off, peak, enc = _plan_and_stream(mh, ref)
    for c, a0, b in mc.query_ranges(ref.scn):
        for r in RS:
            a = a0 - a0 % r
            y = _rows(ref, [c], a, b)[0]
            for saturate in (True, False):
                tag = (name, c, a, b, r, saturate)
                want = OC.rebin_u8(y, r) if saturate else OC.rebin_u32(y, r)
                g = plan.decode_rebin(pay, seg_off, peak, enc, [c], a, b, r, saturate).cpu().numpy()
                g = g if saturate else g.view(np.uint32)
                diff = np.flatnonzero(g[0] != want)
                assert g.shape == (1, want.size) and diff.size == 0, tag + ("bin", int(diff[0]) if diff.size else -1)
            if r == 1:       # bins of one sample, exact sums: the range decode itself
                rng_rows = plan.decode_range(pay, seg_off, peak, enc, [c], a, b).cpu().numpy()
                assert np.array_equal(g.astype(np.uint8), rng_rows) and int(g.max()) < 256, tag
    assert plan.decode_ok(), name
    plan.close()
