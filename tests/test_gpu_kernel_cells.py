"""Every production encoder and byte-output decoder instance (tests/kernel_cells.py; the packed-output decoders run in
tests/test_gpu_stream_decode.py) against the CPU oracle, with the data that sends a kernel down its rare paths.

Each encoder cell runs four patterns over the layouts of its task form (seg_chunks 1..4, lengths below 16, off
multiples of 16, whole chunks and one past), NOSORT and APPROX in turn:

  matched  Poisson counts, coded with the word calibrated on the same data
  drift    a word calibrated on quiet data, then data that sits on the symbol of the LONGEST code: at L = 4 every
           sub-stream fills the encoder's 32-dword staging exactly, at L >= 5 every chunk takes the global slow path.
           On the first layout half the channels carry the out-of-range word (255, 255), which must code and
           decode as (0, 0) -- in the in-wave table build (wave form) and in k_lut_preset (workgroup form)
  lanes    alternate 16-sample pieces of the longest and the shortest code: the widest chunk headers
  clip     counts far above 15 (and 3): clipped by the encoder, for packed input first by the intermediate
  mixed    not here: every pattern above keeps a channel's chunks on one route (all staged or all slow); segments
           that switch between the routes are tests/test_gpu_mixed_chunks.py (scenarios: tests/mixed_chunks.py)

Packed cells read pieces built on the host (the documented bit layout, _bitpack) or by mh_deinterleave_packed
(equal-length layouts), contiguous and chunk-blocked.  Every run checks the segment sizes, every used payload word
and the channel bit totals against the oracle (encode or encode_preset); that a byte-layout plan decodes both the
GPU's stream and the oracle's to exactly the oracle's decode, leaving the bytes between windows untouched; and that
the compacted stream passes mh_validate_stream."""
import ctypes as ct
import zlib

import numpy as np
import pytest
import torch

import oracle
from tests import kernel_cells as kc
from tests.test_gpu_parity import _bitpack

pytestmark = pytest.mark.gpu

OC = oracle.c
H = 6            # calibration window 2^6 samples
FILL = 0xAB      # decode output outside the windows must keep this
PATTERNS = ("matched", "drift", "lanes", "clip")


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, container, stream  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    info = muahuff.device_info(0)
    assert "gfx950" in info["arch"], info
    return muahuff


def _ident(c):
    return c.key.replace("mh::", "").replace(" ", "")


def _order(S, mode, peak):
    """idx[rank] = symbol"""
    return OC.approx_sort_rule(S, int(peak)) if mode == OC.MODE_APPROX else np.arange(S)


def _quiet_word(rng, S, mode, rows, C):
    """the (peak, enc) word calibrated on 64 quiet samples per channel"""
    data, off, ln = OC.flatten([np.minimum(rng.poisson(0.05, size=64), 255).astype(np.uint8) for _ in range(C)])
    m = OC.measure(data, off, ln, OC.Params(S, H, mode, OC.WIN_FULL, rows))
    return m["peak"].copy(), m["enc"].copy()


def _make(pattern, rng, S, mode, rows, lens):
    """-> (channels, word): word None = calibrate on the data itself"""
    C = len(lens)
    if pattern in ("matched", "clip"):
        chans = []
        for T in lens:
            x = rng.poisson(float(np.exp(rng.uniform(np.log(0.05), np.log(6.0)))), size=T)
            if pattern == "clip":
                u = rng.random_sample(T)
                x = np.where(u < 0.4, rng.randint(0, 256, size=T), np.where(u < 0.7, rng.randint(16, 41, size=T), x))
            chans.append(np.minimum(x, 255).astype(np.uint8))
        return chans, None
    peak, enc = _quiet_word(rng, S, mode, rows, C)
    chans = []
    for c, T in enumerate(lens):
        idx = _order(S, mode, peak[c])
        top, short = int(idx[S - 1]), int(idx[0])
        if top == S - 1:  # the clipped symbol: any count at or above it
            topv = rng.choice(np.array([S - 1, 15, 16, 200, 255], np.uint8), size=T)
        else:
            topv = np.full(T, top, np.uint8)
        if pattern == "drift":
            x = topv.copy()
            k = min(T, 300)                       # a short prefix of ordinary counts; the rest is the top rank
            x[:k] = rng.randint(0, 20, size=k)
        else:                                     # lanes: odd pieces longest code, even ones shortest
            x = np.where((np.arange(T) >> 4) & 1, topv, short).astype(np.uint8)
        chans.append(x)
    return chans, (peak, enc)


def _pack_host(chans, bits, off, stride, size):
    lim, pb = (1 << bits) - 1, 2 * bits
    buf = np.zeros(size, np.uint8)
    for c, x in enumerate(chans):
        npiece = (len(x) + 15) // 16
        s = np.zeros(npiece * 16, np.uint32)
        s[:len(x)] = np.minimum(x, lim)
        by = _bitpack(s.reshape(npiece, 16), bits)      # [npiece, pb]
        for j in range(0, npiece, 1024):
            at = int(off[c]) + (j // 1024) * stride if stride else int(off[c]) + j * pb
            n = min(1024, npiece - j)
            buf[at:at + n * pb] = by[j:j + n].reshape(-1)
    return buf


def _pack_device(mh, chans, bits, off, stride, size):
    x = torch.from_numpy(np.ascontiguousarray(np.stack(chans, axis=1))).cuda()   # [T, C] time-major
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    mh._lib.check(mh._lib.lib().mh_deinterleave_packed(ct.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], bits,
                                                       ct.c_void_p(out.data_ptr()), ct.c_void_p(d_off.data_ptr()),
                                                       stride, None))
    return out


def _run(mh, cell, case, lens, sc, mode, pattern, rng, word255=False, blocked=False):
    S, rows = case.S, np.array(case.rows, np.uint8)
    K, C = rows.shape[0], len(lens)
    tag = (cell.symbol, S, case.maxlen, lens, sc, mode, pattern, word255, blocked)
    chans, word = _make(pattern, rng, S, mode, rows, lens)
    data, off, ln = OC.flatten(chans)
    p = OC.Params(S, H, mode, OC.WIN_FULL, rows, seg_chunks=sc)
    if word is None and cell.input_bits != 8:  # packed plans only take a preset word: calibrate it on the oracle
        m = OC.measure(data, off, ln, p)
        word = (m["peak"].copy(), m["enc"].copy())
    if word is not None and word255:
        word = (word[0].copy(), word[1].copy())
        word[0][::2] = 255
        word[1][::2] = 255
    dplan = mh.codec.Plan(off, ln, S, H, mode, mh.WIN_FULL, rows, seg_chunks=sc)     # byte layout: decodes
    d_data = torch.from_numpy(data).cuda()
    if word is None:
        e = dplan.encode(d_data)
        oe = OC.encode(data, off, ln, p)
        assert np.array_equal(e.peak.cpu().numpy(), oe["peak"]) and np.array_equal(e.enc.cpu().numpy(), oe["enc"]), tag
        eplan = dplan
    else:
        pk, en = word
        # the (0, 0) stream: out-of-range entries replaced by hand, not by the oracle's own rule
        pk0 = np.where(pk < S, pk, 0).astype(np.uint8)
        en0 = np.where(en < K, en, 0).astype(np.uint8)
        oe = OC.encode_preset(data, off, ln, p, pk0, en0)
        if cell.input_bits == 8:
            eplan, src = dplan, d_data
        else:
            bits, pb = cell.input_bits, 2 * cell.input_bits
            cb = 1024 * pb
            nch = [(T + kc.CHUNK - 1) // kc.CHUNK for T in lens]
            if blocked:
                poff, stride = np.arange(C, dtype=np.uint64) * np.uint64(cb), C * cb
                size = max(nch) * stride + 64
            else:
                sz = [((T + 15) // 16 * pb + 15) // 16 * 16 for T in lens]
                poff, stride = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64), 0
                size = int(sum(sz)) + 64
            if len(set(lens)) == 1:      # end to end: the device de-interleaver writes the pieces
                src = _pack_device(mh, chans, bits, poff, stride, size)
            else:
                src = torch.from_numpy(_pack_host(chans, bits, poff, stride, size)).cuda()
            eplan = mh.codec.Plan(poff, ln, S, H, mode, mh.WIN_FULL, rows, seg_chunks=sc, input_bits=bits,
                                  chunk_stride=stride)
        e = eplan.encode(src, preset=(torch.from_numpy(pk).cuda(), torch.from_numpy(en).cuda()))
    nseg = dplan.n_segments
    seg = dplan.segments()
    assert eplan.n_segments == nseg and np.array_equal(seg["off"], oe["seg"]["off"]), tag
    assert dplan.payload_cap_words == oe["payload"].size, tag
    sw = e.seg_words.cpu().numpy().astype(np.uint64)[:nseg]
    assert np.array_equal(sw, oe["seg_words"]), tag
    assert np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), oe["ch_bits"]), tag
    pay = e.payload.cpu().numpy().view(np.uint32)
    for s in range(nseg):
        o, n = int(seg["off"][s]), int(sw[s])
        assert np.array_equal(pay[o:o + n], oe["payload"][o:o + n]), tag + ("segment", s)
    # decode: the GPU's stream and the oracle's, with the word as given (out-of-range entries decode as 0)
    od = OC.decode(oe["payload"], off, ln, p, oe["peak"], oe["enc"], len(data))
    want = np.full(len(data), FILL, np.uint8)
    for c, x in enumerate(chans):
        o = int(off[c])
        assert np.array_equal(od[o:o + len(x)], np.minimum(x, S - 1)), tag
        want[o:o + len(x)] = od[o:o + len(x)]
    from muahuff.codec import Encoded
    theirs = Encoded(torch.from_numpy(oe["payload"].view(np.int32)).cuda(), e.seg_words, e.ch_bits, e.peak, e.enc,
                     e.skipped)
    for what, enc in (("gpu stream", e), ("oracle stream", theirs)):
        out = torch.full((len(data),), FILL, dtype=torch.uint8, device="cuda")
        dplan.decode(enc, out)
        assert np.array_equal(out.cpu().numpy(), want), tag + (what,)
    assert dplan.decode_ok(), tag
    # the compacted stream is the oracle's segments back to back, and passes the structural check
    dense, tot = eplan.compact(e)
    total = int(tot.item())
    dense_h = dense.payload[:total].cpu().numpy().view(np.uint32).copy()
    assert total == int(oe["seg_words"].sum()), tag
    assert np.array_equal(dense_h, np.concatenate([oe["payload"][int(o):int(o) + int(n)]
                                                   for o, n in zip(seg["off"], oe["seg_words"])])), tag
    lib = mh._lib.lib()
    rc = lib.mh_validate_stream(ln.ctypes.data, C, S, H, mode, mh.WIN_FULL, rows.ctypes.data, K, sc,
                                dense_h.ctypes.data, total, oe["seg_words"].ctypes.data, nseg,
                                oe["peak"].ctypes.data, oe["enc"].ctypes.data)
    assert rc == 0, tag + (lib.mh_last_error(),)
    for pl in {id(dplan): dplan, id(eplan): eplan}.values():
        pl.close()


def _layouts(cell, pattern):
    """(case, lens, seg_chunks, mode, word255, blocked) per layout: the cases in turn, NOSORT / APPROX alternating"""
    k = PATTERNS.index(pattern)
    for i, (lens, sc) in enumerate(cell.layouts):
        yield (cell.cases[i % len(cell.cases)], lens, sc, (i + k) % 2, pattern == "drift" and i == 0, i % 2 == 1)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cell", kc.ENCODER_CELLS, ids=_ident)
def test_encoder_cell_vs_oracle(mh, cell, pattern):
    rng = np.random.RandomState(zlib.crc32((cell.key + pattern).encode()))
    for case, lens, sc, mode, w255, blocked in _layouts(cell, pattern):
        _run(mh, cell, case, lens, sc, mode, pattern, rng, word255=w255, blocked=blocked)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cell", kc.DECODER_CELLS, ids=_ident)
def test_decoder_cell_vs_oracle(mh, cell, pattern):
    """Every case of the cell (both sides of the W caps), the oracle's stream and the GPU's decoded by the cell."""
    rng = np.random.RandomState(zlib.crc32((pattern + cell.key).encode()))
    for j, case in enumerate(cell.cases):
        lens, sc = cell.layouts[(j + PATTERNS.index(pattern)) % len(cell.layouts)]
        _run(mh, cell, case, lens, sc, j % 2, pattern, rng, word255=pattern == "drift" and j == 0)


@pytest.mark.parametrize("S", [3, 6, 10])
def test_stream_encoder_drift_vs_oracle(mh, S):
    """The calibrate-then-stream path end to end (StreamEncoder: de-interleave into the packed chunk-blocked
    intermediate, preset encode, compaction): a channel set calibrated quiet that bursts into its top symbol.
    The dense payload, segment sizes and bit totals equal the oracle's encode_preset under the stored word."""
    from muahuff import stream
    rng = np.random.RandomState(40 + S)
    tab = np.array(kc.R[{3: (3, 2), 6: (6, 5), 10: (10, 9)}[S]], np.uint8)
    C = 9
    se = stream.StreamEncoder(C, S, H, tab)
    peak, enc = se.calibrate(np.minimum(rng.poisson(0.05, size=(64, C)), 255).astype(np.uint8))
    peak, enc = peak.cpu().numpy(), enc.cpu().numpy()
    for T in (2 * kc.CHUNK + 5, 8 * kc.CHUNK, 7):         # wave tasks, workgroup tasks, one short piece
        x = np.full((T, C), 255, np.uint8)
        x[:200] = rng.randint(0, 20, size=(min(T, 200), C))
        c = se.encode_block(x)
        data, off, ln = OC.flatten([x[:, i].copy() for i in range(C)])
        oe = OC.encode_preset(data, off, ln, OC.Params(S, H, 1, OC.WIN_FULL, tab, seg_chunks=se.seg_chunks), peak, enc)
        assert np.array_equal(c.seg_words, oe["seg_words"]), T
        assert np.array_equal(c.ch_bits, oe["ch_bits"]), T
        want = np.concatenate([oe["payload"][int(o):int(o) + int(n)] for o, n in zip(oe["seg"]["off"], oe["seg_words"])])
        assert np.array_equal(c.payload, want), T
        assert np.array_equal(stream.StreamEncoder.decode_block(c), np.minimum(x, S - 1)), T
    se.close()
