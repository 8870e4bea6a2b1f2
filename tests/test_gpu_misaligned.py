"""Every byte-layout codec kernel instance and every histogram kernel on byte-misaligned channels (scenarios:
tests/misaligned.py; placement, address residues and the oracle's own indifference to offsets:
tests/test_host_misaligned.py) against the CPU oracle, bit for bit.

Codec cells run the patterns `matched` and `drift` of tests/test_gpu_kernel_cells.py (drift: the L >= 5 cells take the
encoder's global slow path and the decoder's unstaged path on every chunk, and the word is a preset one) on channels
at odd addresses, touching or 1, 3 and 117 bytes apart, under MH_WIN_AFTER_CAL, _REF_HALF_TRUNC and _REF_HALF with
h = 0..3; the MH_WIN_REF_HALF scenarios hold channels the rule skips, touching coded neighbours.  Checked per run:
segment directory, seg_words, every used payload word, ch_bits, peak, enc, skipped; the GPU's stream and the oracle's
decoded into a buffer full of a marker byte and compared WHOLE -- gaps, guards, the calibration prefix, skipped
channels, the live samples behind a REF_HALF window and the touching neighbour keep the marker; decode_ok; the
compacted stream through mh_validate_stream.

Measure scenarios compare every output of mh_measure, twice in a row on one plan (the one-launch form hands its
scratch back zeroed)."""
import zlib

import numpy as np
import pytest
import torch

import oracle
from tests import misaligned as ma
from tests.test_gpu_kernel_cells import FILL, _ident, _make

pytestmark = pytest.mark.gpu

OC = oracle.c
PATTERNS = ("matched", "drift")


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    info = muahuff.device_info(0)
    assert "gfx950" in info["arch"], info
    return muahuff


def _device(host):
    """the buffer on the device, on a 128-byte boundary: the offsets are the address residues"""
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 128 == 0
    return t


def _run(mh, cell, s, pattern, rng, word255):
    S, rows, sc = s.case.S, np.array(s.case.rows, np.uint8), s.seg_chunks
    K, C = rows.shape[0], len(s.lens)
    tag = (cell.symbol, s, pattern, word255)
    chans, word = _make(pattern, rng, S, s.mode, rows, s.lens)
    data, off, ln = ma.layout(chans, s.shift)
    p = OC.Params(S, s.h, s.mode, s.window, rows, seg_chunks=sc)
    plan = mh.codec.Plan(off, ln, S, s.h, s.mode, s.window, rows, seg_chunks=sc)
    d_data = _device(data)
    skipped = np.array([ma.window(T, s.h, s.window)[2] for T in s.lens], np.uint8)
    if word is None:
        e = plan.encode(d_data)
        oe = OC.encode(data, off, ln, p)
        assert np.array_equal(e.peak.cpu().numpy(), oe["peak"]) and np.array_equal(e.enc.cpu().numpy(), oe["enc"]), tag
        assert np.array_equal(e.skipped.cpu().numpy(), oe["skipped"]), tag
        assert np.array_equal(oe["skipped"], skipped), tag
    else:
        pk, en = word
        if word255:
            pk, en = pk.copy(), en.copy()
            pk[::2] = 255
            en[::2] = 255
        # the (0, 0) stream: out-of-range entries replaced by hand, not by the oracle's own rule
        oe = OC.encode_preset(data, off, ln, p, np.where(pk < S, pk, 0).astype(np.uint8),
                              np.where(en < K, en, 0).astype(np.uint8))
        e = plan.encode(d_data, preset=(torch.from_numpy(pk).cuda(), torch.from_numpy(en).cuda()))
    nseg = plan.n_segments
    seg = plan.segments()
    for k in ("ch", "first", "n", "off"):
        assert np.array_equal(seg[k], oe["seg"][k]), tag + (k,)
    assert plan.payload_cap_words == oe["payload"].size, tag
    sw = e.seg_words.cpu().numpy().astype(np.uint64)[:nseg]
    assert np.array_equal(sw, oe["seg_words"]), tag
    assert np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), oe["ch_bits"]), tag
    # a channel that MH_WIN_REF_HALF skips has no segment and no bits, whichever word codes the rest (mh_encode_preset
    # and the oracle's encode_preset have no `skipped` output of their own: the rule is the plan's)
    assert not np.isin(seg["ch"], np.flatnonzero(skipped)).any(), tag
    assert not e.ch_bits.cpu().numpy()[skipped == 1].any(), tag
    pay = e.payload.cpu().numpy().view(np.uint32)
    for i in range(nseg):
        o, n = int(seg["off"][i]), int(sw[i])
        assert np.array_equal(pay[o:o + n], oe["payload"][o:o + n]), tag + ("segment", i)
    # decode: the oracle's output on the windows, the marker everywhere else
    od = OC.decode(oe["payload"], off, ln, p, oe["peak"], oe["enc"], len(data))
    want = np.full(len(data), FILL, np.uint8)
    for x, o in zip(chans, off):
        w0, w1, _skip = ma.window(len(x), s.h, s.window)
        assert np.array_equal(od[int(o) + w0:int(o) + w1], np.minimum(x[w0:w1], S - 1)), tag
        want[int(o) + w0:int(o) + w1] = od[int(o) + w0:int(o) + w1]
    from muahuff.codec import Encoded
    theirs = Encoded(torch.from_numpy(oe["payload"].view(np.int32)).cuda(), e.seg_words, e.ch_bits, e.peak, e.enc,
                     e.skipped)
    for what, enc in (("gpu stream", e), ("oracle stream", theirs)):
        out = torch.full((len(data),), FILL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 128 == 0
        plan.decode(enc, out)
        got = out.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, "first bytes that differ", bad[:8].tolist(), "channel offsets", off.tolist()) + tag
    assert plan.decode_ok(), tag
    dense, tot = plan.compact(e)
    total = int(tot.item())
    dense_h = dense.payload[:total].cpu().numpy().view(np.uint32).copy()
    assert total == int(oe["seg_words"].sum()), tag
    if nseg:
        assert np.array_equal(dense_h, np.concatenate([oe["payload"][int(o):int(o) + int(n)]
                                                       for o, n in zip(seg["off"], oe["seg_words"])])), tag
    lib = mh._lib.lib()
    rc = lib.mh_validate_stream(ln.ctypes.data, C, S, s.h, s.mode, s.window, rows.ctypes.data, K, sc,
                                dense_h.ctypes.data, total, oe["seg_words"].ctypes.data, nseg,
                                oe["peak"].ctypes.data, oe["enc"].ctypes.data)
    assert rc == 0, tag + (lib.mh_last_error(),)
    plan.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cell", ma.CODEC_CELLS, ids=_ident)
def test_codec_cell_on_misaligned_channels_vs_oracle(mh, cell, pattern):
    rng = np.random.RandomState(zlib.crc32((cell.key + pattern + "misaligned").encode()))
    for i, s in enumerate(ma.codec_scenarios(cell)):
        _run(mh, cell, s, pattern, rng, word255=pattern == "drift" and i == 0)


@pytest.mark.parametrize("m", ma.measure_scenarios(), ids=lambda m: m.ident)
def test_measure_on_misaligned_channels_vs_oracle(mh, m):
    rows = np.array(ma.MEASURE_ROWS[m.S], np.uint8)
    lens, gaps, _kinds = m.lens()
    data, off, ln = ma.layout(ma.measure_channels(m.h, m.window, m.shift), m.shift, gaps)
    om = OC.measure(data, off, ln, OC.Params(m.S, m.h, m.mode, m.window, rows))
    plan = mh.codec.Plan(off, ln, m.S, m.h, m.mode, m.window, rows)
    d_data = _device(data)
    for call in range(2):
        g = plan.measure(d_data)
        for name, got, want in (("cutoff", g.cutoff, om["cutoff"]), ("cal_hist", g.cal_hist, om["cal_sorted"]),
                                ("peak", g.peak, om["peak"]), ("enc", g.enc, om["enc"]),
                                ("post_hist", g.post_hist, om["post_mapped"]), ("bits", g.bits, om["bits"]),
                                ("skipped", g.skipped, om["skipped"])):
            got = got.cpu().numpy()
            bad = np.flatnonzero((got.astype(np.int64) != want.astype(np.int64)).reshape(len(lens), -1).any(axis=1))
            assert bad.size == 0, (m, "call", call, name, "channels", bad.tolist(),
                                   [(int(off[c]), lens[c]) for c in bad[:6]])
    plan.close()
