"""Random access in time on the GPU (mh_decode_range, codec.Plan.decode_range, container_io.decompress_range,
api.decompress with start / stop): every row of a range query equals the CPU oracle's decode of the whole channel,
sliced and zero-extended, for every window rule, both format revisions, every decoder rung and ranges cut on every
kind of boundary; nothing outside the rows is written; corrupt input is flagged or rejected; full size matches
mh_decode byte for byte."""
import numpy as np
import pytest

import muahuff
from muahuff import container_io as cio
from tests.test_host_range_decode import _oracle_container

pytestmark = pytest.mark.gpu
CH = muahuff.CHUNK


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    return torch


def _dense_decode(chans, c):
    """oracle decode of a container's dense payload: the oracle decoder takes slot offsets, so rebuild them densely"""
    import oracle
    OC = oracle.c
    hd = c.header
    data, off, ln = OC.flatten(chans)
    wflag = hd["window"] | (OC.WIN_REV2_SEGMENTS if hd["format_revision"] == 2 else 0)
    p = OC.Params(hd["S"], hd["h"], hd["mode"], wflag, np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])
    seg = OC.plan_segments(np.array(ln, np.uint64), p)
    slots = np.zeros(int(seg["cap_words"]) + 4, np.uint32)
    pos = 0
    for s, n in enumerate(c.seg_words):
        slots[int(seg["off"][s]):int(seg["off"][s]) + int(n)] = c.payload[pos:pos + int(n)]
        pos += int(n)
    full = OC.decode(slots, off, ln, p, c.peak, c.enc, len(data))
    return [full[int(o):int(o) + int(n)] for o, n in zip(off, ln)]


def _rows(full, sel, start, stop):
    rows = np.zeros((len(sel), stop - start), np.uint8)
    for i, ch in enumerate(sel):
        x = full[ch][start:stop]
        rows[i, :len(x)] = x
    return rows


def _ranges(lens, h, window, sc, rng):
    w0, w1 = cio.window_bounds(lens, h, window)
    T = max(lens)
    r = [(0, 0), (7, 7), (0, 1), (T - 1, T), (0, T), (3, 13), (5, 37), (1000, 3100), (CH - 5, CH + 21),
         (2 * CH - 1, 2 * CH + 1), (sc * CH - 100, sc * CH + 100), (1, 2 * sc * CH + 777)]
    for c in range(len(lens)):
        a = int(w0[c])
        r += [(max(a - 3, 0), min(a + 50, T)), (a + 1024 - 2, min(a + 1024 + 3, T)), (max(int(w1[c]) - 9, 0), T),
              (min(lens[c] - 5, T), T)]
    for _ in range(6):
        a, b = sorted(int(x) for x in rng.randint(0, T + 1, size=2))
        r.append((a, b))
    return [(a, b) for a, b in r if 0 <= a <= b <= T]


LENS = [16 * CH + 1000, 50000, 20 * CH + 3, 5, 70001, 16385, 3 * CH + 77, 300000]
CASES = [(S, h, window, rev) for S in (2, 3, 4, 5, 7, 10) for window in (0, 1, 2, 3) for rev in (2, 3)
         for h in ((2, 3, 6)[(S + window + rev) % 3],)]


@pytest.mark.parametrize("S,h,window,rev", CASES)
def test_range_rows_equal_the_oracle(gpu, S, h, window, rev):
    sc = 1 + (S + window) % 3
    c, chans = _oracle_container(LENS, S, h, window, sc, rev, seed=S * 7 + window)
    full = _dense_decode(chans, c)
    rng = np.random.RandomState(S + 10 * window + rev)
    C = len(LENS)
    sels = [None, [2, 0, 7], list(range(C))[::-1], [4, 4, 1, 4]]
    for k, (a, b) in enumerate(_ranges(LENS, h, window, sc, rng)):
        sel = sels[k % len(sels)]
        got = cio.decompress_range(c, a, b, channels=sel).cpu().numpy()
        want = _rows(full, list(range(C)) if sel is None else sel, a, b)
        assert got.shape == want.shape and np.array_equal(got, want), (S, h, window, rev, a, b, sel)


def test_every_range_decoder_rung_is_exercised():
    """S = 2, 3 (maxlen <= 2), 4 (3), 5 (4: W >= 2L) and 7, 10 (long codes: hybrid) cover the four instances"""
    from tests import helpers
    L = {S: int(helpers.sclv_tables()[S].max()) for S, *_ in CASES}
    assert {1, 2} & set(L.values()) and 3 in L.values() and 4 in L.values() and max(L.values()) >= 6


def test_canary_outside_the_rows_and_padded_pitch(gpu):
    torch = gpu
    from muahuff import codec
    c, chans = _oracle_container(LENS, 3, 6, 2, 2, 3, seed=1)
    full = _dense_decode(chans, c)
    hd = c.header
    plan = codec.Plan(np.zeros(len(LENS), np.uint64), c.ch_len, 3, hd["h"], hd["mode"], cio.plan_window(hd),
                      np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])
    pay = torch.zeros(c.payload.size + 4, dtype=torch.int32, device="cuda")
    pay[:c.payload.size] = torch.from_numpy(c.payload.view(np.int32)).cuda()
    dense_off = np.concatenate([[0], np.cumsum(c.seg_words)[:-1]]).astype(np.int64)
    seg_off = torch.from_numpy(dense_off).cuda()
    peak, enc = torch.from_numpy(c.peak.copy()).cuda(), torch.from_numpy(c.enc.copy()).cuda()
    for (a, b, lead) in ((CH + 3, 3 * CH + 5, 7), (0, max(LENS), 0), (64, 64 + 16, 13), (300, 299 + 2 * CH, 1)):
        sel = [6, 0, 2, 2, 7]
        n = b - a
        pitch = n + lead + 45
        buf = torch.full((len(sel), pitch), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[:, lead:lead + n]
        out = plan.decode_range(pay, seg_off, peak, enc, sel, a, b, out=view)
        assert plan.decode_ok() and out.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        assert (host[:, :lead] == 0xA5).all() and (host[:, lead + n:] == 0xA5).all(), (a, b)
        assert np.array_equal(host[:, lead:lead + n], _rows(full, sel, a, b)), (a, b)
    # argument errors of the binding and of the C call
    with pytest.raises(ValueError):
        plan.decode_range(pay, seg_off, peak, enc, [0], 5, 4)
    with pytest.raises(IndexError):
        plan.decode_range(pay, seg_off, peak, enc, [len(LENS)], 0, 4)
    plan.close()


def test_packed_plan_is_refused(gpu):
    torch = gpu
    from muahuff import MODE_APPROX, WIN_FULL, codec, sclv
    lens = np.array([3 * CH, 2 * CH], np.uint64)
    plan = codec.Plan(np.array([0, 3 * CH // 4], np.uint64), lens, 3, 0, MODE_APPROX, WIN_FULL, sclv.table(3),
                      input_bits=2)
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    o = torch.zeros(8, dtype=torch.int64, device="cuda")
    b = torch.zeros(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(muahuff.MuaHuffError) as e:
        plan.decode_range(z, o, b, b, [0], 0, 4)
    assert e.value.code == muahuff._lib.ERR_ARG
    plan.close()


def test_files_revision_3_revision_2_and_stream_blocks(gpu, tmp_path):
    torch = gpu
    from muahuff import container, stream
    from tests import helpers
    rng = np.random.RandomState(9)
    chans = [np.minimum(rng.poisson(1.1, size=T), 255).astype(np.uint8) for T in (16 * CH + 1000, 50000, 20 * CH + 3)]
    cs = container.ChannelSet.from_channels(chans)
    tab = helpers.sclv_tables()[3]
    new = cio.compress(cs, 3, 6, 1, tab)
    # revision 2, built the way test_revision_2_containers_are_still_read builds one
    plan = muahuff.codec.Plan(cs.ch_off, cs.ch_len, 3, 6, 1, muahuff.WIN_AFTER_CAL | muahuff.WIN_REV2_SEGMENTS, tab,
                              seg_chunks=new.header["seg_chunks"])
    e = plan.encode(cs.data)
    d, tot = plan.compact(e)
    total = int(tot.item())
    hdr = dict(new.header)
    hdr["format_revision"] = 2
    old = cio.Compressed(hdr, cs.ch_len.copy(), e.peak.cpu().numpy(), e.enc.cpu().numpy(), e.skipped.cpu().numpy(),
                         e.ch_bits.cpu().numpy().astype(np.uint64), e.seg_words.cpu().numpy().astype(np.uint64)[:plan.n_segments],
                         d.payload[:total].cpu().numpy().view(np.uint32).copy())
    plan.close()
    # a stream block: preset WIN_FULL, h = 0
    T, C = 3 * CH + 500, 6
    blk = np.minimum(rng.poisson(0.9, size=(T, C)), 255).astype(np.uint8)
    enc_ = stream.StreamEncoder(C, 3, 6, tab)
    enc_.calibrate(torch.from_numpy(blk[:64].copy()).cuda())
    conts = [("rev3", new), ("rev2", old), ("block", enc_.encode_block(torch.from_numpy(blk).cuda()))]
    for name, c in conts:
        fn = str(tmp_path / (name + ".muahuff"))
        cio.save(fn, c)
        ref = cio.decompress(c).to_channels()
        lens = [int(x) for x in c.ch_len]
        for (a, b, sel) in ((0, max(lens), None), (CH + 5, CH + 5 + 16384, [2, 0]), (3, 4, [1]), (40000, 60000, [1, 1])):
            b = min(b, max(lens))
            sel_ = list(range(len(lens))) if sel is None else sel
            want = _rows(ref, sel_, a, b)
            with cio.open(fn) as f:
                got = cio.decompress_range(f, a, b, channels=sel).cpu().numpy()
                first, end = cio.range_segments(lens, c.header["h"], c.header["window"], c.header["seg_chunks"], a, b,
                                                c.header["format_revision"])
                words = sum(int(np.sum(c.seg_words[first[ch]:end[ch]])) for ch in set(sel_))
                assert f.bytes_read == f.head_bytes + 4 * words, name
            assert np.array_equal(got, want), (name, a, b, sel)
            tm = cio.decompress_range(c, a, b, channels=sel, time_major=True).cpu().numpy()
            assert np.array_equal(tm, want.T), (name, a, b)
            api = muahuff.decompress(fn, channels=sel, start=a, stop=b)
            assert len(api) == len(sel_) and all(np.array_equal(x, y) for x, y in zip(api, want))


def test_untrusted_input_is_flagged_or_rejected(gpu):
    torch = gpu
    from muahuff import codec
    c, chans = _oracle_container(LENS, 5, 6, 2, 2, 3, seed=3)
    a, b, sel = CH + 100, 5 * CH + 100, [0, 2, 7]
    pay, seg_off, segs = cio.gather_range(c, a, b, np.array(sel))
    # check=True: a garbled header in a segment the query reads raises before anything reaches the GPU
    bad = c.payload.copy()
    dense_off = np.concatenate([[0], np.cumsum(c.seg_words)[:-1]]).astype(np.int64)
    for s in segs:
        bad[int(dense_off[int(s)])] ^= 0xFFF
    cb = cio.Compressed(c.header, c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words, bad)
    with pytest.raises(ValueError):
        cio.decompress_range(cb, a, b, channels=sel)
    # check=False on a truncated payload: status flag, and nothing outside the rows is written
    hd = c.header
    plan = codec.Plan(np.zeros(len(LENS), np.uint64), c.ch_len, hd["S"], hd["h"], hd["mode"], cio.plan_window(hd),
                      np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])
    for payload in (pay[:len(pay) // 3], np.where(np.arange(len(pay)) % 97 == 0, np.uint32(0xFFFFFFFF), pay).astype(np.uint32)):
        d_pay = torch.from_numpy(payload.view(np.int32).copy()).cuda()
        n = b - a
        buf = torch.full((len(sel), n + 64), 0xA5, dtype=torch.uint8, device="cuda")
        plan.decode_range(d_pay, torch.from_numpy(seg_off.view(np.int64)).cuda(), torch.from_numpy(c.peak.copy()).cuda(),
                          torch.from_numpy(c.enc.copy()).cuda(), sel, a, b, out=buf[:, 32:32 + n])
        flagged = not plan.decode_ok()
        host = buf.cpu().numpy()
        assert (host[:, :32] == 0xA5).all() and (host[:, 32 + n:] == 0xA5).all()
        if payload.size < pay.size:
            assert flagged
    plan.close()


def test_full_size_range_equals_decode(gpu):
    """1024 x 1e7 S = 3 (synth): the whole-recording range is mh_decode's output byte for byte, three random ranges are
    device-side slices of it."""
    torch = gpu
    from muahuff import MODE_APPROX, WIN_AFTER_CAL, codec, sclv, synth
    C, T = 1024, 10_000_000
    cs = synth.generate(C, T, seed=3)
    tab = sclv.table(3)
    plan = codec.Plan(cs.ch_off, cs.ch_len, 3, 6, MODE_APPROX, WIN_AFTER_CAL, tab)
    e = plan.encode(cs.data)
    ref = torch.zeros_like(cs.data)
    plan.decode(e, ref)
    seg_off = torch.from_numpy(plan.segments()["off"].astype(np.int64)).cuda()
    del cs
    out = plan.decode_range(e.payload, seg_off, e.peak, e.enc, None, 0, T)
    assert plan.decode_ok()
    off = torch.from_numpy(plan.ch_off.astype(np.int64)).cuda()
    mat = ref.as_strided((C, T), (int(plan.ch_off[1] - plan.ch_off[0]), 1), int(plan.ch_off[0]))
    assert np.all(np.diff(plan.ch_off.astype(np.int64)) == int(plan.ch_off[1] - plan.ch_off[0]))
    assert torch.equal(out, mat)
    del out
    rng = np.random.RandomState(5)
    for n in (1000, 16384, 1_000_000):
        a = int(rng.randint(0, T - n))
        sel = sorted(rng.choice(C, 96, replace=False).tolist())
        got = plan.decode_range(e.payload, seg_off, e.peak, e.enc, sel, a, a + n)
        assert plan.decode_ok()
        assert torch.equal(got, mat[torch.tensor(sel, device="cuda"), a:a + n]), n
    del off
    plan.close()
