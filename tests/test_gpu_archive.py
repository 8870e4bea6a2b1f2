"""The recording archive on the GPU (archive.py): append (host and device blocks, pipelined or not, with and without
recalibration) -> one file -> read() of any global range, selection and bin factor.  Expectations are plain NumPy on the
input (min(x, S-1) of the concatenated blocks), the CPU oracle's decode / measure / preset encode of the stored blocks and
the oracle's re-binning."""
import shutil

import numpy as np
import pytest

import muahuff
import oracle
from muahuff import archive
from muahuff import container_io as cio
from tests import helpers

pytestmark = pytest.mark.gpu
OC = oracle.c
CH = muahuff.CHUNK
LENS = (CH + 1, 3 * CH + 7, 40, 2 * CH, 5 * CH + 3)
CASES = ((3, 7), (5, 70), (10, 23))       # (S, channels): 2-bit and 4-bit packing, a long code
RS = (1, 3, 7, 50, 128, 1000, 4096, 16)   # 16 divides the first step of the last three blocks, 3 that of the third
H, SC, NT = 6, 2, 16


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    return torch


def _draw(lens, C, seed, swap=False):
    """time-major Poisson blocks whose rate changes per block and per channel; swap: quiet and busy channels trade
    places from block to block, so that calibration peaks move"""
    rng = np.random.RandomState(seed)
    out = []
    for b, Tb in enumerate(lens):
        if swap:
            lam = np.where((np.arange(C) + b) % 2 == 0, 0.2, 2.6)
        else:
            lam = np.array([(0.15, 0.8, 2.5, 4.0)[(c + b) % 4] for c in range(C)])
        out.append(np.minimum(rng.poisson(lam, size=(Tb, C)), 255).astype(np.uint8))
    return out


def _write(torch, fn, blocks, S, **kw):
    C = blocks[0].shape[1]
    with archive.create(fn, C, S=S, hist_bits=H, sclv_rows=helpers.sclv_tables()[S], seg_chunks=SC, **kw) as w:
        for k, x in enumerate(blocks):
            w.append(torch.from_numpy(x).cuda() if k % 2 else x)      # host arrays and device tensors alike
    return fn


_RECS = {}


@pytest.fixture(scope="module")
def recs(gpu, tmp_path_factory):
    """(S, C) -> (archive path, input blocks, expectation [C, T] = min(x, S-1) of the concatenated input); built once"""
    def get(S, C):
        if (S, C) not in _RECS:
            blocks = _draw(LENS, C, 100 * S + C)
            fn = _write(gpu, str(tmp_path_factory.mktemp("rec") / ("s%d.mua" % S)), blocks, S, meta={"S": S})
            want = np.ascontiguousarray(np.minimum(np.concatenate(blocks), S - 1).T)
            want.setflags(write=False)
            _RECS[(S, C)] = (fn, blocks, want)
        return _RECS[(S, C)]
    return get


def _oracle_decode(c):
    """the CPU oracle's decode of one stored block -> [C, Tb]"""
    hd = c.header
    p = OC.Params(hd["S"], hd["h"], hd["mode"], hd["window"], np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])
    C, Tb = len(c.ch_len), int(c.ch_len[0])
    data, off, ln = OC.flatten([np.zeros(Tb, np.uint8)] * C)
    seg = OC.plan_segments(ln, p)
    slots = np.zeros(seg["cap_words"] + 4, np.uint32)
    d = 0
    for o, n in zip(seg["off"], c.seg_words):
        slots[int(o):int(o) + int(n)] = c.payload[d:d + int(n)]
        d += int(n)
    full = OC.decode(slots, off, ln, p, c.peak, c.enc, len(data), nthreads=NT)
    return np.stack([full[int(o):int(o) + Tb] for o in off])


def _tm(block):
    chans = [np.ascontiguousarray(block[:, c]) for c in range(block.shape[1])]
    return OC.flatten(chans)


def _rebinned(rows, r, saturate):
    nb = (rows.shape[1] + r - 1) // r
    out = np.zeros((rows.shape[0], nb), np.uint8 if saturate else np.uint32)
    for i, y in enumerate(rows):
        if nb:
            out[i] = OC.rebin_u8(y, r) if saturate else OC.rebin_u32(y, r)
    return out


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _edges(lens):
    """block boundaries, chunk and segment boundaries inside the blocks, each with its neighbours"""
    T, pts, t0 = sum(lens), {0, 1}, 0
    for Tb in lens:
        for p in [t0] + [t0 + k * CH for k in range(1, Tb // CH + 1)] + [t0 + k * SC * CH for k in range(1, Tb // (SC * CH) + 1)]:
            pts.update((p - 1, p, p + 1))
        t0 += Tb
    pts.update((T - 1, T))
    return sorted(p for p in pts if 0 <= p <= T)


@pytest.mark.parametrize("S,C", CASES)
def test_round_trip(gpu, recs, S, C):
    fn, blocks, want = recs(S, C)
    with archive.open(fn) as a:
        assert (a.C, a.S, a.T, a.truncated, a.meta) == (C, S, sum(LENS), False, {"S": S})
        assert [b.Tb for b in a.blocks] == list(LENS)
        got = a.read(0, a.T)
        assert got.dtype == gpu.uint8 and tuple(got.shape) == (C, a.T)
        assert np.array_equal(got.cpu().numpy(), want)
        t0 = 0
        for i, Tb in enumerate(LENS):      # every stored block is a stream the CPU oracle decodes to the same samples
            assert np.array_equal(_oracle_decode(a.block(i)), want[:, t0:t0 + Tb]), i
            t0 += Tb


@pytest.mark.parametrize("S,C", CASES)
def test_ranges_and_selections(gpu, recs, S, C):
    fn, _blocks, want = recs(S, C)
    T = want.shape[1]
    rng = np.random.RandomState(S)
    e = _edges(LENS)
    ranges = [(0, 0), (T, T), (5, 5), (0, 1), (T - 1, T), (0, T)]
    ranges += [(p, q) for p, q in zip(e, e[1:])] + [(p, q) for p, q in zip(e, e[3:])][::4]
    ranges += [(e[i], e[-1 - i]) for i in range(0, len(e) // 2, 5)]
    ranges += [tuple(sorted(int(v) for v in rng.randint(0, T + 1, size=2))) for _ in range(8)]
    sels = [None, list(range(C))[::-1], [4, 4, 1, 4, 0], [C - 1, 2], [3]]
    with archive.open(fn) as a:
        for k, (p, q) in enumerate(ranges):
            sel = sels[k % len(sels)]
            rows = want[list(range(C)) if sel is None else sel, p:q]
            tm = k % 3 == 2
            got = a.read(p, q, channels=sel, time_major=tm).cpu().numpy()
            assert got.shape == (rows.T.shape if tm else rows.shape) and np.array_equal(got, rows.T if tm else rows), (p, q, sel, tm)


@pytest.mark.parametrize("S,C", CASES)
def test_binning(gpu, recs, S, C):
    fn, _blocks, want = recs(S, C)
    T = want.shape[1]
    t1, t2 = LENS[0], LENS[0] + LENS[1]
    seen255 = above255 = False
    with archive.open(fn) as a:
        for j, r in enumerate(RS):
            spans = [(0, T), (t1 - t1 % r, t2 + 45), ((t1 + 3000) - (t1 + 3000) % r, T - 1), (t2 - t2 % r, t2 - t2 % r + 1)]
            for k, (p, q) in enumerate(spans):
                sel = [None, [2, 0, 2], list(range(C))[::-1]][(j + k) % 3]
                rows = want[list(range(C)) if sel is None else sel, p:q]
                for saturate in (True, False):
                    exp = _rebinned(rows, r, saturate)
                    got = _host(a.read(p, q, channels=sel, bin=r, saturate=saturate))
                    assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), (r, p, q, saturate)
                    seen255 |= saturate and bool((exp == 255).any())
                    above255 |= (not saturate) and int(exp.max()) > 255
            tm = a.read(0, T, channels=[1, 0], bin=r, time_major=True).cpu().numpy()
            assert np.array_equal(tm, _rebinned(want[[1, 0]], r, True).T)
    assert seen255 and above255


def test_rows_land_inside_a_canary_buffer(gpu, recs):
    torch = gpu
    fn, _blocks, want = recs(5, 70)
    t1, t2 = LENS[0], LENS[0] + LENS[1] + LENS[2]
    sel = [6, 0, 2, 2, 69]
    with archive.open(fn) as a:
        for (p, q, r, saturate) in ((t1 - 100, t2 + 333, None, True), (t1 - 34 - (t1 - 34) % 50, t2 + 5, 50, True), (0, a.T, 16, False),
                                    (t1 - 34 - (t1 - 34) % 3, t2 + 5000, 3, True), (0, t1 + 1, 1, False)):
            cols = q - p if r is None else (q - p + r - 1) // r
            dt = torch.uint8 if saturate else torch.int32
            canary = 0xA5 if saturate else 0x5A5A5A5A
            buf = torch.full((len(sel) + 2, cols + 7 + 45), canary, dtype=dt, device="cuda")
            view = buf[1:-1, 7:7 + cols]
            got = a.read(p, q, channels=sel, bin=r, saturate=saturate, out=view)
            assert got.data_ptr() == view.data_ptr()
            host = buf.cpu().numpy()
            assert (host[0] == canary).all() and (host[-1] == canary).all()
            assert (host[1:-1, :7] == canary).all() and (host[1:-1, 7 + cols:] == canary).all(), (p, q, r)
            exp = want[sel, p:q] if r is None else _rebinned(want[sel, p:q], r, saturate)
            assert np.array_equal(host[1:-1, 7:7 + cols].view(exp.dtype), exp), (p, q, r)


@pytest.mark.parametrize("S,C", CASES)
def test_stored_words_without_recalibration(gpu, recs, S, C):
    fn, blocks, _want = recs(S, C)
    rows = helpers.sclv_tables()[S]
    data, off, ln = _tm(blocks[0])
    m = OC.measure(data, off, ln, OC.Params(S, H, 1, 3, rows), nthreads=NT)
    with archive.open(fn) as a:
        peak, enc = a.words()
        assert peak.shape == (len(LENS), C)
        for i, x in enumerate(blocks):
            assert np.array_equal(peak[i], m["peak"]) and np.array_equal(enc[i], m["enc"]), i
            data, off, ln = _tm(x)
            ref = OC.encode_preset(data, off, ln, OC.Params(S, 0, 1, 3, rows, SC), m["peak"], m["enc"], nthreads=NT)
            c = a.block(i)
            assert np.array_equal(c.ch_bits, ref["ch_bits"]) and np.array_equal(c.seg_words, ref["seg_words"]), i


@pytest.mark.parametrize("S", (3, 5))
@pytest.mark.parametrize("pipeline", (True, False))
def test_stored_words_with_recalibration(gpu, tmp_path, S, pipeline):
    C = 10
    rows = helpers.sclv_tables()[S]
    blocks = _draw(LENS, C, 7 + S, swap=True)
    fn = _write(gpu, str(tmp_path / "r.mua"), blocks, S, recalibrate=1, pipeline=pipeline)
    with archive.open(fn) as a:
        peak, enc = a.words()
        stored = [a.block(i).ch_bits.astype(np.int64) for i in range(len(LENS))]
        got = a.read(0, a.T).cpu().numpy()
    assert np.array_equal(got, np.minimum(np.concatenate(blocks), S - 1).T)      # every block still decodes exactly
    fresh = []
    for x in blocks:
        data, off, ln = _tm(x)
        fresh.append(OC.measure(data, off, ln, OC.Params(S, H, 1, 3, rows), nthreads=NT))
    assert np.array_equal(peak[0], fresh[0]["peak"]) and np.array_equal(enc[0], fresh[0]["enc"])
    for b in range(len(LENS)):
        data, off, ln = _tm(blocks[b])       # each block is coded with the word it stores
        ref = OC.encode_preset(data, off, ln, OC.Params(S, 0, 1, 3, rows, SC), peak[b], enc[b], nthreads=NT)
        assert np.array_equal(stored[b], ref["ch_bits"].astype(np.int64)), b
    for b in range(len(LENS) - 1):
        take = stored[b] - fresh[b]["bits"].astype(np.int64) >= 1
        assert np.array_equal(peak[b + 1], np.where(take, fresh[b]["peak"], peak[b])), b
        assert np.array_equal(enc[b + 1], np.where(take, fresh[b]["enc"], enc[b])), b
    assert (peak[1:] != peak[:-1]).any()     # the input makes peaks move, and the word follows


@pytest.mark.parametrize("S", (3, 5))
def test_pipelined_and_plain_writers_agree_byte_for_byte(gpu, tmp_path, S):
    torch = gpu
    from muahuff.stream import StreamEncoder
    C, Tb = 12, CH + 77
    rows = helpers.sclv_tables()[S]
    blocks = _draw((Tb,) * 8, C, 50 + S)
    files = [_write(torch, str(tmp_path / ("p%d.mua" % p)), blocks, S, pipeline=bool(p)) for p in (1, 0)]
    se = StreamEncoder(C, S, H, rows, seg_chunks=SC)
    se.calibrate(blocks[0])
    third = str(tmp_path / "c.mua")
    with archive.create(third, C, S=S, hist_bits=H, sclv_rows=rows, seg_chunks=SC) as w:
        for x in blocks:
            w.append_compressed(se.encode_block(x))
    se.close()
    raw = [open(f, "rb").read() for f in files + [third]]
    assert raw[0] == raw[1] and raw[0] == raw[2]
    with archive.open(files[0]) as a:
        assert a.T == 8 * Tb and not a.truncated
    # the same holds while the word moves
    swap = _draw((Tb,) * 8, C, 60 + S, swap=True)
    files = [_write(torch, str(tmp_path / ("q%d.mua" % p)), swap, S, pipeline=bool(p), recalibrate=1) for p in (1, 0)]
    assert open(files[0], "rb").read() == open(files[1], "rb").read()


def _three(torch, tmp_path, S=5, C=9):
    lens = (2 * CH + 5, 4 * CH + 7, CH + 1)
    blocks = _draw(lens, C, 31)
    fn = _write(torch, str(tmp_path / "l.mua"), blocks, S)
    return fn, lens, np.ascontiguousarray(np.minimum(np.concatenate(blocks), S - 1).T)


def test_a_short_read_touches_one_block_only(gpu, tmp_path):
    fn, lens, want = _three(gpu, tmp_path)
    ch, a0 = 4, SC * CH - 30      # 100 samples of one channel across a segment boundary of the middle block
    with archive.open(fn) as a:
        b = a.blocks[1]
        c = a.block(1)
        head, trailer = a.header_bytes, a.trailer_bytes
    pay = 4 * c.payload.size
    non_payload = 32 + b.nbytes - (pay + (-pay % 8))
    first, end = cio.range_segments(c.ch_len, 0, 3, SC, a0, a0 + 100)
    assert end[ch] - first[ch] == 2
    words = int(c.seg_words[int(first[ch]):int(end[ch])].sum())
    with archive.open(fn) as a:
        assert a.bytes_read <= head + trailer
        got = a.read(lens[0] + a0, lens[0] + a0 + 100, channels=[ch]).cpu().numpy()
        assert np.array_equal(got, want[[ch], lens[0] + a0:lens[0] + a0 + 100])
        assert a.bytes_read <= head + trailer + non_payload + 4 * words, (a.bytes_read, head, trailer, non_payload, words)
        assert list(a._files) == [1]      # the other blocks were never opened


def test_a_corrupt_segment_is_rejected_or_flagged(gpu, tmp_path):
    torch = gpu
    fn, lens, _want = _three(torch, tmp_path)
    ch, a0 = 4, SC * CH + 500
    with archive.open(fn) as a:
        b = a.blocks[1]
        c = a.block(1)
    first, _end = cio.range_segments(c.ch_len, 0, 3, SC, a0, a0 + 100)
    word = int(np.concatenate([[0], np.cumsum(c.seg_words)])[int(first[ch])])
    pay = 4 * c.payload.size
    at = b.offset + b.nbytes - (pay + (-pay % 8)) + 4 * word
    bad = str(tmp_path / "bad.mua")
    shutil.copy(fn, bad)
    with open(bad, "r+b") as f:
        f.seek(at)
        w = int.from_bytes(f.read(4), "little")
        assert w == int(c.payload[word])
        f.seek(at)
        f.write((w ^ 0xFFF).to_bytes(4, "little"))
    p, q = lens[0] + a0, lens[0] + a0 + 100
    with archive.open(bad) as a:
        buf = torch.full((3, 100 + 64), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError):
            a.read(p, q, channels=[ch], out=buf[1:2, 32:132])
        assert (buf.cpu().numpy() == 0xA5).all()      # rejected on the host: nothing was launched
        assert not a._plans
        with pytest.raises(ValueError):
            a.read(p, q, channels=[ch], check=False, out=buf[1:2, 32:132])
        host = buf.cpu().numpy()
        assert (host[0] == 0xA5).all() and (host[2] == 0xA5).all() and (host[1, :32] == 0xA5).all() and (host[1, 132:] == 0xA5).all()
        # the neighbouring channel and the other blocks are as good as ever
        good = a.read(p, q, channels=[ch + 1]).cpu().numpy()
    with archive.open(fn) as a:
        assert np.array_equal(good, a.read(p, q, channels=[ch + 1]).cpu().numpy())


def test_the_api_answers_from_an_archive(gpu, recs):
    fn, _blocks, want = recs(5, 70)
    T = want.shape[1]
    t1 = LENS[0]
    got = muahuff.decompress(fn, channels=[3, 1])
    assert len(got) == 2 and all(g.dtype == np.uint8 and np.array_equal(g, want[ch]) for g, ch in zip(got, (3, 1)))
    for (p, q, sel) in ((t1 - 16, t1 + 16384, [2, 0]), (40000, 60001, [1, 1]), (0, T, None)):
        sel_ = list(range(70)) if sel is None else sel
        api = muahuff.decompress(fn, channels=sel, start=p, stop=q)
        assert len(api) == len(sel_) and all(np.array_equal(x, y) for x, y in zip(api, want[sel_, p:q])), (p, q)
        for r in (7, 50):
            p_ = p - p % r
            api = muahuff.decompress(fn, channels=sel, start=p_, stop=q, bin=r)
            exp = _rebinned(want[sel_, p_:q], r, True)
            assert len(api) == len(sel_) and all(x.dtype == np.uint8 and np.array_equal(x, y) for x, y in zip(api, exp)), (p, q, r)
    got = muahuff.decompress(fn, channels=[5], bin=1000)
    assert np.array_equal(got[0], OC.rebin_u8(want[5], 1000))


def test_real_channel_count(gpu, tmp_path):
    """1024 channels x 3 blocks x 2 chunks at S = 3: the chunk-blocked packed layout at its real width"""
    torch = gpu
    C, S, Tb = 1024, 3, 2 * CH
    g = torch.Generator(device="cuda").manual_seed(5)
    blocks = [((torch.rand((Tb, C), device="cuda", generator=g) < 0.3).to(torch.uint8) +
               (torch.rand((Tb, C), device="cuda", generator=g) < 0.1 * (k + 1)).to(torch.uint8) * 3) for k in range(3)]
    fn = str(tmp_path / "w.mua")
    with archive.create(fn, C, S=S, hist_bits=H, seg_chunks=SC) as w:
        for x in blocks:
            w.append(x)
    want = torch.cat(blocks).clamp(max=S - 1).t().contiguous()
    with archive.open(fn) as a:
        assert a.T == 3 * Tb
        assert torch.equal(a.read(0, a.T), want)
        got = a.read(Tb - 104, Tb + 100, channels=[1023, 0], bin=8, saturate=False)
        exp = want[[1023, 0], Tb - 104:Tb + 100]
    assert np.array_equal(_host(got), _rebinned(exp.cpu().numpy(), 8, False))
